"""tests/student_t_reference.py has to earn its place as a yardstick: exact and closed-form values at nu = 1 and 2, agreement with
itself at twice the working precision, monotonicity in t, the interleaving of even and odd nu (two different formulas), and scipy
at moderate arguments."""
import math
from decimal import Decimal, localcontext
from fractions import Fraction

import pytest

import student_t_reference as st

NUS = (1, 2, 3, 4, 5, 8, 13, 28, 29, 30, 59, 60, 126, 127, 4000, 4001)
WS = (1e-10, 1e-4, 0.05, 0.42, 1.0, 30.0, 1e3, 1e5)


def rel(a, b):
    """|a - b| / |b| in 120 digits (the default decimal context has 28); a: Decimal, b: Decimal or Fraction"""
    with localcontext() as ctx:
        ctx.prec = 120
        if isinstance(b, Fraction):
            b = Decimal(b.numerator) / Decimal(b.denominator)
        return abs(a - b) / abs(b)


def test_exact_values():
    """nu = 1: tail(1) = 1/2.  nu = 2: tail = 1 - t / sqrt(2 + t^2), rational where 2 + t^2 is a square: t = 1/2, 7/4, 31/8"""
    assert rel(st.tail(1.0, 1), Fraction(1, 2)) < Decimal("1e-70")
    for t, want in ((0.5, Fraction(2, 3)), (1.75, Fraction(2, 9)), (3.875, Fraction(2, 33))):
        assert rel(st.tail(t, 2), want) < Decimal("1e-70"), t
    for nu in NUS:
        assert st.tail(0.0, nu) == 1
        assert st.tail(-1.25, nu) == st.tail(1.25, nu)


def test_closed_forms_in_float64_written_without_the_complement():
    """nu = 1: 1 - 2 atan(t) / pi = 2 atan(1 / t) / pi.  nu = 2: 1 - s = (1 - s^2) / (1 + s) with s = t / sqrt(2 + t^2), 1 - s^2 = 2 / (2 + t^2).
    Neither form cancels, so float64 holds them to a few ulps at every t"""
    for t in (1e-9, 1e-3, 0.3, 1.0, 2.5, 40.0, 1e4, 1e9):
        assert math.isclose(float(st.tail(t, 1)), 2 * math.atan2(1.0, t) / math.pi, rel_tol=1e-15), t
        s = t / math.sqrt(2 + t * t)
        assert math.isclose(float(st.tail(t, 2)), 2 / ((2 + t * t) * (1 + s)), rel_tol=1e-15), t


def test_agrees_with_itself_at_twice_the_working_precision():
    deep = 0
    for nu in NUS:
        for w in WS:
            t = math.sqrt(w * nu)
            p1 = st.tail(t, nu)
            if p1 is None:
                assert st.digits_needed(t, nu) > st.MAX_DIGITS
                continue
            assert 0 < p1 <= 1
            assert rel(p1, st.tail(t, nu, scale=2)) < Decimal("1e-40"), (nu, w)
            deep += p1 < Decimal("1e-100")
    assert deep >= 6                           # (the cancellation the working precision is there for was exercised)


def test_none_only_below_the_double_range():
    """the cut: 63.5 * log10(1 + w) > 340 at nu = 126"""
    assert st.tail(math.sqrt(126 * 2.2e5), 126) is not None and st.tail(math.sqrt(126 * 2.4e5), 126) is None
    assert st.tail(math.sqrt(126 * 2.2e5), 126) < Decimal("1e-330")


def test_monotone_in_t():
    for nu in (1, 2, 3, 28, 29, 60, 127, 4000):
        ts = [math.sqrt(w * nu) * f for w in WS for f in (1.0, 1.0 + 2.0 ** -40, 1.5)]
        ps = [st.tail(t, nu) for t in sorted(ts)]
        ps = [p for p in ps if p is not None]
        assert len(ps) >= 9 and all(a > b for a, b in zip(ps, ps[1:])), nu


def test_even_and_odd_nu_interleave():
    """heavier tails at fewer degrees of freedom: tail(t, nu - 1) > tail(t, nu) > tail(t, nu + 1); the neighbours of an even nu come
    from the other formula"""
    for nu in (2, 3, 4, 5, 28, 29, 30, 60, 61, 126, 4000):
        for t in (1e-6, 0.1, 1.0, 3.0, 12.0, 37.0, 300.0)[:6 if nu > 1000 else 7]:      # (t = 300 at nu = 4000 is below the double range)
            lo, mid, hi = st.tail(t, nu + 1), st.tail(t, nu), st.tail(t, nu - 1)
            assert lo < mid < hi, (nu, t)
    # and the gap closes as it must: d/dnu of the tail at large nu is O(1 / nu^2) of it for a fixed t
    a, b, c = (st.tail(2.0, nu) for nu in (3999, 4000, 4001))
    with localcontext() as ctx:
        ctx.prec = 120
        assert rel(a - b, b - c) < Decimal("2e-3")


def test_against_scipy_at_moderate_arguments():
    """a sanity check, not a yardstick: scipy itself is off by up to 2e-13 at nu = 4000"""
    stats = pytest.importorskip("scipy.stats")
    worst = 0.0
    for nu in (1, 2, 3, 4, 5, 8, 13, 28, 29, 30, 60, 61, 126, 127):
        for t in (1e-6, 1e-2, 0.5, 1.0, 2.0, 3.5, 6.0, 10.0):
            got, want = float(st.tail(t, nu)), 2 * float(stats.t.sf(t, nu))
            worst = max(worst, abs(got / want - 1))
            assert math.isclose(got, want, rel_tol=1e-12), (nu, t, got, want)
    print("worst relative difference from 2 * scipy.stats.t.sf: %.2e" % worst)
