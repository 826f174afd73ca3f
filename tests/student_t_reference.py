"""Two-sided tail of Student's t distribution, P(|T_nu| > |t|), for an integer nu >= 1, in decimal arithmetic of as many digits as the
tail needs -- the yardstick of tests/test_gpu_assoc_plane.py, checked by tests/test_student_t_reference_cpu.py.

The finite closed forms of Abramowitz & Stegun 26.7.3 / 26.7.4 with theta = atan(t / sqrt(nu)), cos^2 theta = nu / (nu + t^2),
sin theta = t / sqrt(nu + t^2):
    nu even:  1 - sin theta * sum_{k=0}^{nu/2-1} [C(2k, k) / 4^k] cos^{2k} theta
    nu odd :  1 - (2 / pi) (theta + sin theta * sum_{k=0}^{(nu-3)/2} [(2k)!! / (2k+1)!!] cos^{2k+1} theta),    nu = 1: 1 - 2 theta / pi
No incomplete beta function, no lgamma, no continued fraction: nothing here is shared with the library (gv_pval_dev.h), the oracle or
tests/assoc_restatement.py.  pi is Machin's 16 atan(1/5) - 4 atan(1/239); atan halves its argument, x -> x / (1 + sqrt(1 + x^2)),
until the Taylor series converges fast.  Standard library only.

Working precision.  The complement cancels every leading digit of a small tail, and the tail is about (1 + w)^-((nu+1)/2) with
w = t^2 / nu, so 80 + ceil((nu + 1)/2 * log10(1 + w)) digits leave about 80 good ones.  Where that exceeds 420 the tail is below
1e-330, far under the smallest double: tail() returns None ("below the double range")."""
import functools
import math
from decimal import Decimal, localcontext

GUARD_DIGITS = 80
MAX_DIGITS = 420


def digits_needed(t, nu):
    w = float(t) * float(t) / nu
    return GUARD_DIGITS + int(math.ceil(0.5 * (nu + 1) * math.log1p(w) / math.log(10.0)))


def _atan_series(x):
    """Taylor series of atan for |x| small (in the current context)"""
    x2, term, total, k = x * x, x, x, 0
    while True:
        k += 1
        term = -term * x2
        add = term / (2 * k + 1)
        if total + add == total:
            return total
        total += add


def _atan(x):
    """atan of a Decimal x >= 0 in the current context: the argument halved until it is below 2^-10, then the series"""
    halvings = 0
    while x > Decimal(1) / 1024:
        x = x / (1 + (1 + x * x).sqrt())
        halvings += 1
    return _atan_series(x) * (2 ** halvings)


def _pi():
    return 16 * _atan_series(Decimal(1) / 5) - 4 * _atan_series(Decimal(1) / 239)


@functools.lru_cache(maxsize=None)
def _tail(t, nu, scale):
    digits = digits_needed(t, nu)
    if digits > MAX_DIGITS:
        return None
    with localcontext() as ctx:
        ctx.prec = digits * scale + 10
        td = Decimal(t)                                      # (exact: every double is a finite decimal)
        r2 = nu + td * td
        c2 = Decimal(nu) / r2
        sin = td / r2.sqrt()
        if nu % 2 == 0:
            term = total = Decimal(1)
            for k in range(1, nu // 2):
                term = term * c2 * (2 * k - 1) / (2 * k)
                total += term
            p = 1 - sin * total
        else:
            theta = _atan(td / Decimal(nu).sqrt())
            inner = theta
            if nu > 1:
                term = total = c2.sqrt()
                for k in range(1, (nu - 1) // 2):
                    term = term * c2 * (2 * k) / (2 * k + 1)
                    total += term
                inner = theta + sin * total
            p = 1 - 2 * inner / _pi()
        ctx.prec = digits * scale
        return +p


def tail(t, nu, scale=1):
    """P(|T_nu| > |t|) as a Decimal good to about 80 digits, or None where it is below 1e-330.  t: a finite float; nu: an integer >= 1.
    scale: a multiple of the working precision (the CPU test compares scale 2 with scale 1)."""
    t = abs(float(t))
    if nu != int(nu) or nu < 1 or not math.isfinite(t):
        raise ValueError("tail: t finite and nu an integer >= 1, not %r, %r" % (t, nu))
    return _tail(t, int(nu), int(scale))
