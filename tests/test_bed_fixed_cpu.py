"""The integer restatement of the bed fixed-point products (tests/bed_fixed_restatement.py), the parts that need no GPU: the restated
products against the exact rational product within a budget derived from the specification, the digits at their edges, the two
integer conversions past |lo| > 2^53, and the condition under which tests/test_gpu_bed_fixed.py can see a defect at all -- on the very
inputs it uses, a dropped lowest digit and a truncating quantiser each change the bits of at least half of the output entries."""
import math
from fractions import Fraction as F

import numpy as np
import pytest

import bed_fixed_restatement as bx
from gvamp_amd import synth

U = bx.U
_CASES = {}


def _case(name):
    if name not in _CASES:
        cs = bx.case(name)
        cs["planes"] = bx.planes(cs["bed"], cs["N"], cs["M"], cs["present"])
        cs["mave"], cs["msig"] = bx.marker_stats(cs["planes"], cs["nonas"])
        _CASES[name] = cs
    return _CASES[name]


def _fr(v):
    return np.array([F(float(t)) for t in v], dtype=object)


def _inv_sqrt(N):
    """1 / sqrt(N) as a Fraction, relative error < 2^-190"""
    return F(1 << 200, math.isqrt(N << 400))


@pytest.fixture(scope="module")
def small():
    """N = 203 x M = 131: ragged N, ~3 % missing genotypes, ~4 % individuals without a phenotype, a monomorphic and an all-missing marker"""
    N, M = 203, 131
    mb = (N + 3) // 4
    bed = synth.synth_bed(N, M, seed=9, miss_ppm=30000).reshape(M, mb).copy()
    bed[5], bed[17] = 0x00, 0x55
    present = np.random.default_rng(3).random(N) >= 0.04
    pl = bx.planes(bed.reshape(-1), N, M, present)
    mave, msig = bx.marker_stats(pl, int(present.sum()))
    rng = np.random.default_rng(4)
    x = rng.standard_normal(M) * 10.0 ** rng.uniform(-3, 0, M)
    p = np.zeros(4 * mb)
    p[:N] = rng.standard_normal(N) * 10.0 ** rng.uniform(-3, 0, N) * present
    w = _fr(msig) * _fr(x)                                              # msig x, exact
    a, b = pl["a"].astype(object), pl["b"].astype(object)
    ex_ax = (a.T @ w - b.T @ (_fr(mave) * w)) * _inv_sqrt(N)           # sum_m b (a - mave) msig x / sqrt N  (b = 0 at NA rows too)
    ex_atx = _fr(msig) * (a @ _fr(p) - _fr(mave) * (b @ _fr(p))) * _inv_sqrt(N)
    return dict(N=N, M=M, present=present, pl=pl, mave=mave, msig=msig, x=x, p=p, w=w, ex_ax=ex_ax, ex_atx=ex_atx)


def _worst(out, exact, budget):
    ratio = max(float(abs(F(float(o)) - e) / bd) for o, e, bd in zip(out, exact, budget) if bd > 0)
    assert all(abs(F(float(o)) - e) <= bd for o, e, bd in zip(out, exact, budget))
    return ratio


def test_mode1_against_the_exact_rational_product(small):
    """Budget, nothing measured.  g = 2^(E-54) is the grid, every quantised entry is off by at most g / 2 = 2^(E-55).

    Ax at individual n:  the integer sum is  sum_m r' (c + dc) + miss (e + de),  |dc|, |de| <= g / 2:   Q = 2^(E-55) sum_m (r' + miss).
      operands: c = fl(msig x) is off by u |msig x|, weight |a - mave| at a present genotype;  at a missing one 3 c + e - mave c should
      be 0 and is e - (mave - 3) c, at most (2u + u^2) |mave - 3| |c| (fl(mave - 3), then the product):   Op.
      K0 = fl(exact sum): u |K0|.   T = fl(integer) (|lo| <= 2^53, asserted): u |T g|.   y = fl(T g - K0): u |y|.
      out = fl(y post), post = fl(1 / fl(sqrt N)): three roundings, (1 + u)^3 - 1 < 4u of |y| / sqrt N.
    ATx at marker m:  sa = fl(X - 3Y) g = sum a p within Qa = 2^(E-55) sum_n a, plus u |sa|;  sm likewise with Qm over miss;
      Pm = fl(P - sm) with P = fl(exact sum): u |P| + Qm + u |sm| + u |Pm|;   core = fma(-mave, Pm, sa): one rounding u |core| on top of
      err(sa) + mave err(Pm);   out = fl(fl(msig core) post): four roundings with post's two, < 5u of |msig core| / sqrt N."""
    s = small
    N, pl, mave, msig = s["N"], s["pl"], s["mave"], s["msig"]
    isq = _inv_sqrt(N)
    S = bx.ax1_sums(pl, mave, msig, s["x"])
    assert bx.lo_exact(S["lo"])
    K0 = float(bx.exact_K0(mave, S["c"]))
    out = bx.ax1_epilogue(S, K0, N, s["present"])
    g2 = F(2) ** (S["E"] - 55)
    absw, mv = np.array([abs(t) for t in s["w"]], dtype=object), _fr(mave)
    a, b, miss, r = (pl[k].astype(object) for k in ("a", "b", "miss", "r"))
    Q = g2 * (r + miss).sum(axis=0)
    op = np.array([sum(U * abs(int(a[m, n]) - mv[m]) * absw[m] * int(b[m, n]) + (2 * U + U * U) * (1 + U) * abs(mv[m] - 3) * absw[m] * int(miss[m, n])
                       for m in range(s["M"])) for n in range(len(out))], dtype=object)
    Tg = [F(float(t)) * F(bx.result_scale(S["E"])) for t in S["T"]]
    y = [F(float(t) - K0) for t in (S["T"] * bx.result_scale(S["E"]))]
    budget = [(Q[n] + op[n] + U * abs(F(K0)) + U * abs(Tg[n]) + U * abs(y[n])) * isq * (1 + F(1, 2 ** 150)) + 4 * U * abs(y[n]) * isq
              for n in range(len(out))]
    pr = np.concatenate([s["present"], np.zeros(len(out) - N, dtype=bool)])
    assert np.all(out[~pr] == 0) and all(e == 0 for e in s["ex_ax"][~pr])
    print("mode 1 Ax: worst error / budget %.3f" % _worst(out[pr], s["ex_ax"][pr], np.array(budget, dtype=object)[pr]))
    bad = bx.ax1_epilogue(bx.ax1_sums(pl, mave, msig, s["x"], "drop0"), K0, N, s["present"])
    assert any(abs(F(float(o)) - e) > bd for o, e, bd in zip(bad[pr], s["ex_ax"][pr], np.array(budget, dtype=object)[pr]))

    A = bx.atx1_sums(pl, s["p"], N, s["present"])
    assert bx.lo_exact(A["lo"])
    P = float(bx.exact_P(s["p"]))
    w = bx.atx1_epilogue(A, P, mave, msig, N)
    g2 = F(2) ** (A["E"] - 55)
    Qa, Qm = g2 * a.sum(axis=1), g2 * miss.sum(axis=1)
    budget = []
    for m in range(s["M"]):
        sa, sm = F(float(A["sa"][m])), F(float(A["sm"][m]))
        Pm = F(P - float(A["sm"][m]))
        core = F(bx.fma(-float(mave[m]), float(Pm), float(sa)))
        e_pm = U * abs(F(P)) + Qm[m] + U * abs(sm) + U * abs(Pm)
        e_core = Qa[m] + U * abs(sa) + abs(mv[m]) * e_pm + U * abs(core)
        budget.append(F(float(msig[m])) * (e_core * (1 + F(1, 2 ** 150)) + 5 * U * abs(core)) * isq)
    print("mode 1 ATx: worst error / budget %.3f" % _worst(w, s["ex_atx"], budget))
    bad = bx.atx1_epilogue(bx.atx1_sums(pl, s["p"], N, s["present"], "drop0"), P, mave, msig, N)
    assert any(abs(F(float(o)) - e) > bd for o, e, bd in zip(bad, s["ex_atx"], budget))


def test_mode2_against_the_exact_rational_product(small):
    """The residual grid: v = q g + q2 g 2^-54 + d with |d| <= 2^(E-109), so every entry is off by at most G = 2^(E-109) per unit of
    plane weight (a' + b on the Ax side; a' resp. b on the ATx side).

    Ax:  Q = G sum_m (a' + b);  operands: c off by u |msig x| (weight a'), e = -fl(mave c) off from -mave msig x by (2u + u^2)
      |mave msig x| (weight b);  head = fl(H) g, res = fl(R) g 2^-54 and their sum: u (|head| + |res| + |head + res|);  out = fl(. post):
      < 4u of the value / sqrt N.
    ATx: sa, sb each as above without operand terms;  core = fma(-mave, sb, sa): err(sa) + mave err(sb) + u |core|;  out: < 5u."""
    s = small
    N, pl, mave, msig = s["N"], s["pl"], s["mave"], s["msig"]
    isq, big = _inv_sqrt(N), 1 + F(1, 2 ** 150)
    a, b = pl["a"].astype(object), pl["b"].astype(object)
    absw, mv = np.array([abs(t) for t in s["w"]], dtype=object), _fr(mave)
    parts = []
    out = bx.ax2(pl, mave, msig, s["x"], N, s["present"], parts=parts)
    head, res = parts[0]
    c, e = bx.ax_operands(2, mave, msig, s["x"])
    G = F(2) ** (bx.exponent(c, e) - 109)
    Q = G * (a + b).sum(axis=0)
    op = (a.T @ (U * absw)) + (b.T @ ((2 * U + U * U) * np.array([abs(t) for t in mv], dtype=object) * absw))
    budget = []
    for n in range(len(out)):
        h, r_ = F(float(head[n])), F(float(res[n]))
        v = F(float(head[n] + res[n]))
        budget.append((Q[n] + op[n] + U * (abs(h) + abs(r_) + abs(v))) * isq * big + 4 * U * abs(v) * isq)
    pr = np.concatenate([s["present"], np.zeros(len(out) - N, dtype=bool)])
    assert np.all(out[~pr] == 0)
    print("mode 2 Ax: worst error / budget %.3f" % _worst(out[pr], s["ex_ax"][pr], np.array(budget, dtype=object)[pr]))
    bad = bx.ax2(pl, mave, msig, s["x"], N, s["present"], "drop0")
    assert any(abs(F(float(o)) - e_) > bd for o, e_, bd in zip(bad[pr], s["ex_ax"][pr], np.array(budget, dtype=object)[pr]))

    parts = []
    w = bx.atx2(pl, mave, msig, s["p"], N, s["present"], parts=parts)
    (ha, ra), (hb, rb), (sa, sb) = parts
    G = F(2) ** (bx.exponent(s["p"]) - 109)
    Qa, Qb = G * a.sum(axis=1), G * b.sum(axis=1)
    budget = []
    for m in range(s["M"]):
        e_sa = Qa[m] + U * (abs(F(float(ha[m]))) + abs(F(float(ra[m]))) + abs(F(float(sa[m]))))
        e_sb = Qb[m] + U * (abs(F(float(hb[m]))) + abs(F(float(rb[m]))) + abs(F(float(sb[m]))))
        core = F(bx.fma(-float(mave[m]), float(sb[m]), float(sa[m])))
        budget.append(F(float(msig[m])) * ((e_sa + abs(mv[m]) * e_sb + U * abs(core)) * big + 5 * U * abs(core)) * isq)
    print("mode 2 ATx: worst error / budget %.3f" % _worst(w, s["ex_atx"], budget))


def test_digits_recombine_to_q_over_the_whole_range_and_at_the_edges():
    top = 2 ** 54 - 1
    qs = [0, 1, -1, 127, 128, -128, -129, 255, 256, top, -top, 2 ** 53, -2 ** 53, 2 ** 54 - 128, -(2 ** 54 - 129), 0x7F7F7F7F7F7F7F >> 2]
    rng = np.random.default_rng(0)
    qs += [int(t) for t in rng.integers(-top, top, 2000)] + [int(t) for t in rng.integers(-70000, 70000, 500)]
    d = bx.digits(qs)
    assert d.min() >= -128 and d.max() <= 127
    assert [sum(int(d[l, k]) << (8 * l) for l in range(7)) for k in range(len(qs))] == qs
    with pytest.raises(AssertionError):
        bx.digits([2 ** 55])                                     # (|q| < 2^54 is what 7 balanced digits hold, with one bit to spare)

    # a power-of-two amax and its predecessor sit in different exponents, and both quantise to |q| < 2^54
    assert bx.exponent([8.0]) == 4 and bx.exponent([math.nextafter(8.0, 0.0)]) == 3
    assert bx.quantise([8.0, -8.0], 4) == [2 ** 53, -2 ** 53]
    assert bx.quantise([math.nextafter(8.0, 0.0)], 3) == [2 ** 54 - 2]
    assert bx.quantise([8.0, 8.0 * (1 - 2.0 ** -53)], 4) == [2 ** 53, 2 ** 53 - 1]
    v = np.random.default_rng(1).standard_normal(300) * 10.0 ** np.random.default_rng(2).uniform(-9, 3, 300)
    E = bx.exponent(v)
    assert 2.0 ** (E - 1) <= np.max(np.abs(v)) < 2.0 ** E and max(abs(t) for t in bx.quantise(v, E)) < 2 ** 54
    assert bx.exponent(np.zeros(3)) is None and bx.quantise([0.0, -0.0], None) == [0, 0] and bx.result_scale(None) == 0.0
    assert math.isnan(bx.exponent([1.0, math.inf])) and math.isnan(bx.exponent([math.nan])) and math.isnan(bx.result_scale(math.nan))

    # exact ties go to the even neighbour, both parities and signs; the flush threshold is 2^(E-55) = half a grid step
    g = 2.0 ** (4 - 54)
    ks = [0, 1, 2, 3, 2 ** 40, 2 ** 40 + 1]
    assert bx.quantise([(k + 0.5) * g for k in ks], 4) == [k if k % 2 == 0 else k + 1 for k in ks]
    assert bx.quantise([-(k + 0.5) * g for k in ks], 4) == [-(k if k % 2 == 0 else k + 1) for k in ks]
    assert bx.quantise([(k + 0.5) * g for k in ks], 4, "trunc") == ks
    half = 0.5 * g
    assert half == 2.0 ** (4 - 55)
    assert bx.quantise([math.nextafter(half, 0.0), half, math.nextafter(half, 1.0), -math.nextafter(half, 1.0), 2.0 ** (4 - 60), -0.0], 4) == \
        [0, 0, 1, -1, 0, 0]
    # the hand-built vectors of the GPU tests carry every one of these
    for name in bx.SHAPES:
        cs = _case(name)
        p = bx.vector_p(cs, 3)
        ops = [p] + [np.concatenate(bx.ax_operands(mode, cs["mave"], cs["msig"], bx.vector_x(cs, 3, mode, cs["mave"], cs["msig"])))
                     for mode in (1, 2)]
        for v in ops:
            E = bx.exponent(v)
            fr = [F(float(t)) * F(2) ** (54 - E) for t in v]
            ties = [t for t in fr if t.denominator == 2]
            assert {int(t - F(1, 2)) % 2 for t in ties if t > 0} == {0, 1} and any(t < 0 for t in ties)
            assert any(0 < abs(t) < F(1, 2) for t in fr) and any(F(1, 2) < abs(t) < 1 for t in fr)
            assert np.max(np.abs(v)) == 2.0 ** (E - 1) and any(abs(t) == 2 ** 53 - 1 for t in fr)
            assert any(t == 0 and math.copysign(1.0, t) < 0 for t in v)


def test_recombination_converts_hi_and_lo_separately():
    """Column sums s3 = 2^29, s0 = 1, s4 = -2^20: lo = 2^53 + 1 is not a double, fl(lo) = 2^53 (tie to even), hi 2^32 = -2^52, so the
    kernel's fl(fl(hi) 2^32 + fl(lo)) = 2^52 where the exact integer 2^52 + 1 IS a double: two roundings, not one.

    Reachable in the worst case only: |lo| <= W K 128 (1 + 2^8 + 2^16 + 2^24) with W the plane weight of a K-entry -- 2 for the X - 3Y
    of ATx (K = N individuals: N > 2 088 960; gv_set_dims admits N < 5 592 405), 4 for the Ax plane r' c + miss e (K = M markers of
    one shard: M > 1 044 480) -- and needs every low digit at -128 on genotypes of top weight.  The digits of a real vector have random
    signs: |lo| ~ sqrt(K) 74 W 2^24, 2^42 at K = 10^6, eleven bits under the limit (|lo| < 2^38 on the shapes of the GPU tests)."""
    s = np.zeros((7, 2), dtype=np.int64)
    s[3, 0], s[0, 0], s[4, 0] = 2 ** 29, 1, -2 ** 20
    s[:, 1] = [5, -7, 100, 2 ** 20, -3, 9, 1]                     # an ordinary row: |lo| < 2^53, both forms agree
    hi, lo = bx.combine(s)
    assert (hi[0], lo[0]) == (-2 ** 20, 2 ** 53 + 1) and not bx.lo_exact(lo) and bx.lo_exact(lo[1:])
    exact = hi[0] * 2 ** 32 + lo[0]
    assert exact == 2 ** 52 + 1 and float(exact) == exact
    assert bx.convert(hi[0], lo[0]) == 2.0 ** 52 and bx.convert(hi[0], lo[0], "one") == 2.0 ** 52 + 1
    assert bx.convert(hi[1], lo[1]) == bx.convert(hi[1], lo[1], "one") == float(hi[1] * 2 ** 32 + lo[1])
    assert 2 ** 53 // (256 * bx.WEIGHT) == 2088960 and 2 ** 53 // (512 * bx.WEIGHT) == 1044480


def _base(name):
    """the unmodified restatement on the inputs of tests/test_gpu_bed_fixed.py, vectors 1..3 (vector 4 is all zero: nothing to change)"""
    key = ("base", name)
    if key not in _CASES:
        cs = _case(name)
        N, pl, mave, msig, pres = cs["N"], cs["planes"], cs["mave"], cs["msig"], cs["present"]
        rows = []
        for kind in (1, 2, 3):
            p = bx.vector_p(cs, kind)
            x1, x2 = (bx.vector_x(cs, kind, mode, mave, msig) for mode in (1, 2))
            S, A = bx.ax1_sums(pl, mave, msig, x1), bx.atx1_sums(pl, p, N, pres)
            K0, P = float(np.sum(mave * S["c"])), float(np.sum(p))     # numpy's pairwise order: neither the exact sum nor the device's order
            rows.append(dict(kind=kind, p=p, x1=x1, x2=x2, S=S, A=A, K0=K0, P=P, z=bx.ax1_epilogue(S, K0, N, pres),
                             w=bx.atx1_epilogue(A, P, mave, msig, N), z2=bx.ax2(pl, mave, msig, x2, N, pres),
                             w2=bx.atx2(pl, mave, msig, p, N, pres)))
        _CASES[key] = rows
    return _CASES[key]


@pytest.mark.parametrize("name", list(bx.SHAPES))
def test_the_unmodified_restatement_passes_the_free_scalar_procedure_with_every_entry_compared(name):
    """K0 / P summed in another order than the exact sum: the procedure finds it, with all npad resp. M entries compared (find_scalar
    evaluates whole arrays: no entry is left out), and it is inside its bound"""
    cs = _case(name)
    N, mave, msig, pres = cs["N"], cs["mave"], cs["msig"], cs["present"]
    for b in _base(name):
        rk = bx.find_K0(b["S"], b["z"], N, pres)
        assert len(b["z"]) == cs["npad"] and rk.contains(b["K0"])
        assert abs(F(b["K0"]) - bx.exact_K0(mave, b["S"]["c"])) <= bx.k0_bound(mave, b["S"]["c"])
        rp = bx.find_P(b["A"], b["w"], mave, msig, N, bx.MONO)
        assert len(b["w"]) == cs["M"] and rp.contains(b["P"]) and abs(F(b["P"]) - bx.exact_P(b["p"])) <= bx.p_bound(b["p"], N)
        print("%s vector %d: K0 %d pinned / %d reproduce every entry (%+.2f ulp from the exact sum), P %d / %d (%+.2f ulp)"
              % (name, b["kind"], rk.pinned, rk.count, bx.ulps(b["K0"], bx.exact_K0(mave, b["S"]["c"])), rp.pinned, rp.count,
                 bx.ulps(b["P"], bx.exact_P(b["p"]))))
        for r in (rk, rp):                              # the run is exactly the set: its members pass, its two neighbours do not
            assert r.count < 64
        assert all(np.array_equal(bx.ax1_epilogue(b["S"], k, N, pres), b["z"]) for k in rk.members())
        assert not any(np.array_equal(bx.ax1_epilogue(b["S"], math.nextafter(k, d), N, pres), b["z"])
                       for k, d in ((rk.members()[0], -math.inf), (rk.members()[-1], math.inf)))
        if b["kind"] == 1:                              # the lmmse_mult form of the epilogue as the GPU test runs it: ATx of z = Ax(x)
            A2, P2, lm = bx.atx1_sums(cs["planes"], b["z"], N, pres), float(np.sum(b["z"])), (1.3, 0.4, b["x1"])
            out = bx.lmmse(1.3, bx.atx1_epilogue(A2, P2, mave, msig, N), 0.4, b["x1"])
            rl = bx.find_P(A2, out, mave, msig, N, bx.MONO, lm)
            print("%s lmmse_mult: P %d pinned / %d reproduce every entry" % (name, rl.pinned, rl.count))
            assert rl.contains(P2)
            for k in (bx._unkey(rl.k0), bx._unkey(rl.k1 - 1)):
                assert np.array_equal(bx.lmmse(1.3, bx.atx1_epilogue(A2, k, mave, msig, N), 0.4, b["x1"]), out)
            for k in (bx._unkey(rl.k0 - 1), bx._unkey(rl.k1)):
                assert not np.array_equal(bx.lmmse(1.3, bx.atx1_epilogue(A2, k, mave, msig, N), 0.4, b["x1"]), out)


@pytest.mark.parametrize("variant", ["drop0", "trunc"])
@pytest.mark.parametrize("name", list(bx.SHAPES))
def test_the_gpu_inputs_can_see_a_dropped_digit_and_a_truncating_quantiser(name, variant):
    """The condition under which tests/test_gpu_bed_fixed.py sees the defect, on its own inputs (same seeds and shapes; mave / msig
    as float64 numpy gives them): of the output entries of each product over the vectors 1..3, the defect changes the bits of at least
    half; on every single vector it changes some; and no double K0 / P makes a defective mode-1 output pass the free-scalar procedure.

    One pair cannot meet "half", whatever the inputs, and is held to "some entries of every vector" instead (the GPU test compares
    every entry with array_equal, so one changed entry fails it): a TRUNCATING quantiser in MODE 2.  The residual of mode 2 is
    v - q g for whatever q the head took, so it absorbs a truncated head exactly; what is left is the truncation of the second level
    at 2^(E-108), far below an ulp of the result, and only the double roundings of fl(H), fl(R) and head + res flip some last bits
    (4 - 52 % of the entries of a vector here, printed below).  In mode 1 the same defect shifts every sum by ~sqrt(K) / 2 grid units on
    ~sqrt(K) 2^53, about half an ulp: the fraction per vector sits between 49 % and 97 %, per product it is above half."""
    cs = _case(name)
    N, pl, mave, msig, pres = cs["N"], cs["planes"], cs["mave"], cs["msig"], cs["present"]
    npres, M = int(pres.sum()), cs["M"]
    total = np.zeros(4, dtype=np.int64)
    for b in _base(name):
        zb = bx.ax1_epilogue(bx.ax1_sums(pl, mave, msig, b["x1"], variant), b["K0"], N, pres)
        wb = bx.atx1_epilogue(bx.atx1_sums(pl, b["p"], N, pres, variant), b["P"], mave, msig, N)
        z2b, w2b = bx.ax2(pl, mave, msig, b["x2"], N, pres, variant), bx.atx2(pl, mave, msig, b["p"], N, pres, variant)
        changed = np.array([np.sum(zb != b["z"]), np.sum(wb != b["w"]), np.sum(z2b != b["z2"]), np.sum(w2b != b["w2"])])
        print("%s vector %d, %s changes %d / %d (Ax 1), %d / %d (ATx 1), %d / %d (Ax 2), %d / %d (ATx 2)"
              % (name, b["kind"], variant, changed[0], npres, changed[1], M, changed[2], npres, changed[3], M))
        assert np.all(changed > 0)
        assert bx.find_K0(b["S"], zb, N, pres).count == 0 and bx.find_P(b["A"], wb, mave, msig, N, bx.MONO).count == 0
        total += changed
    assert 2 * total[0] >= 3 * npres and 2 * total[1] >= 3 * M
    if variant == "drop0":
        assert 2 * total[2] >= 3 * npres and 2 * total[3] >= 3 * M
