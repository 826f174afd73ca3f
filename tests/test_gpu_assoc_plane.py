"""gvp::t_two_sided (gv_pval_dev.h) over the whole (nu, w = t^2 / nu) plane, and the association test at small per-marker sample
sizes, through the three kernels that inline it: k_pvals_test (kernel mode 0), k_fin_pvals (modes 1 and 2, both resident layouts)
and k_dosage_assoc.  The yardstick of p is tests/student_t_reference.py (decimal arithmetic, finite closed forms), evaluated AT THE
DEVICE'S OWN t, so that the conditioning of t does not enter; beta, se and t are held to the long-double restatement by the rule of
tests/test_gpu_assoc.py.

The grid.  On bed data the sample size of marker k is the number of its present genotypes among the phenotyped individuals, so one
small bed reaches every integer nu = n_k - 2.  In leave-one-out the marker's own effect is added back analytically, so x1_hat[k]
sets the marker's t alone: with v the standardised column and e = y - z1 over the marker's present, phenotyped entries, S_vv, S_ve,
S_ee their centred sums, alpha = S_ve / S_vv and S_perp = S_ee - alpha S_ve,
    x1_hat[k] = (-alpha +- sqrt(w S_perp / S_vv)) sqrt(N)
gives t^2 / nu = w up to rounding (signs alternate).  Every coverage condition below is computed from what the device returned.
The masked parametrisation takes N = 149, the smallest N with 128 phenotyped individuals when every 7th from 3 on is masked: the
counts among the phenotyped are those of the unmasked case (N = 128), and every masked individual carries a present genotype that
must not count.

The bar on p, an error budget and no measurement of the code: for p_ref >= 1e-290, |p / p_ref - 1| <= 2^-52 (1024 + 16 |ln p_ref|).
16 |ln p|: the products a log1p(w) and T ln x, log1p itself and the argument of exp each contribute about an ulp of a quantity no
larger than |ln p|; four times that.  1024: two lgamma calls of magnitude up to 71 at an assumed 4 ulp each (568), the Lentz
products (about 200), the rest.  Below 1e-290, or where the reference is below the double range: 0 <= p <= 1e-289.

Worst share of that envelope per region, as printed by the tests on an MI355X (a host compilation of the header stays below 9 %):
    direct fraction, a < 15            0.023   nu 28,    w 1e3,   p 1.5e-43   (rel err 1.3e-14)
    complement fraction, a < 15        0.043   nu 29,    w 0.05,  p 0.24      (rel err 1.0e-14)
    expansion, 15 <= a < 30 (lgamma)   0.032   nu 57,    w 0.415, p 9.5e-6    (rel err 8.5e-15)
    expansion, a >= 30, small samples  0.024   nu 126,   w 0.41,  p 5.1e-11   (rel err 7.5e-15)
    expansion, a >= 30, N = 20000      0.082   nu 19997, w 0.062, p 6.1e-263  (rel err 1.9e-13)
    fraction, a >= 15 and w > 0.42     0.038   nu 126,   w 30,    p 8.0e-96   (rel err 3.8e-14)
The three kernels give the same figures where they meet the same t (dosage data: 0.032 at most).  The lgamma band is no worse than
its neighbours: the 4 ulp assumed for the GPU's lgamma are not used up.

What the module found when it was written: with two present genotypes beta came out finite, t as NaN from kernel mode 0 and as -0.0
from modes 1 and 2 on the same data, and a marker monomorphic among its present genotypes got beta = -inf from modes 1 and 2 (NaN
from mode 0) -- sxy / 0 with sxy a rounding error of the fixed-point sums.  gvp::marker_stats now returns NaN in all four outputs
for n < 3 and for sumsqx == 0.
"""
import functools
import math
from decimal import Decimal, localcontext

import numpy as np
import pytest

import assoc_restatement as ar
import dosage_na_restatement as dr
import student_t_reference as st
import test_gpu_assoc as tga
from gvamp_amd import capi

pytestmark = pytest.mark.gpu
LD = np.longdouble
KEYS = tga.KEYS

NUS = (1, 2, 3, 4, 5, 8, 13, 26, 27, 28, 29, 30, 31, 32, 57, 58, 59, 60, 61, 62, 63, 126)
WS = (1e-10, 1e-4, 0.05, 0.3, 0.40, 0.41, 0.415, 0.42, 0.425, 0.43, 0.44, 0.6, 1.0, 4.0, 30.0, 1e3, 1e5)
WS_DOSAGE = (1e-4, 0.41, 0.43, 4.0, 1e3)
SEAM_NUS = (28, 30, 58, 60, 126)
REGIONS = ("direct fraction, a < 15", "complement fraction, a < 15", "expansion, 15 <= a < 30", "expansion, a >= 30",
           "fraction, a >= 15 and w > 0.42")
DEGENERATE = ("n = 0", "n = 1", "n = 2, two genotypes", "n = 2, one genotype", "n = 40, monomorphic")
P_FLOOR = 1e-290          # below it p is held to 0 <= p <= P_CAP
P_CAP = 1e-289


# ---- the yardstick of p ------------------------------------------------------------------------------------------------------------
def region(t, nu):
    """which evaluation gvp::t_two_sided takes: its own expressions, in float64"""
    a, w = 0.5 * nu, t * t / nu
    if a >= 15.0 and w <= 0.42:
        return 2 if a < 30.0 else 3
    if a >= 15.0:
        return 4
    return 0 if 1.0 / (1.0 + w) < (a + 1.0) / (a + 0.5 + 2.0) else 1


def envelope(p_ref):
    return 2.0 ** -52 * (1024.0 + 16.0 * abs(math.log(p_ref)))


def p_against_reference(p, t, n, rows, what):
    """assertion 2: p[rows] against tail(|t|, n - 2); prints the worst share of the envelope per region, then asserts.  Returns the
    reference values as floats (0.0 where below the double range)"""
    worst, where, bad, pref = [0.0] * 5, [None] * 5, [], {}
    for k in rows:
        nu, tk, pk = int(n[k]) - 2, float(t[k]), float(p[k])
        assert math.isfinite(tk) and tk != 0.0 and nu >= 1, (what, k, tk, nu)
        ref = st.tail(tk, nu)
        pref[k] = 0.0 if ref is None else float(ref)
        if ref is None or ref < Decimal(P_FLOOR):
            if not 0.0 <= pk <= P_CAP:
                bad.append((k, nu, tk, pk, "below 1e-290: 0 <= p <= 1e-289"))
            continue
        with localcontext() as ctx:
            ctx.prec = 50
            err = float(abs(Decimal(pk) - ref) / ref) if math.isfinite(pk) else math.inf
        share = err / envelope(float(ref))
        r = region(tk, nu)
        if not share <= worst[r]:
            worst[r], where[r] = share, (nu, tk * tk / nu, float(ref), err)
        if not share <= 1.0:
            bad.append((k, nu, tk, pk, "rel err %.3e, envelope %.3e, region '%s'" % (err, envelope(float(ref)), REGIONS[r])))
    for r in range(5):
        if where[r] is not None:
            print("%s | %-32s worst share of the envelope %.4f  at nu %d w %.4g p %.3e (rel err %.3e)" % ((what, REGIONS[r], worst[r]) + where[r]))
    assert not bad, (what, bad[:8])
    return pref


def coverage(t, n, rows, pref, what, per_region, per_seam_side, w_span):
    """assertion 1, from the device's own t and n: markers on either side of w = 0.42 at the seam nu, w below and above w_span at
    every nu, markers per region of t_two_sided, and an in-range p below 1e-100"""
    nu = {k: int(n[k]) - 2 for k in rows}
    w = {k: float(t[k]) ** 2 / nu[k] for k in rows}
    for s in SEAM_NUS:
        below = sum(1 for k in rows if nu[k] == s and 0.38 < w[k] <= 0.42)
        above = sum(1 for k in rows if nu[k] == s and 0.42 < w[k] < 0.46)
        assert below >= per_seam_side and above >= per_seam_side, (what, "seam w = 0.42 at nu", s, below, above)
    for s in NUS:
        ws = [w[k] for k in rows if nu[k] == s]
        assert ws and min(ws) < w_span[0] and max(ws) > w_span[1], (what, s, ws)
    counts = [0] * 5
    for k in rows:
        counts[region(float(t[k]), nu[k])] += 1
    print("%s | markers per region %s" % (what, counts))
    assert min(counts) >= per_region, (what, dict(zip(REGIONS, counts)))
    assert any(P_FLOOR <= pref[k] < 1e-100 for k in rows), what


def held_to_the_restatement(got, ref, ref64, what, dead, pref):
    """assertion 3: tests/test_gpu_assoc.py::check -- beta, se, t within 16 x the float64 restatement's own deviation from long double,
    never less than 1e-12 (and its p bar, rtol 1e-8, on top of the envelope) -- on every row but the degenerate ones (`dead`).  The
    rows whose p is below 1e-290 (a subnormal p has no relative accuracy to hold) get the same rule for beta, se and t alone"""
    under = np.array([k for k in pref if pref[k] < P_FLOOR], dtype=np.int64)
    tga.check(got, ref, ref64, what, skip=np.concatenate([np.asarray(dead, dtype=np.int64), under]))
    if under.size == 0:
        return

    def sub(d):
        return {k: np.asarray(d[k])[under] for k in ("beta", "se", "t")}

    dev64, devg = tga.deviation(sub(ref64), sub(ref)), tga.deviation(sub(got), sub(ref))
    for k in ("beta", "se", "t"):
        print("%s, %d rows with p < 1e-290: %-4s float64 dev %.3e  GPU dev %.3e" % (what, under.size, k, dev64[k], devg[k]))
        assert devg[k] <= max(16.0 * dev64[k], 1e-12), (what, k, devg[k], dev64[k])


def not_nan(res, rows):
    """the entries of the four outputs at `rows` that are not NaN"""
    return [(k, key, float(res[key][k])) for k in rows for key in KEYS if not np.isnan(res[key][k])]


# ---- the construction --------------------------------------------------------------------------------------------------------------
def effect_for(v, e, w, sign, N):
    """x1_hat of the module docstring, in long double; v, e over the marker's present, phenotyped entries"""
    v, e = np.asarray(v, dtype=LD), np.asarray(e, dtype=LD)
    vc, ec = v - v.mean(), e - e.mean()
    svv, sve, see = (vc * vc).sum(), (vc * ec).sum(), (ec * ec).sum()
    alpha = sve / svv
    sperp = see - alpha * sve
    assert svv > 0 and sperp > 0
    return float((-alpha + sign * np.sqrt(LD(w) * sperp / svv)) * np.sqrt(LD(N)))


def pack_bed(G, have):
    """hard calls and presence flags (M x N) -> PLINK 2-bit rows: 2 -> 00, missing -> 01, 1 -> 10, 0 -> 11; the padding is 00"""
    M, N = G.shape
    mb = (N + 3) // 4
    code = np.zeros((M, 4 * mb), dtype=np.uint8)
    code[:, :N] = np.where(have, np.choose(G, [3, 2, 0]), 1)
    c = code.reshape(M, mb, 4)
    return (c[:, :, 0] | (c[:, :, 1] << 2) | (c[:, :, 2] << 4) | (c[:, :, 3] << 6)).astype(np.uint8).reshape(-1)


def host_marker_stats(G, have, na):
    """k_marker_stats, count form: mave and msig of the device, from the counts"""
    P = have & (na != 0)[None, :]
    n2, n1, n0 = (((G == g) & P).sum(axis=1).astype(np.float64) for g in (2, 1, 0))
    cnt = n0 + n1 + n2
    mu = np.where(cnt != 0, (2.0 * n2 + n1) / np.where(cnt != 0, cnt, 1.0), 0.0)
    ssq = n2 * (2.0 - mu) ** 2 + n1 * (1.0 - mu) ** 2 + n0 * mu ** 2
    sg = np.where(ssq != 0, 1.0 / np.sqrt(np.where(ssq != 0, ssq, 1.0) / (na.sum() - 1.0)), 1.0)
    return mu, sg, cnt.astype(np.int64)


def na_mask(N, masked):
    na = np.ones(N)
    if masked:
        na[3::7] = 0.0
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    for i in np.nonzero(na)[0]:
        m4[i >> 2] |= 1 << (i & 3)
    return na, m4, int(na.sum())


def bed_rows(rng, counts, ph, N, masked_ix, degenerate):
    """genotypes of one row per entry of `counts` (present genotypes among the phenotyped individuals `ph`), never monomorphic, then
    the degenerate rows; a present genotype at every masked individual"""
    M = len(counts) + (len(DEGENERATE) if degenerate else 0)
    G, have = np.zeros((M, N), dtype=np.int64), np.zeros((M, N), dtype=bool)
    for k, n in enumerate(counts):
        who = ph[rng.permutation(ph.size)[:n]] if n < ph.size else ph
        g = rng.integers(0, 3, who.size)
        if np.all(g == g[0]):
            g[0] = (g[0] + 1) % 3
        G[k, who], have[k, who] = g, True
    if degenerate:
        k = len(counts)
        G[k + 1, ph[5]], have[k + 1, ph[5]] = 2, True
        G[k + 2, ph[[7, 90]]], have[k + 2, ph[[7, 90]]] = [0, 1], True
        G[k + 3, ph[[8, 91]]], have[k + 3, ph[[8, 91]]] = 2, True
        G[k + 4, ph[20:60]], have[k + 4, ph[20:60]] = 1, True
    if masked_ix.size:
        G[:, masked_ix], have[:, masked_ix] = rng.integers(0, 3, (M, masked_ix.size)), True
    return G, have


def bed_inputs(N, masked, counts, targets, degenerate, seed):
    """bed, mask, y, z1 = 0, x1_hat and the restatement's results (long double and float64) of one bed case"""
    rng = np.random.default_rng(seed)
    na, m4, nonas = na_mask(N, masked)
    ph = np.nonzero(na)[0]
    G, have = bed_rows(rng, counts, ph, N, np.nonzero(na == 0)[0], degenerate)
    M = G.shape[0]
    npad = 4 * ((N + 3) // 4)
    y, z1 = np.zeros(npad), np.zeros(npad)
    y[ph] = rng.standard_normal(ph.size)
    mave, msig, cnt = host_marker_stats(G, have, na)
    assert np.array_equal(cnt[:len(counts)], counts)
    V, b = ar.bed_columns(G, have, mave, msig)
    x1 = np.full(M, 0.7 * math.sqrt(N))
    for k, w in enumerate(targets):
        at = have[k] & (na != 0)
        x1[k] = effect_for(V[k, at], y[:N][at], w, 1.0 if k % 2 == 0 else -1.0, N)
    ref = ar.assoc(V, b, na, y, z1, x1)
    ref64 = ar.assoc(*ar.bed_columns(G, have, mave, msig, dtype=np.float64), na, y, z1, x1, dtype=np.float64, with_p=False)
    ref64["p"] = np.zeros(M)
    bed = pack_bed(G, have)
    for a in (bed, y, z1, x1, cnt):
        a.setflags(write=False)
    return dict(N=N, M=M, bed=bed, m4=m4, nonas=nonas, masked=masked, y=y, z1=z1, x1=x1, cnt=cnt, mave=mave, msig=msig, ref=ref, ref64=ref64,
                alive=np.arange(len(counts)), dead=np.arange(len(counts), M))


@functools.lru_cache(maxsize=None)
def small_case(masked):
    counts = np.array([nu + 2 for nu in NUS for _ in WS])
    targets = [w for _ in NUS for w in WS]
    return bed_inputs(149 if masked else 128, masked, counts, targets, True, 7)


PATHS = {"mode 0, raw rows": (True, 1, 0), "mode 1, tile layout": (False, 2, 1), "mode 1, two stripe sets": (False, 1, 1),
         "mode 2": (False, 2, 2)}


def run_bed(c, raw, layout, mode):
    """gv_assoc_loo and gv_pvals_loo of one bed case on one path"""
    with capi.Shard(c["N"], c["M"]) as sh:
        sh.set_layout(raw, layout)
        sh.set_kernel_mode(mode)
        sh.upload_bed(c["bed"])
        if c["masked"]:
            sh.set_mask(c["m4"], c["nonas"])
        sh.compute_markers_statistics()
        mave, msig = sh.marker_stats()
        dz, dy, dx = sh.vecN(c["z1"]), sh.vecN(c["y"]), sh.vecM(c["x1"])
        narrow = sh.pvals_calc(dz, dy, dx)
        wide = sh.assoc_calc(dz, dy, dx)
        assert sh.get_kernel_mode() == mode and sh.get_layout() == layout
    assert np.allclose(mave, c["mave"], rtol=1e-14, atol=0) and np.allclose(msig, c["msig"], rtol=1e-14, atol=0)
    return wide, narrow


@functools.lru_cache(maxsize=None)
def small_run(masked, path):
    return run_bed(small_case(masked), *PATHS[path])


# ---- small samples: the seams of t_two_sided, every path of the bed data ------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("masked", [False, True])
def test_small_samples_p_over_the_plane_and_the_rest_against_the_restatement(masked, path):
    c = small_case(masked)
    wide, narrow = small_run(masked, path)
    what = "small%s, %s" % (" masked" if masked else "", path)
    assert np.array_equal(narrow, wide["p"], equal_nan=True), what                                   # assertion 4
    pref = p_against_reference(wide["p"], wide["t"], c["cnt"], c["alive"], what)                     # assertion 2
    coverage(wide["t"], c["cnt"], c["alive"], pref, what, per_region=20, per_seam_side=2, w_span=(1e-8, 1e4))
    held_to_the_restatement(wide, c["ref"], c["ref64"], what, c["dead"], pref)                       # assertion 3
    signs = np.sign(wide["t"][c["alive"]])
    assert (signs > 0).sum() >= 150 and (signs < 0).sum() >= 150


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("masked", [False, True])
def test_fewer_than_three_present_genotypes_or_one_genotype_give_nan(masked, path):
    """assertion 6: n = 0, 1, 2 (two genotypes, one genotype) and a marker monomorphic among its 40 present genotypes"""
    c = small_case(masked)
    assert list(c["cnt"][c["dead"]]) == [0, 1, 2, 2, 40]
    assert not not_nan(c["ref"], c["dead"]), "the restatement"
    wide, narrow = small_run(masked, path)
    rows = dict(zip(c["dead"], DEGENERATE))
    found = [(rows[k], key, v) for k, key, v in not_nan(wide, c["dead"])]
    found += [(rows[k], "p (gv_pvals_loo)", float(narrow[k])) for k in c["dead"] if not np.isnan(narrow[k])]
    assert not found, (path, found)


@pytest.mark.parametrize("masked", [False, True])
def test_the_two_resident_layouts_of_mode_1_agree_bit_for_bit(masked):
    """assertion 5, the degenerate rows included"""
    (wa, na_), (wb, nb) = small_run(masked, "mode 1, tile layout"), small_run(masked, "mode 1, two stripe sets")
    differ = [(key, int(k), float(wa[key][k]), float(wb[key][k])) for key in KEYS
              for k in np.nonzero(~((wa[key] == wb[key]) | (np.isnan(wa[key]) & np.isnan(wb[key]))))[0]]
    assert not differ, differ[:8]
    assert np.array_equal(na_, nb, equal_nan=True)


# ---- large samples: the deep tail, the underflow and the h == 0 cut ----------------------------------------------------------------
LARGE_U = (1e-5, 1e-2, 0.5, 3.0, 30.0, 100.0, 235.0, 460.0, 600.0, 640.0, 655.0, 692.0, 715.0, 740.0, 765.0, 2000.0)
LARGE_W = (0.43, 1.0)         # the far corner: the fraction at large a


@functools.lru_cache(maxsize=None)
def large_case():
    """N = 20000; n = 20000, 19999, 12002; w set through u = (a - 1/4) log1p(w), the exponent of the expansion: p ~ e^-u / sqrt(pi u)"""
    counts, targets = [], []
    for n in (20000, 19999, 12002):
        T = 0.5 * (n - 2) - 0.25
        for w in [math.expm1(u / T) for u in LARGE_U] + list(LARGE_W):
            counts.append(n)
            targets.append(w)
    return bed_inputs(20000, False, np.array(counts), targets, False, 11)


def test_large_samples_deep_tail_underflow_and_cut():
    c = large_case()
    what = "large, mode 1"
    wide, narrow = run_bed(c, False, 2, 1)
    assert np.array_equal(narrow, wide["p"], equal_nan=True), what
    t, n, rows = wide["t"], c["cnt"], c["alive"]
    pref = p_against_reference(wide["p"], t, n, rows, what)
    u = np.array([(0.5 * (n[k] - 2) - 0.25) * math.log1p(t[k] ** 2 / (n[k] - 2)) for k in rows])
    w = t ** 2 / (n - 2)
    assert any(P_FLOOR <= pref[k] < 1e-100 for k in rows) and any(P_FLOOR <= pref[k] < 1e-270 for k in rows)
    assert any(pref[k] < 1e-300 and u[k] < 740 for k in rows), "past the underflow of p, before exp(-u) == 0"
    assert any(760 < u[k] and w[k] <= 0.42 for k in rows), "the h == 0 cut"
    assert any(w[k] > 0.42 for k in rows) and any(w[k] < 1e-8 for k in rows)
    assert all(region(float(t[k]), int(n[k]) - 2) in (3, 4) for k in rows)
    held_to_the_restatement(wide, c["ref"], c["ref64"], what, c["dead"], pref)


# ---- dosage data: the third copy, k_dosage_assoc ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dosage_case():
    N, bits, scale = 128, 8, 1.0 / 127.0
    rng = np.random.default_rng(13)
    counts = np.array([nu + 2 for nu in NUS for _ in WS_DOSAGE])
    targets = [w for _ in NUS for w in WS_DOSAGE]
    M = len(counts) + 4
    B = np.full((M, N), 255, dtype=np.uint8)
    for k, n in enumerate(counts):
        who = rng.permutation(N)[:n]
        B[k, who] = rng.integers(0, 255, n)
        if np.all(B[k, who] == B[k, who[0]]):
            B[k, who[0]] = (int(B[k, who[0]]) + 1) % 255
    k = len(counts)                                           # n = 0; n = 1; n = 2; constant among 40
    B[k + 1, 5], B[k + 2, [7, 90]], B[k + 3, 20:60] = 17, [3, 200], 99
    na = np.ones(N)
    y, z1 = rng.standard_normal(N), np.zeros(N)
    s, s64 = dr.stats(B, bits, na, scale), dr.stats(B, bits, na, scale, dtype=np.float64)
    V = s["D"] * s["w"][:, None]
    x1 = np.full(M, 0.7 * math.sqrt(N))
    for k, w in enumerate(targets):
        at = B[k] != 255
        x1[k] = effect_for(V[k, at], y[at], w, 1.0 if k % 2 == 0 else -1.0, N)
    ref, ref64 = dr.assoc(s, na, y, z1, x1), dr.assoc(s64, na, y, z1, x1, with_p=False)
    ref64["p"] = np.zeros(M)
    assert np.array_equal(s["cnt"][:len(counts)], counts) and list(s["cnt"][len(counts):]) == [0, 1, 2, 40]
    return dict(N=N, M=M, B=B, scale=scale, y=y, z1=z1, x1=x1, cnt=s["cnt"], ref=ref, ref64=ref64, alive=np.arange(len(counts)),
                dead=np.arange(len(counts), M))


def test_dosage_with_missing_entries_over_the_plane():
    """110 markers: two of five w on the near side of 0.42, so the expansion regions hold 12 and 10 markers and each side of a seam
    one -- the conditions of the bed case scaled to this grid (10 per region, one per side, w down to 1e-4 and up to 1e3)"""
    c = dosage_case()
    what = "dosage8 with missing entries"
    with capi.Shard(c["N"], c["M"]) as sh:
        sh.upload_dosage(c["B"], c["scale"], missing=True)
        sh.compute_markers_statistics()
        cnt = sh.marker_counts()
        wide = sh.assoc_calc(sh.vecN(c["z1"]), sh.vecN(c["y"]), sh.vecM(c["x1"]))
    assert np.array_equal(cnt, c["cnt"])
    pref = p_against_reference(wide["p"], wide["t"], cnt, c["alive"], what)
    coverage(wide["t"], cnt, c["alive"], pref, what, per_region=10, per_seam_side=1, w_span=(1e-3, 1e2))
    held_to_the_restatement(wide, c["ref"], c["ref64"], what, c["dead"], pref)
    assert not not_nan(c["ref"], c["dead"]) and not not_nan(wide, c["dead"]), not_nan(wide, c["dead"])
