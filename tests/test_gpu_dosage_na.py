"""Missing entries in compact dosage data: the all-ones code (255 / 65535) as a reserved code that every kernel skips
(gv_set_dosage_missing), against the long-double restatement of tests/dosage_na_restatement.py, against the plain kernels bit for bit
where no reserved code is present, and against the bed path and the oracle through a bed file with missing genotypes.

Bars, those of tests/test_gpu_dosage.py and tests/test_gpu_assoc.py (the formulas are the same): statistics rtol 1e-13, products
rel-l2 < 1e-13, p rtol 1e-8, beta / se / t 16 x the float64 deviation of the restatement and never less than 1e-12."""
import functools
import os
import subprocess
import threading

import numpy as np
import pytest

import assoc_restatement as ar
import dosage_na_restatement as dr
from gvamp_amd import capi, hostapi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS, VARS = [0.90, 0.07, 0.03], [0, 0.001, 0.01]
LD = np.longdouble
DTYPE = {8: np.uint8, 16: np.uint16}
TEST_SCALE = {8: 1.0 / 127.0, 16: 2.0 ** -14}
DYADIC = {8: 2.0 ** -6, 16: 2.0 ** -14}
STEP = {8: 64, 16: 16384}
KEYS = ("beta", "se", "t", "p")
SWITCH = "GV_DOSAGE_NA_KERNELS"


def rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


def na_mask(N, with_na):
    """(mask4 nibbles, na[N], nonas): every 7th individual from 3 on has no phenotype"""
    na = np.ones(N)
    if with_na:
        na[3::7] = 0.0
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    for n in np.nonzero(na)[0]:
        m4[n >> 2] |= 1 << (n & 3)
    return m4, na, int(na.sum())


def npad_of(N):
    return 4 * ((((N + 3) // 4) + 63) // 64 * 64)


def codes_with_missing(N, M, bits, seed):
    """synth_dosage_na at 30 000 ppm plus rows placed by hand; returns (codes, {name: row})"""
    R = dr.reserved(bits)
    B = synth.synth_dosage_na(N, M, seed, bits, 30000)
    rows = {}
    if N == 1:
        B[0, 0] = R                                           # its only entry missing
        rows["all_missing"] = 0
        return B, rows
    B[0] = R                                                  # cnt = 0: mu' = 0, msig == 1, products exactly 0
    rows["all_missing"] = 0
    B[1] = R
    B[1, 2] = 77                                              # one present entry, at an individual with a phenotype
    rows["one_present"] = 1
    B[2] = 200 if bits == 8 else 40001                        # present entries constant: q == 0, msig == 1.0 exactly
    B[2, 1::3] = R
    rows["constant"] = 2
    if M >= 7:
        for r in (3, 4, 5, 6):
            B[r][B[r] == R] = R - 1
        B[3, 0] = R                                           # missing only at n = 0
        B[4, N - 1] = R                                       # missing only at n = N - 1
        B[5, 3] = R                                           # missing only at an individual whose phenotype is masked (na[3::7] = 0)
        rows.update(first=3, last=4, masked=5)
        if bits == 16:
            B[6, 1], B[6, 2] = 255, 0xFF00                    # ordinary values that share a byte with the reserved code
            rows["bytes"] = 6
    return B, rows


@functools.lru_cache(maxsize=2)
def case(bits, N, M, with_na):
    """inputs and the restatement of one case, computed once and left unchanged"""
    B, rows = codes_with_missing(N, M, bits, N * 7 + M)
    m4, na, nonas = na_mask(N, with_na)
    rng = np.random.default_rng(N + M + bits)
    npad = npad_of(N)
    x, x2 = rng.standard_normal(M), rng.standard_normal(M)
    p, p2 = np.zeros(npad), np.zeros(npad)
    p[:N], p2[:N] = rng.standard_normal(N), rng.standard_normal(N)
    out = dict(B=B, rows=rows, m4=m4, na=na, nonas=nonas, x=x, x2=x2, p=p, p2=p2, scale=TEST_SCALE[bits])
    for a in (B, x, x2, p, p2):
        a.setflags(write=False)
    return out


SHAPES = [(1, 1), (5, 3), (1003, 700), (4099, 301)]


@pytest.mark.parametrize("with_na", [False, True])
@pytest.mark.parametrize("N,M", SHAPES)
@pytest.mark.parametrize("bits", [8, 16])
def test_statistics_and_products_vs_long_double_restatement(bits, N, M, with_na):
    c = case(bits, N, M, with_na)
    B, rows, scale, nonas, x, x2 = c["B"], c["rows"], c["scale"], c["nonas"], c["x"], c["x2"]
    R = dr.reserved(bits)
    with capi.Shard(N, M) as sh:
        sh.upload_dosage(B, scale, missing=True)
        info = sh.dosage_info()
        assert info == dict(bits=bits, scale=scale, missing=True, reserved=int((B == R).sum()), na_kernels=True), info
        if with_na:
            sh.set_mask(c["m4"], nonas)
        npad = 4 * sh.mbytes
        p, p2 = c["p"][:npad], c["p2"][:npad]
        for alpha in (0.3, 1.0):
            st = dr.stats(B, bits, c["na"], scale, alpha)
            sh.compute_markers_statistics(alpha)
            mave, msig = sh.marker_stats()
            rm, rs = st["mave"], st["msig"]
            print("alpha %.1f: mave max rel %.3e  msig max rel %.3e" % (alpha, float(np.max(np.abs(mave - rm) / np.maximum(np.abs(rm), LD(1e-300)))),
                                                                        float(np.max(np.abs(msig - rs) / np.abs(rs)))))
            assert np.allclose(mave, rm.astype(np.float64), rtol=1e-13, atol=0)
            assert np.allclose(msig, rs.astype(np.float64), rtol=1e-13, atol=0)
            assert np.array_equal(sh.marker_counts(), st["cnt"].astype(np.float64))       # exact
        # (alpha = 1.0 from here on)
        assert st["cnt"][rows["all_missing"]] == 0 and mave[rows["all_missing"]] == 0.0 and msig[rows["all_missing"]] == 1.0
        if "one_present" in rows:
            assert st["cnt"][rows["one_present"]] == 1 and msig[rows["one_present"]] == 1.0
            assert mave[rows["one_present"]] == scale * 77
            assert msig[rows["constant"]] == 1.0              # q == 0 exactly over the present entries, whatever the scale
        if "masked" in rows:
            assert st["cnt"][rows["first"]] == nonas - 1 and st["cnt"][rows["last"]] == nonas - (0 if c["na"][N - 1] == 0 else 1)
            assert st["cnt"][rows["masked"]] == nonas - (0 if with_na else 1)
        if "bytes" in rows:
            assert st["cnt"][rows["bytes"]] == nonas
        z, w = sh.Ax(x), sh.ATx(p)
        rz, rw = dr.ax(st, x, npad), dr.atx(st, p)
        print("Ax rel %.3e  ATx rel %.3e" % (rel(z, rz), rel(w, rw)))
        assert rel(z, rz) < 1e-13
        assert rel(w, rw) < 1e-13
        assert np.all(z[N:] == 0.0)                                    # exact zeros at the pad slots
        assert w[rows["all_missing"]] == 0.0                           # a row of missing entries: products exactly 0
        if M == 1:
            assert np.all(z == 0.0)
        if with_na and N > 3 and M > 3:
            assert np.all(z[3:N:7] != 0.0)                             # no phenotype mask in Ax
        assert np.array_equal(sh.Ax(x), z) and np.array_equal(sh.ATx(p), w)     # bit-reproducible
        # two-vector forms: with missing data each slot is bit-equal to the one-vector call on that vector
        dx, dx2, dz, dz2 = sh.vecM(x), sh.vecM(x2), sh.vecN(), sh.vecN()
        sh.ax2_dev(dx, dx2, dz, dz2)
        assert np.array_equal(dz.download(), z) and np.array_equal(dz2.download(), sh.Ax(x2))
        dp, dp2, dw, dw2 = sh.vecN(p), sh.vecN(p2), sh.vecM(), sh.vecM()
        sh.atx2_dev(dp, dp2, dw, dw2)
        assert np.array_equal(dw.download(), w) and np.array_equal(dw2.download(), sh.ATx(p2))
        tau, gam2 = 1.7, 0.35
        d = sh.vecM()
        sh.lmmse_mult(dx, tau, gam2, d)
        expect = dr.lmmse_mult(st, x, tau, gam2)
        print("lmmse_mult rel %.3e" % rel(d.download(), expect))
        assert rel(d.download(), expect) < 1e-13


# ---- the two instantiations against each other ------------------------------------------------------------------------------------
def everything(sh, c, N, M):
    """statistics, products, two-vector products, lmmse_mult and gv_assoc_loo of a shard, as arrays to compare bit for bit"""
    npad = 4 * sh.mbytes
    x, x2, p, p2 = c["x"], c["x2"], c["p"][:npad], c["p2"][:npad]
    sh.set_mask(c["m4"], c["nonas"])
    sh.compute_markers_statistics()
    out = list(sh.marker_stats()) + [sh.marker_counts(), sh.Ax(x), sh.ATx(p)]
    dx, dx2, dz, dz2 = sh.vecM(x), sh.vecM(x2), sh.vecN(), sh.vecN()
    sh.ax2_dev(dx, dx2, dz, dz2)
    dp, dp2, dw, dw2 = sh.vecN(p), sh.vecN(p2), sh.vecM(), sh.vecM()
    sh.atx2_dev(dp, dp2, dw, dw2)
    d = sh.vecM()
    sh.lmmse_mult(dx, 1.7, 0.35, d)
    out += [dz.download(), dz2.download(), dw.download(), dw2.download(), d.download()]
    y = np.zeros(npad)
    y[:N] = p2[:N] * 2
    a = sh.assoc_calc(sh.vecN(p), sh.vecN(y), sh.vecM(x * 0.1))
    return out + [a[k] for k in KEYS]


@pytest.mark.parametrize("N,M", [(1003, 700), (4099, 301)])
@pytest.mark.parametrize("bits", [8, 16])
def test_without_a_reserved_code_both_instantiations_give_the_same_bits(monkeypatch, bits, N, M):
    c = case(bits, N, M, True)
    B = synth.synth_dosage_na(N, M, 5, bits, 0)
    B[2] = 200 if bits == 8 else 40001                       # a constant row: NaN from both
    assert not np.any(B == dr.reserved(bits))
    scale = TEST_SCALE[bits]
    monkeypatch.delenv(SWITCH, raising=False)
    with capi.Shard(N, M) as off, capi.Shard(N, M) as short:
        off.upload_dosage(B, scale)
        short.upload_dosage(B, scale, missing=True)
        assert off.dosage_info() == dict(bits=bits, scale=scale, missing=False, reserved=0, na_kernels=False)
        # the shortcut: option on, no reserved code counted -- the plain kernels, and the count 0
        assert short.dosage_info() == dict(bits=bits, scale=scale, missing=True, reserved=0, na_kernels=False)
        monkeypatch.setenv(SWITCH, "1")                      # read by gv_create, per context
        with capi.Shard(N, M) as forced:
            forced.upload_dosage(B, scale, missing=True)
            assert forced.dosage_info() == dict(bits=bits, scale=scale, missing=True, reserved=0, na_kernels=True)
            ref = everything(off, c, N, M)
            assert np.array_equal(ref[2], np.full(M, float(c["nonas"])))
            assert np.isnan(ref[-1][2]) and np.all(np.isfinite(np.delete(ref[-1], 2)))
            for sh in (forced, short):
                for a, b in zip(everything(sh, c, N, M), ref):
                    assert np.array_equal(a, b, equal_nan=True)
        with capi.Shard(N, M) as off2:                       # the switch forces nothing while the option is off
            off2.upload_dosage(B, scale)
            assert off2.dosage_info()["na_kernels"] is False


# ---- option off ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
def test_option_off_reserved_codes_are_values_and_the_setting_is_pinned_while_codes_are_resident(bits):
    N, M = 1003, 700
    c = case(bits, N, M, True)
    B, scale, x = c["B"], c["scale"], c["x"]
    R = dr.reserved(bits)
    st = dr.stats(B, bits, c["na"], scale, missing=False)     # == the definition tests/test_gpu_dosage.py restates (test_dosage_na_cpu.py)
    with capi.Shard(N, M) as sh:
        assert sh.dosage_info() == dict(bits=0, scale=0.0, missing=False, reserved=0, na_kernels=False)
        sh.upload_dosage(B, scale)
        assert sh.dosage_info() == dict(bits=bits, scale=scale, missing=False, reserved=0, na_kernels=False)
        sh.set_mask(c["m4"], c["nonas"])
        sh.compute_markers_statistics()
        mave, msig = sh.marker_stats()
        assert np.allclose(mave, st["mave"].astype(np.float64), rtol=1e-13, atol=0)
        assert np.allclose(msig, st["msig"].astype(np.float64), rtol=1e-13, atol=0)
        assert mave[0] == scale * R                            # the row of reserved codes is a constant row at the value it is
        assert np.array_equal(sh.marker_counts(), np.full(M, float(c["nonas"])))
        npad = 4 * sh.mbytes
        p = c["p"][:npad]
        print("off: Ax rel %.3e  ATx rel %.3e" % (rel(sh.Ax(x), dr.ax(st, x, npad)), rel(sh.ATx(p), dr.atx(st, p))))
        assert rel(sh.Ax(x), dr.ax(st, x, npad)) < 1e-13 and rel(sh.ATx(p), dr.atx(st, p)) < 1e-13
        z = sh.Ax(x)
        with pytest.raises(capi.GvError, match="gv_set_dosage_missing: %d-bit codes are resident" % bits):
            sh.set_dosage_missing(True)
        sh.set_dosage_missing(False)                           # the setting they were uploaded with: nothing to refuse
        assert np.array_equal(sh.Ax(x), z) and sh.dosage_info()["missing"] is False
        sh.upload_bed(synth.synth_bed(N, M, seed=3, miss_ppm=0))      # another kind replaces the data set: the setting is free again
        sh.set_dosage_missing(True)
        sh.upload_dosage(B, scale, missing=True)
        assert sh.dosage_info()["reserved"] == int((B == R).sum())
        with pytest.raises(capi.GvError, match="gv_set_dosage_missing"):
            sh.set_dosage_missing(False)
        sh.upload_meth(synth.synth_meth(N, M, 7))                    # ... and the count is reset with it
        assert sh.dosage_info() == dict(bits=0, scale=0.0, missing=True, reserved=0, na_kernels=False)


# ---- one context through every kind: the allocation an upload of the same width reuses, and the state it must not inherit -------------
def test_one_context_through_a_sequence_of_uploads_equals_a_fresh_context_after_each(monkeypatch):
    """Eight uploads into ONE context -- two of them (2 and 5) of the width already held, which keep the allocation -- and after each
    one gv_dosage_info, gv_get_layout, the resident bytes of gv_ingest_info2, the marker statistics, the counts and both products
    are those of a fresh context given that upload alone, bit for bit.  N = 1203: one whole 1024-column step and a partial one, N no
    multiple of 4; M = 450: no multiple of the 32- or 16-row wave groups."""
    monkeypatch.delenv(SWITCH, raising=False)
    N, M = 1203, 450
    pitch = (N + 63) // 64 * 64
    s1, s2 = 1.0 / 127.0, 2.0 ** -6
    m4, _na, nonas = na_mask(N, True)
    rng = np.random.default_rng(N + M)
    x = rng.standard_normal(M)
    p = np.zeros(4 * ((N + 3) // 4))
    p[:N] = rng.standard_normal(N)
    b8a, b8b = synth.synth_dosage(N, M, 11, 8), synth.synth_dosage(N, M, 12, 8)
    n8a, _rows = codes_with_missing(N, M, 8, 13)
    n8b = synth.synth_dosage_na(N, M, 14, 8, 30000)
    n16 = synth.synth_dosage_na(N, M, 15, 16, 0)
    b16 = synth.synth_dosage(N, M, 16, 16)
    b8a[0, 0], b16[0, 0] = 255, 65535                          # option off: the all-ones code is a value
    assert not np.any(n16 == 65535) and np.any(n8a == 255) and np.any(n8b == 255) and not np.array_equal(n8a, n8b)
    bed, meth = synth.synth_bed(N, M, seed=3, miss_ppm=5000), synth.synth_meth(N, M, 7)
    none = dict(bits=0, scale=0.0, reserved=0, na_kernels=False)

    def codes(B, scale, missing):
        R = dr.reserved(8 * B.dtype.itemsize)
        res = int((B == R).sum()) if missing else 0
        info = dict(bits=8 * B.dtype.itemsize, scale=scale, missing=missing, reserved=res, na_kernels=res != 0)
        return (lambda sh: sh.upload_dosage(B, scale, missing=missing)), info, 3 + B.dtype.itemsize, B.dtype.itemsize

    steps = [codes(b8a, s1, False),
             codes(b8b, s2, False),                              # the width held: the allocation is kept
             ((lambda sh: sh.upload_bed(bed)), dict(none, missing=False), 2, None),
             codes(n8a, s1, True),
             codes(n8b, s2, True),                               # the width held, with the state of missing entries to reset
             codes(n16, TEST_SCALE[16], True),                   # option on, no reserved code: the plain kernels
             ((lambda sh: sh.upload_meth(meth)), dict(none, missing=True), 3, 8),
             codes(b16, TEST_SCALE[16], False)]

    def observe(sh, is_codes):
        sh.compute_markers_statistics()
        out = list(sh.marker_stats()) + [sh.Ax(x), sh.ATx(p)]
        return out + ([sh.marker_counts()] if is_codes else [])

    with capi.Shard(N, M) as one:
        one.set_mask(m4, nonas)
        for k, (upload, info, layout, esz) in enumerate(steps, 1):
            upload(one)
            with capi.Shard(N, M) as fresh:
                fresh.set_mask(m4, nonas)
                if info["missing"] and not info["bits"]:
                    fresh.set_dosage_missing(True)               # (the setting outlives the dataset)
                upload(fresh)
                for sh in (one, fresh):
                    assert sh.dosage_info() == info, (k, sh.dosage_info())
                    assert sh.get_layout() == layout, (k, sh.get_layout())
                    if esz:
                        assert sh.ingest_stats()["resident_GB"] == esz * M * pitch / 1e9, (k, sh.ingest_stats())
                assert one.ingest_stats()["resident_GB"] == fresh.ingest_stats()["resident_GB"], k
                got, ref = observe(one, info["bits"] != 0), observe(fresh, info["bits"] != 0)
            assert len(got) == len(ref) and all(np.all(np.isfinite(a)) for a in ref[2:]), k
            for a, b in zip(got, ref):
                assert np.array_equal(a, b), k
            if info["bits"]:
                assert np.any(got[-1] != nonas) == info["na_kernels"], k


# ---- bed parity: a bed file with missing genotypes, written as codes with the reserved code --------------------------------------
_VAMP_KW = dict(iterations=6, CG_max_iter=30, rho=0.5, seed=7, gam1=1e-8, gamw=2.0)


def bed_as_codes(G, have, bits):
    B = (G * STEP[bits]).astype(DTYPE[bits])
    B[~have] = dr.reserved(bits)
    return B


@functools.lru_cache(maxsize=1)
def _bed_case():
    from oracle import gvoracle
    N, M = 2000, 1500
    bed = synth.synth_bed(N, M, seed=17, miss_ppm=20000)
    G, have = ar.decode_bed(bed, N, M)
    assert (~have).sum() > 10000
    beta, y = gvoracle.sim_phen(bed, N, M, 0.5, 300, 7, nthreads=4)
    return N, M, bed, G, have, y


@functools.lru_cache(maxsize=None)
def _bed_runs(fuse):
    from oracle import gvoracle
    N, M, bed, G, have, y = _bed_case()
    ref = gvoracle.infere(bed, N, M, y, PROBS, VARS, **_VAMP_KW)
    with capi.Shard(N, M, anchor=True) as sb:
        sb.upload_bed(bed)
        rb = hostapi.infere_linear(sb, y, PROBS, VARS, fuse_solves=fuse, **_VAMP_KW)
    return ref, rb


@pytest.mark.parametrize("fuse", [0, 4])
@pytest.mark.parametrize("bits", [8, 16])
def test_vamp_on_codes_of_a_bed_with_missing_genotypes_matches_bed_run_and_oracle(oracle, bits, fuse):
    N, M, bed, G, have, y = _bed_case()
    ref, rb = _bed_runs(fuse)
    with capi.Shard(N, M) as sd:
        sd.upload_dosage(bed_as_codes(G, have, bits), DYADIC[bits], missing=True)
        assert sd.dosage_info()["na_kernels"] and sd.dosage_info()["reserved"] == int((~have).sum())
        rd = hostapi.infere_linear(sd, y, PROBS, VARS, fuse_solves=fuse, **_VAMP_KW)
    assert rd.niter == rb.niter == ref.niter
    print("x_hat rel to bed run %.3e, to oracle %.3e" % (rel(rd.x_est, rb.x_est), rel(rd.x_est, ref.x_est)))
    assert rel(rd.x_est, rb.x_est) < 1e-9 and rel(rd.x_est, ref.x_est) < 1e-9
    for it in range(rd.niter):
        t, b, o = rd.trace[it], rb.trace[it], ref.trace[it]
        assert (t["cg_iters"], t["onsager_iters"]) == (b["cg_iters"], b["onsager_iters"]) == (o["cg_iters"], o["onsager_iters"])


def deviation(got, ref):
    """tests/test_gpu_assoc.py: |d beta| / (|beta| + se), |d se| / se, |d t| / (|t| + 1), maxima over the rows"""
    g = {k: np.asarray(got[k], dtype=LD) for k in ("beta", "se", "t")}
    r = {k: np.asarray(ref[k], dtype=LD) for k in ("beta", "se", "t")}
    sb, ss = np.abs(r["beta"]) + r["se"], r["se"]
    return dict(beta=float(np.max(np.abs(g["beta"] - r["beta"]) / np.where(sb > 0, sb, LD(1)))),
                se=float(np.max(np.abs(g["se"] - r["se"]) / np.where(ss > 0, ss, LD(1)))),
                t=float(np.max(np.abs(g["t"] - r["t"]) / (np.abs(r["t"]) + 1))))


def check(got, ref, ref64, what, keep):
    """got against ref (long double) on the rows `keep`: beta / se / t within 16 x the float64 restatement's deviation (never less than
    1e-12), p to rtol 1e-8"""
    gk, rk, r64 = ({k: np.asarray(d[k])[keep] for k in d} for d in (got, ref, ref64))
    assert np.all(np.isfinite(rk["t"])), what
    for k in KEYS:
        assert np.all(np.isfinite(gk[k])), (what, k)
    dev64, devg = deviation(r64, rk), deviation(gk, rk)
    for k in ("beta", "se", "t"):
        bound = max(16.0 * dev64[k], 1e-12)
        print("%s %-4s float64 dev %.3e  GPU dev %.3e  bound %.3e" % (what, k, dev64[k], devg[k], bound))
        assert devg[k] <= bound, (what, k, devg[k], bound)
    rp = np.asarray(rk["p"], dtype=np.float64)
    pos = rp > 0
    print("%s p    max rel %.3e" % (what, float(np.max(np.abs(gk["p"][pos] / rp[pos] - 1))) if pos.any() else 0.0))
    assert np.allclose(gk["p"], rp, rtol=1e-8, atol=0), what


@pytest.mark.parametrize("bits", [8, 16])
def test_assoc_loo_on_codes_of_a_bed_with_missing_genotypes_equals_the_bed_path(bits):
    N, M, bed, G, have, y = _bed_case()
    rng = np.random.default_rng(5)
    x1 = rng.standard_normal(M) * (rng.random(M) < 0.05) * 3.0
    na = np.ones(N)
    B = bed_as_codes(G, have, bits)
    st, st64 = dr.stats(B, bits, na, DYADIC[bits]), dr.stats(B, bits, na, DYADIC[bits], dtype=np.float64)
    npad = 4 * ((N + 3) // 4)
    yy = np.zeros(npad)
    yy[:N] = y
    with capi.Shard(N, M) as sb:
        sb.upload_bed(bed)
        sb.compute_markers_statistics()
        z1 = sb.Ax(x1)
        b_loo = sb.assoc_calc(sb.vecN(z1), sb.vecN(yy), sb.vecM(x1))
    with capi.Shard(N, M) as sd:
        sd.upload_dosage(B, DYADIC[bits], missing=True)
        sd.compute_markers_statistics()
        d_loo = sd.assoc_calc(sd.vecN(z1), sd.vecN(yy), sd.vecM(x1))
    ref, ref64 = dr.assoc(st, na, yy, z1, x1), dr.assoc(st64, na, yy, z1, x1, with_p=False)
    keep = np.ones(M, dtype=bool)
    dev64, devd = deviation(ref64, ref), deviation(d_loo, b_loo)
    for k in ("beta", "se", "t"):
        bound = max(16.0 * dev64[k], 1e-12)
        print("dosage%d vs bed %-4s dev %.3e  float64 restatement dev %.3e  bound %.3e" % (bits, k, devd[k], dev64[k], bound))
        assert devd[k] <= bound
    print("dosage%d vs bed p max rel %.3e" % (bits, float(np.max(np.abs(d_loo["p"] / b_loo["p"] - 1)))))
    assert np.allclose(d_loo["p"], b_loo["p"], rtol=1e-8, atol=0)
    check(d_loo, ref, ref64, "dosage%d bed-with-missing loo" % bits, keep)


# ---- association on dosage data with missing entries ------------------------------------------------------------------------------
def chrom_layout(M):
    """sorted chromosomes: two markers outside 1..23 at each end, chromosome 1 of one marker, chromosome 2 of five, the rest over 4..23"""
    body = M - 2 - 1 - 5 - 2
    rest = 4 + (np.arange(body) * 20) // body
    return np.concatenate([[0, 0], [1], [2] * 5, rest, [24, 24]]).astype(np.int32)


@functools.lru_cache(maxsize=1)
def assoc_case(bits, N, M, with_na):
    c = case(bits, N, M, with_na)
    rng = np.random.default_rng(1000 * bits + N + M + int(with_na))
    B = c["B"].copy()
    R = dr.reserved(bits)
    B[7] = R
    B[7, 4:6] = 9, 200                                        # cnt == 2: no test
    B[8] = R
    B[8, 4:7] = 9, 200, 31                                    # cnt == 3: the smallest sample with a test
    B[0], B[M - 3] = c["B"][M - 3], c["B"][0]                 # (the row of missing entries on a tested chromosome)
    B[1], B[M - 4] = c["B"][M - 4], c["B"][1]
    na, scale = c["na"], c["scale"]
    chrom = chrom_layout(M)
    x1 = np.zeros(M)
    x1[np.linspace(9, M - 10, 6).astype(int)] = np.sqrt(N) * np.array([1.2, -0.9, 0.5, -0.3, 0.15, -0.05])
    x1 += (rng.random(M) < 0.02) * rng.standard_normal(M) * 0.05 * np.sqrt(N)
    st, st64 = dr.stats(B, bits, na, scale), dr.stats(B, bits, na, scale, dtype=np.float64)
    npad = 4 * ((N + 3) // 4)
    z1, y = np.zeros(npad), np.zeros(npad)
    z1[:N] = dr.ax(st, x1, N).astype(np.float64)
    y[:N] = z1[:N] + rng.standard_normal(N)
    y[:N][na == 0] = 1e300                                    # whatever a caller may leave at the NA slots
    y[N:] = -1e300                                            # ... and in the padding
    ref = {"loo": dr.assoc(st, na, y, z1, x1), "loco": dr.assoc(st, na, y, z1, x1, chrom=chrom)}
    ref64 = {"loo": dr.assoc(st64, na, y, z1, x1, with_p=False), "loco": dr.assoc(st64, na, y, z1, x1, chrom=chrom, with_p=False)}
    dead = (st["cnt"] < 3) | (st["q"] == 0)
    return dict(B=B, chrom=chrom, x1=x1, z1=z1, y=y, ref=ref, ref64=ref64, dead=dead, cnt=st["cnt"])


@pytest.mark.parametrize("with_na", [False, True])
@pytest.mark.parametrize("N,M", [(1003, 700), (4099, 301)])
@pytest.mark.parametrize("bits", [8, 16])
def test_assoc_vs_long_double_restatement(bits, N, M, with_na):
    c, a = case(bits, N, M, with_na), assoc_case(bits, N, M, with_na)
    dead, chrom = a["dead"], a["chrom"]
    assert dead[[2, 7, M - 3, M - 4]].all() and not dead[8] and a["cnt"][8] == 3 and dead.sum() == 4
    with capi.Shard(N, M) as sh:
        sh.upload_dosage(a["B"], c["scale"], missing=True)
        assert sh.dosage_info()["na_kernels"]
        if with_na:
            sh.set_mask(c["m4"], c["nonas"])
        sh.compute_markers_statistics()
        dz, dy, dx = sh.vecN(a["z1"]), sh.vecN(a["y"]), sh.vecM(a["x1"])
        loo, loco = sh.assoc_calc(dz, dy, dx), sh.assoc_calc(dz, dy, dx, chrom=chrom)
        assert all(np.array_equal(sh.assoc_calc(dz, dy, dx)[k], loo[k], equal_nan=True) for k in KEYS)      # bit-reproducible
    tested = (chrom >= 1) & (chrom <= 23)
    for res, name, isdead in ((loo, "loo", dead), (loco, "loco", dead & tested)):
        for k in KEYS:                                         # cnt < 3 and constant rows: NaN in all four outputs, both sides
            assert np.all(np.isnan(res[k][isdead])) and np.all(np.isnan(np.asarray(a["ref"][name][k])[isdead])), (name, k)
        check(res, a["ref"][name], a["ref64"][name], "dosage%d %dx%d na=%d %s" % (bits, N, M, with_na, name), ~isdead)
    for k in KEYS:
        assert np.all(loco[k][~tested] == 0.0)


@pytest.mark.parametrize("bits", [8, 16])
def test_loco_with_one_chromosome_and_zero_effects_equals_loo_bit_for_bit(bits):
    N, M = 1003, 700
    c, a = case(bits, N, M, True), assoc_case(bits, N, M, True)
    with capi.Shard(N, M) as sh:
        sh.upload_dosage(a["B"], c["scale"], missing=True)
        sh.set_mask(c["m4"], c["nonas"])
        sh.compute_markers_statistics()
        dz, dy, dx = sh.vecN(a["z1"]), sh.vecN(a["y"]), sh.vecM(np.zeros(M))
        loo, loco = sh.assoc_calc(dz, dy, dx), sh.assoc_calc(dz, dy, dx, chrom=np.ones(M, dtype=np.int32))
    for k in KEYS:
        assert np.array_equal(loo[k], loco[k], equal_nan=True)
    assert np.isfinite(loo["t"]).sum() == M - 4


# ---- generator, file, driver, shards -----------------------------------------------------------------------------------------------
def outputs(sh, x, p):
    sh.compute_markers_statistics()
    return sh.marker_stats() + (sh.marker_counts(), sh.Ax(x), sh.ATx(p))


@pytest.mark.parametrize("bits", [8, 16])
def test_device_generator_and_file_upload_equal_the_host_twin_bit_for_bit(tmp_path, bits):
    """gv_synth_dosage_na at a shard offset, upload_dosage_file(missing=True) at S*N*bits/8 and upload_dosage of the same slice of
    synth.synth_dosage_na: the same reserved-code count, and identical statistics, counts and products (the accessor of the existing
    ingest test); the products of unit vectors read every code of a few rows back"""
    N, Mt, S, M, seed, ppm = 1203, 900, 317, 450, 99, 30000
    scale = 1.0 / 127.0 if bits == 8 else 1.0 / 16384.0           # what gv_synth_dosage_na sets
    full = synth.synth_dosage_na(N, Mt, seed, bits, ppm)
    R = dr.reserved(bits)
    path = str(tmp_path / "codes.bin")
    full.tofile(path)
    rng = np.random.default_rng(1)
    x = rng.standard_normal(M)
    p = np.zeros(4 * ((N + 3) // 4))
    p[:N] = rng.standard_normal(N)
    outs = []
    for how in ("array", "file", "synth"):
        with capi.Shard(N, M, Mt=Mt, S=S) as sh:
            if how == "file":
                sh.upload_dosage_file(path, bits, scale, missing=True)
            elif how == "array":
                sh.upload_dosage(full[S:S + M], scale, missing=True)
            else:
                sh.synth_dosage_na(seed, bits, ppm)
            info = sh.dosage_info()
            assert info == dict(bits=bits, scale=scale, missing=True, reserved=int((full[S:S + M] == R).sum()), na_kernels=True), (how, info)
            outs.append(outputs(sh, x, p))
            if how == "synth":
                # every code of rows 0, 1 and M - 1 through ATx of unit vectors: (code - mu') w / sqrt(N), an exact 0 where missing
                mave, msig = outs[-1][0], outs[-1][1]
                rows = [0, 1, M - 1]
                got = np.empty((3, N))
                e = np.zeros(p.size)
                for n in range(N):
                    e[n] = 1.0
                    got[:, n] = sh.ATx(e)[rows]
                    e[n] = 0.0
                sub = full[S:S + M][rows]
                codes = got * np.sqrt(N) / (msig[rows] * scale)[:, None] + (mave[rows] / scale)[:, None]
                assert np.array_equal(np.rint(codes[sub != R]).astype(np.int64), sub[sub != R].astype(np.int64))
                assert np.all(got[sub == R] == 0.0)
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert np.array_equal(a, b)
    st = dr.stats(full[S:S + M], bits, np.ones(N), scale)
    assert np.array_equal(outs[0][2], st["cnt"].astype(np.float64))
    assert rel(outs[0][3][:N], dr.ax(st, x, N)) < 1e-13


def test_gvamp_main_real_dosage_missing_equals_the_host_api_run_and_the_flag_reaches_the_kernels(tmp_path):
    N, Mt, it = 600, 1500, 3
    B = synth.synth_dosage_na(N, Mt, 41, 8, 30000)
    cfile, pfile = str(tmp_path / "codes.u8"), str(tmp_path / "y.phen")
    B.tofile(cfile)
    rng = np.random.default_rng(6)
    beta = rng.standard_normal(Mt) * (rng.random(Mt) < 0.05) * 0.15
    with capi.Shard(N, Mt) as sh:
        sh.upload_dosage(B, 1.0 / 127.0, missing=True)
        sh.compute_markers_statistics()
        g = sh.Ax(beta * np.sqrt(N))[:N]
    raw = 1.5 + 2.0 * (g + 0.7 * rng.standard_normal(N))
    with open(pfile, "w") as f:
        for i in range(N):
            f.write("F%d I%d %s\n" % (i, i, repr(float(raw[i]))))
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")

    def run(name, extra):
        out = str(tmp_path / name) + "/"
        cmd = [exe, "--run-mode", "infere", "--geno-format", "dosage8", "--bed-file", cfile, "--phen-files", pfile, "--N", str(N),
               "--Mt", str(Mt), "--out-dir", out, "--out-name", "d", "--iterations", str(it), "--probs", "0.9,0.1", "--vars", "0,0.01",
               "--rho", "0.5", "--CG-max-iter", "20", "--seed", "4"] + extra
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        return np.fromfile(out + "d_it_%d.bin" % it), res.stdout

    x_on, log_on = run("on", ["--dosage-missing", "1"])
    x_off, log_off = run("off", [])
    assert "the all-ones code is a missing entry" in log_on and "the all-ones code is a missing entry" not in log_off
    y = raw * np.sqrt((N - 1) / np.sum((raw - raw.mean()) ** 2))      # data::read_phen: scaled, not centred
    kw = dict(iterations=it, CG_max_iter=20, rho=0.5, seed=4, gam1=1e-6, gamw=2.0, fuse_solves=4)
    with capi.Shard(N, Mt) as sh:
        sh.upload_dosage_file(cfile, 8, 1.0 / 127.0, missing=True)
        r = hostapi.infere_linear(sh, y, [0.9, 0.1], [0.0, 0.01], **kw)
    print("driver vs host API rel %.3e; flag off vs on rel %.3e" % (rel(r.x1[it - 1], x_on), rel(x_off, x_on)))
    assert rel(r.x1[it - 1], x_on) < 1e-9
    assert np.all(np.isfinite(x_on)) and np.any(x_on != 0)
    assert rel(x_off, x_on) > 1e-3                                      # without the flag 255 is the value 2.008: another design matrix


def test_two_shards_over_host_transport_match_one_shard():
    N, Mt, nshards, bits = 1100, 2500, 2, 8
    full = synth.synth_dosage_na(N, Mt, 23, bits, 30000)
    scale = TEST_SCALE[bits]
    rng = np.random.default_rng(nshards)
    x = rng.standard_normal(Mt)
    p = np.zeros(4 * ((N + 3) // 4))
    p[:N] = rng.standard_normal(N)
    with capi.Shard(N, Mt) as sh:
        sh.upload_dosage(full, scale, missing=True)
        sh.compute_markers_statistics()
        z1, w1, c1 = sh.Ax(x), sh.ATx(p), sh.marker_counts()
        d = sh.vecM()
        sh.lmmse_mult(sh.vecM(x), 1.3, 0.2, d)
        l1 = d.download()
    results, errors = [None] * nshards, []
    size, modu = divmod(Mt, nshards)

    def work(rank):
        try:
            M = size + 1 if rank < modu else size
            S = sum(size + 1 if r < modu else size for r in range(rank))
            with capi.Shard(N, M, Mt=Mt, S=S) as sh:
                sh.upload_dosage(full[S:S + M], scale, missing=True)
                sh.comm_init_local(7900 + nshards, nshards, rank)
                sh.compute_markers_statistics()
                z, w = sh.Ax(x[S:S + M]), sh.ATx(p)
                d = sh.vecM()
                sh.lmmse_mult(sh.vecM(x[S:S + M]), 1.3, 0.2, d)
                results[rank] = (z, w, d.download(), sh.marker_counts())
        except Exception as e:   # noqa: BLE001
            errors.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(nshards)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not errors, errors
    for res in results:
        assert rel(res[0], z1) < 1e-9
    assert rel(np.concatenate([res[1] for res in results]), w1) < 1e-9
    assert rel(np.concatenate([res[2] for res in results]), l1) < 1e-9
    assert np.array_equal(np.concatenate([res[3] for res in results]), c1)
