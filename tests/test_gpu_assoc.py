"""gv_assoc_*: effect, standard error, t and p of the per-marker association test, for bed data in both kernel families and for
compact dosage data of both widths, against the long-double restatement of tests/assoc_restatement.py.

Bars.  p: rtol 1e-8, atol 0 (the project's p-value bar).  beta, se, t: the same restatement is evaluated in plain float64 numpy and
its deviation from long double measured; the GPU (another summation tree) is allowed 16 times that, never less than 1e-12.  The
deviation of a statistic is measured against its own magnitude plus the scale of its sampling noise -- |d beta| / (|beta| + se),
|d t| / (|t| + 1), |d se| / se -- because an estimate within its noise of zero has no meaningful relative error."""
import functools
import os
import subprocess

import numpy as np
import pytest

import assoc_restatement as ar
from gvamp_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
DTYPE = {8: np.uint8, 16: np.uint16}
TEST_SCALE = {8: 1.0 / 127.0, 16: 2.0 ** -14}
DYADIC = {8: 2.0 ** -6, 16: 2.0 ** -14}
KEYS = ("beta", "se", "t", "p")


def deviation(got, ref):
    """max deviation of beta / se / t from the long-double reference `ref`, every row compared (a LOCO row outside 1..23 holds exact
    zeros on both sides: its scale is 0 and any difference counts in full)"""
    g = {k: np.asarray(got[k], dtype=LD) for k in ("beta", "se", "t")}
    r = {k: np.asarray(ref[k], dtype=LD) for k in ("beta", "se", "t")}
    sb, ss = np.abs(r["beta"]) + r["se"], r["se"]
    return dict(beta=float(np.max(np.abs(g["beta"] - r["beta"]) / np.where(sb > 0, sb, LD(1)))),
                se=float(np.max(np.abs(g["se"] - r["se"]) / np.where(ss > 0, ss, LD(1)))),
                t=float(np.max(np.abs(g["t"] - r["t"]) / (np.abs(r["t"]) + 1))))


def check(got, ref, ref64, what, skip=None):
    """got (GPU) against ref (long double) under the bars of the module docstring; `skip`: rows left out of the comparisons"""
    keep = np.ones(ref["t"].shape, dtype=bool)
    if skip is not None:
        keep[skip] = False
    gk, rk, r64 = ({k: np.asarray(d[k])[keep] for k in d} for d in (got, ref, ref64))
    assert np.all(np.isfinite(rk["t"])), what
    for k in KEYS:
        assert np.all(np.isfinite(gk[k])), (what, k)
    dev64, devg = deviation(r64, rk), deviation(gk, rk)
    for k in ("beta", "se", "t"):
        bound = max(16.0 * dev64[k], 1e-12)
        print("%s %-4s float64 dev %.3e  GPU dev %.3e  ratio %.2f  bound %.3e" % (what, k, dev64[k], devg[k],
                                                                                 devg[k] / dev64[k] if dev64[k] > 0 else float("inf"), bound))
        assert devg[k] <= bound, (what, k, devg[k], bound)
    rp = rk["p"].astype(np.float64)
    pos = rp > 0                                              # (exact zeros -- underflow, LOCO rows outside 1..23 -- compare as 0 == 0 below)
    print("%s p    max rel %.3e  (min p > 0 %.3e)" % (what, float(np.max(np.abs(gk["p"][pos] / rp[pos] - 1))) if pos.any() else 0.0,
                                                      rp[pos].min() if pos.any() else 0.0))
    assert np.allclose(gk["p"], rp, rtol=1e-8, atol=0), what
    nz = gk["se"] != 0                                        # (se == 0: the exact zeros of a LOCO row outside 1..23)
    assert np.all(np.sign(gk["t"][nz]) == np.sign(gk["beta"][nz])) and np.all(gk["se"][nz] > 0), what


def na_mask(N, with_na):
    na = np.ones(N)
    if with_na:
        na[3::7] = 0.0
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    for n in np.nonzero(na)[0]:
        m4[n >> 2] |= 1 << (n & 3)
    return m4, na, int(na.sum())


def chrom_layout(M):
    """sorted chromosomes: a few markers outside 1..23 at both ends, chromosome 1 of a single marker, chromosome 2 of five (no
    multiple of the kernel's four rows per wave), chromosome 3 empty, the rest spread over 4..23"""
    if M < 100:
        return np.array(([1, 2, 30] + [30] * M)[:M], dtype=np.int32)
    body = M - 2 - 1 - 5 - 2
    rest = 4 + (np.arange(body) * 20) // body
    return np.concatenate([[0, 0], [1], [2] * 5, rest, [24, 24]]).astype(np.int32)


def effects(N, M, const_row, rng):
    """sparse x1_hat with a few strong effects of both signs (p down to 1e-100 and below at N >= 1000)"""
    x1 = np.zeros(M)
    amp = np.sqrt(N) * np.array([1.2, -0.9, 0.5, -0.3, 0.15, -0.05])
    idx = [i for i in np.unique(np.linspace(0, M - 1, 6).astype(int)) if i != const_row]
    x1[idx] = amp[:len(idx)]
    x1 += (rng.random(M) < 0.02) * rng.standard_normal(M) * 0.05 * np.sqrt(N)
    x1[const_row] = 0.7                                     # (a constant row's value is 0: its effect moves nothing)
    return x1


SHAPES = [(7, 3), (1003, 700), (4099, 301), (257, 70001)]


@functools.lru_cache(maxsize=1)
def dosage_case(bits, N, M, with_na):
    """inputs and the restatement's results of one case (long double and float64, LOO and LOCO), computed once, left unchanged"""
    rng = np.random.default_rng(1000 * bits + N + M + int(with_na))
    B = synth.synth_dosage(N, M, N * 5 + M, bits)
    m4, na, nonas = na_mask(N, with_na)
    const_row = M // 2
    B[const_row] = 200 if bits == 8 else 40001
    if with_na:
        B[const_row, 3::7] = 7                                 # constant among the individuals with a phenotype only
    scale = TEST_SCALE[bits]
    chrom = chrom_layout(M)
    assert 1 <= chrom[const_row] <= 23
    x1 = effects(N, M, const_row, rng)
    V, b, msig = ar.dosage_columns(B, scale, na)
    npad = 4 * ((N + 3) // 4)
    z1 = np.zeros(npad)
    z1[:N] = ((V.T @ x1.astype(LD)) / np.sqrt(LD(N))).astype(np.float64)      # A x1_hat (no phenotype mask in the dense Ax)
    y = np.zeros(npad)
    y[:N] = z1[:N] + rng.standard_normal(N)
    y[:N][na == 0] = 1e300                                       # whatever a caller may leave at the NA slots
    y[N:] = -1e300                                               # ... and in the padding
    ref = {"loo": ar.assoc(V, b, na, y, z1, x1), "loco": ar.assoc(V, b, na, y, z1, x1, chrom=chrom)}
    V64 = ar.dosage_columns(B, scale, na, dtype=np.float64)[0]
    del V
    ref64 = {"loo": ar.assoc(V64, None, na, y, z1, x1, dtype=np.float64, with_p=False),
             "loco": ar.assoc(V64, None, na, y, z1, x1, chrom=chrom, dtype=np.float64, with_p=False)}
    for r in ref64.values():
        r["p"] = np.zeros(M)
    for a in (B, x1, y, z1, chrom):
        a.setflags(write=False)
    return dict(B=B, m4=m4, nonas=nonas, scale=scale, chrom=chrom, x1=x1, y=y, z1=z1, const_row=const_row, ref=ref, ref64=ref64)


@pytest.mark.parametrize("with_na", [False, True])
@pytest.mark.parametrize("N,M", SHAPES)
@pytest.mark.parametrize("bits", [8, 16])
def test_dosage_vs_long_double_restatement(bits, N, M, with_na):
    c = dosage_case(bits, N, M, with_na)
    cr, chrom = c["const_row"], c["chrom"]
    with capi.Shard(N, M) as sh:
        sh.upload_dosage(c["B"], c["scale"])
        if with_na:
            sh.set_mask(c["m4"], c["nonas"])
        sh.compute_markers_statistics()
        assert sh.marker_stats()[1][cr] == 1.0
        dz, dy, dx = sh.vecN(c["z1"]), sh.vecN(c["y"]), sh.vecM(c["x1"])
        loo = sh.assoc_calc(dz, dy, dx)
        loco, pred = sh.assoc_calc(dz, dy, dx, chrom=chrom, want_pred=True)
        assert all(np.array_equal(sh.assoc_calc(dz, dy, dx)[k], loo[k], equal_nan=True) for k in KEYS)      # bit-reproducible
    for res, name in ((loo, "loo"), (loco, "loco")):
        assert all(np.isnan(res[k][cr]) for k in KEYS), (name, [res[k][cr] for k in KEYS])       # the constant row
        assert all(np.isnan(c["ref"][name][k][cr]) for k in KEYS)
        check(res, c["ref"][name], c["ref64"][name], "dosage%d %dx%d na=%d %s" % (bits, N, M, with_na, name), skip=[cr])
    outside = (chrom < 1) | (chrom > 23)
    assert outside.any()
    for k in KEYS:
        assert np.all(loco[k][outside] == 0.0) and not np.any(np.signbit(loco[k][outside]))
    assert pred.shape == (23, 4 * ((N + 3) // 4)) and np.all(pred[2] == 0)          # chromosome 3 is empty
    if N >= 1000:
        p = np.delete(c["ref"]["loo"]["p"], cr)
        assert p.min() < 1e-100 and p.max() > 0.5
    if M > 3:
        t = np.delete(loo["t"], cr)
        assert (t > 0).any() and (t < 0).any()


# ---- dosage equals bed -------------------------------------------------------------------------------------------------------------
def bed_as_codes(G, bits):
    """hard calls as codes: 64 {0, 1, 2} at scale 2^-6, 16384 {0, 1, 2} at scale 2^-14"""
    return (G * (64 if bits == 8 else 16384)).astype(DTYPE[bits])


@functools.lru_cache(maxsize=1)
def bed_without_missing(oracle_mod):
    N, M = 1203, 900
    rng = np.random.default_rng(33)
    bed = synth.synth_bed(N, M, seed=19, miss_ppm=0)
    m4, na, nonas = na_mask(N, True)
    x1 = rng.standard_normal(M) * (rng.random(M) < 0.05) * 3.0
    chrom = np.sort(rng.integers(1, 24, M)).astype(np.int32)
    chrom[chrom == 7] = 8
    mave, msig = oracle_mod.marker_stats(bed, N, M, mask4=m4, nonas=nonas)
    z1 = oracle_mod.ax(bed, N, M, mave, msig, x1, mask4=m4)
    y = np.zeros(z1.size)
    y[:N] = (z1[:N] + rng.standard_normal(N)) * na
    o_loo = oracle_mod.pvals(bed, N, M, z1, y, x1, mask4=m4, nonas=nonas, nthreads=4)
    o_loco = oracle_mod.pvals(bed, N, M, z1, y, x1, chrom=chrom, mask4=m4, nonas=nonas, nthreads=4)
    with capi.Shard(N, M) as sh:
        sh.upload_bed(bed)
        sh.set_mask(m4, nonas)
        sh.compute_markers_statistics()
        dz, dy, dx = sh.vecN(z1), sh.vecN(y), sh.vecM(x1)
        b_loo, b_loco = sh.assoc_calc(dz, dy, dx), sh.assoc_calc(dz, dy, dx, chrom=chrom)
    G, have = ar.decode_bed(bed, N, M)
    assert have.all()
    return N, M, G, m4, nonas, x1, chrom, z1, y, o_loo, o_loco, b_loo, b_loco


@pytest.mark.parametrize("bits", [8, 16])
def test_dosage_on_codes_of_a_bed_equals_the_bed_path_and_the_oracle(oracle, bits):
    N, M, G, m4, nonas, x1, chrom, z1, y, o_loo, o_loco, b_loo, b_loco = bed_without_missing(oracle)
    with capi.Shard(N, M) as sh:
        sh.upload_dosage(bed_as_codes(G, bits), DYADIC[bits])
        sh.set_mask(m4, nonas)
        sh.compute_markers_statistics()
        # z1 of the bed data is masked at the NA individuals, the dense Ax is not: p is masked there either way
        dz, dy, dx = sh.vecN(z1), sh.vecN(y), sh.vecM(x1)
        d_loo, d_loco = sh.assoc_calc(dz, dy, dx), sh.assoc_calc(dz, dy, dx, chrom=chrom)
    for d, b, o, name in ((d_loo, b_loo, o_loo, "loo"), (d_loco, b_loco, o_loco, "loco")):
        print("%s: p dosage/bed max rel %.3e, t max rel %.3e" % (name, np.max(np.abs(d["p"] / b["p"] - 1)), np.max(np.abs(d["t"] / b["t"] - 1))))
        assert np.allclose(d["p"], b["p"], rtol=1e-8, atol=0) and np.allclose(d["t"], b["t"], rtol=1e-9, atol=0)
        assert np.allclose(d["p"], o, rtol=1e-8, atol=0) and np.allclose(b["p"], o, rtol=1e-8, atol=0)
        assert np.allclose(d["beta"], b["beta"], rtol=1e-9, atol=0) and np.allclose(d["se"], b["se"], rtol=1e-9, atol=0)


# ---- bed data, both kernel families ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def bed_case(oracle_mod):
    """the case of test_gpu_pvals.py::test_pvals_loo_and_loco_vs_oracle with the restatement's results"""
    N, M = 1203, 900
    rng = np.random.default_rng(21)
    bed = synth.synth_bed(N, M, seed=55, miss_ppm=15000)
    present = rng.random(N) >= 0.02
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    for n in np.nonzero(present)[0]:
        m4[n >> 2] |= 1 << (n & 3)
    nonas = int(present.sum())
    x1 = rng.standard_normal(M) * (rng.random(M) < 0.05) * 3.0
    chrom = np.sort(rng.integers(1, 24, M)).astype(np.int32)
    chrom[chrom == 7] = 8
    mave, msig = oracle_mod.marker_stats(bed, N, M, mask4=m4, nonas=nonas)
    z1 = oracle_mod.ax(bed, N, M, mave, msig, x1, mask4=m4)
    y = np.zeros(4 * ((N + 3) // 4))
    y[:N] = (z1[:N] + rng.standard_normal(N)) * present
    G, have = ar.decode_bed(bed, N, M)
    ref, ref64 = {}, {}
    for name, ch in (("loo", None), ("loco", chrom)):
        ref[name] = ar.assoc(*ar.bed_columns(G, have, mave, msig), present, y, z1, x1, chrom=ch)
        ref64[name] = ar.assoc(*ar.bed_columns(G, have, mave, msig, dtype=np.float64), present, y, z1, x1, chrom=ch, dtype=np.float64,
                               with_p=False)
        ref64[name]["p"] = np.zeros(M)
    return N, M, bed, m4, nonas, x1, chrom, z1, y, ref, ref64


@pytest.mark.parametrize("mode", [0, 1])
def test_bed_p_is_bit_identical_to_gv_pvals_and_the_rest_holds(oracle, mode):
    N, M, bed, m4, nonas, x1, chrom, z1, y, ref, ref64 = bed_case(oracle)
    with capi.Shard(N, M, anchor=(mode == 0)) as sh:
        sh.upload_bed(bed)
        sh.set_mask(m4, nonas)
        sh.set_kernel_mode(mode)
        sh.compute_markers_statistics()
        dz, dy, dx = sh.vecN(z1), sh.vecN(y), sh.vecM(x1)
        p_loo, p_loco = sh.pvals_calc(dz, dy, dx), sh.pvals_calc(dz, dy, dx, chrom=chrom)
        a_loo, a_loco = sh.assoc_calc(dz, dy, dx), sh.assoc_calc(dz, dy, dx, chrom=chrom)
        assert np.array_equal(sh.pvals_calc(dz, dy, dx), p_loo)            # (and gv_pvals_* after gv_assoc_* is what it was before)
    assert np.array_equal(a_loo["p"], p_loo) and np.array_equal(a_loco["p"], p_loco)     # nothing existing moved
    check(a_loo, ref["loo"], ref64["loo"], "bed mode %d loo" % mode)
    check(a_loco, ref["loco"], ref64["loco"], "bed mode %d loco" % mode)


# ---- the index list ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
def test_loco_on_one_chromosome_without_effects_equals_loo_bit_for_bit(bits):
    """every marker on chromosome 1 and x1_hat = 0: the same residual, the rows through the index list instead of the identity"""
    N, M = 2051, 1301
    rng = np.random.default_rng(bits)
    B = synth.synth_dosage(N, M, 77, bits)
    m4, na, nonas = na_mask(N, True)
    npad = 4 * ((N + 3) // 4)
    z1, y = np.zeros(npad), np.zeros(npad)
    z1[:N], y[:N] = rng.standard_normal(N), rng.standard_normal(N) * 2
    with capi.Shard(N, M) as sh:
        sh.upload_dosage(B, TEST_SCALE[bits])
        sh.set_mask(m4, nonas)
        sh.compute_markers_statistics()
        dz, dy, dx = sh.vecN(z1), sh.vecN(y), sh.vecM(np.zeros(M))
        loo = sh.assoc_calc(dz, dy, dx)
        loco = sh.assoc_calc(dz, dy, dx, chrom=np.ones(M, dtype=np.int32))
    for k in KEYS:
        assert np.all(np.isfinite(loo[k])) and np.array_equal(loo[k], loco[k]), k
    assert np.any(loo["t"] != 0)


# ---- sharding ----------------------------------------------------------------------------------------------------------------------
def test_forced_multi_reproduces_one_rank_bit_for_bit():
    N, M = 2049, 1300
    rng = np.random.default_rng(4)
    B = synth.synth_dosage(N, M, 4, 8)
    chrom = chrom_layout(M)
    x1 = effects(N, M, M // 2, rng)
    npad = 4 * ((N + 3) // 4)
    y = np.zeros(npad)
    y[:N] = rng.standard_normal(N)
    outs = []
    for transport in (0, 1):
        with capi.Shard(N, M) as sh:
            if transport:
                sh._ck(sh.L.gv_debug_force_multi(sh.h, transport, 0))
            sh.upload_dosage(B, TEST_SCALE[8])
            sh.compute_markers_statistics()
            dx = sh.vecM(x1)
            dz, dy = sh.vecN(sh.Ax(x1)), sh.vecN(y)
            loo = sh.assoc_calc(dz, dy, dx)
            loco, pred = sh.assoc_calc(dz, dy, dx, chrom=chrom, want_pred=True)
            outs.append([loo[k] for k in KEYS] + [loco[k] for k in KEYS] + [pred])
    for a, b in zip(outs[0], outs[1]):
        assert np.all(np.isfinite(a)) and np.array_equal(a, b)
    assert np.any(outs[0][6] != 0)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    N, M = 300, 200
    chrom = np.ones(M, dtype=np.int32)
    with capi.Shard(N, M) as sh:
        sh.upload_meth(synth.synth_meth(N, M, 3))
        sh.compute_markers_statistics()
        z1, y, x1 = sh.vecN(), sh.vecN(), sh.vecM()
        for ch in (None, chrom):
            with pytest.raises(capi.GvError, match="gv_assoc: not available for methylation data"):
                sh.assoc_calc(z1, y, x1, chrom=ch)
    with capi.Shard(N, M) as sh:
        sh.synth_dosage(1, 8)
        z1, y, x1 = sh.vecN(), sh.vecN(), sh.vecM()
        with pytest.raises(capi.GvError, match="gv_assoc: marker statistics must be computed first"):
            sh.assoc_calc(z1, y, x1)
        sh.compute_markers_statistics()
        for bad in ((x1, y, x1), (z1, x1, x1), (z1, y, z1)):
            with pytest.raises(capi.GvError, match="gv_assoc: bad vector spaces"):
                sh.assoc_calc(*bad)
            with pytest.raises(capi.GvError, match="gv_assoc: bad vector spaces"):
                sh.assoc_calc(*bad, chrom=chrom)
        out = capi.AssocOut()
        with pytest.raises(capi.GvError, match="chrom is NULL"):
            sh._ck(sh.L.gv_assoc_loco(sh.h, z1.h, y.h, x1.h, None, capi.C.byref(out), None))
        with pytest.raises(capi.GvError, match="out is NULL"):
            sh._ck(sh.L.gv_assoc_loo(sh.h, z1.h, y.h, x1.h, None))
        sh._ck(sh.L.gv_assoc_loo(sh.h, z1.h, y.h, x1.h, capi.C.byref(out)))       # every output NULL: computed, nothing copied out
        # gv_pvals_* on dosage data is still refused
        with pytest.raises(capi.GvError, match=r"gv_pvals: not available for compact dosage data \(8-bit codes\)"):
            sh.pvals_calc(z1, y, x1)
        with pytest.raises(capi.GvError, match=r"gv_pvals: not available for compact dosage data \(8-bit codes\)"):
            sh.pvals_calc(z1, y, x1, chrom=chrom)


# ---- driver ------------------------------------------------------------------------------------------------------------------------
def test_gvamp_main_real_store_assoc_on_a_dosage8_file(tmp_path):
    N, Mt, it = 600, 1500, 3
    B = synth.synth_dosage(N, Mt, 41, 8)
    cfile, pfile, bim = str(tmp_path / "codes.u8"), str(tmp_path / "y.phen"), str(tmp_path / "d.bim")
    B.tofile(cfile)
    chrom = np.repeat(np.arange(1, 13), Mt // 12)
    with open(bim, "w") as f:
        for i, ch in enumerate(chrom):
            f.write("%s\trs%d\t0\t%d\tA\tG\n" % ("X" if ch == 12 else str(ch), i, i + 1))
    chrom = np.where(chrom == 12, 23, chrom).astype(np.int32)
    rng = np.random.default_rng(6)
    beta = rng.standard_normal(Mt) * (rng.random(Mt) < 0.05) * 0.15
    with capi.Shard(N, Mt) as sh:
        sh.upload_dosage(B, 1.0 / 127.0)
        sh.compute_markers_statistics()
        g = sh.Ax(beta * np.sqrt(N))[:N]
    raw = 1.5 + 2.0 * (g + 0.7 * rng.standard_normal(N))
    with open(pfile, "w") as f:
        for i in range(N):
            f.write("F%d I%d %s\n" % (i, i, repr(float(raw[i]))))
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
    files = ["d_assoc_%s%s.bin" % (loco, k) for loco in ("", "LOCO_") for k in KEYS]

    def run(out, extra):
        cmd = [exe, "--run-mode", "infere", "--geno-format", "dosage8", "--bed-file", cfile, "--bim-file", bim, "--phen-files", pfile,
               "--N", str(N), "--Mt", str(Mt), "--out-dir", out, "--out-name", "d", "--iterations", str(it), "--probs", "0.9,0.1",
               "--vars", "0,0.01", "--rho", "0.5", "--CG-max-iter", "20", "--seed", "4"] + extra
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        return res.stdout

    out = str(tmp_path / "plain") + "/"
    run(out, [])
    assert not [f for f in os.listdir(out) if "assoc" in f]
    out = str(tmp_path / "assoc") + "/"
    run(out, ["--store-assoc", "1"])
    assert all(os.path.exists(out + f) for f in files), sorted(os.listdir(out))
    assert not [f for f in os.listdir(out) if "pvals" in f]                 # independent of --store-pvals
    x1 = np.fromfile(out + "d_it_%d.bin" % it) * np.sqrt(N)
    y = np.zeros(4 * ((N + 3) // 4))
    y[:N] = raw * np.sqrt((N - 1) / np.sum((raw - raw.mean()) ** 2))        # data::read_phen: scaled, not centred
    with capi.Shard(N, Mt) as sh:
        sh.upload_dosage_file(cfile, 8, 1.0 / 127.0)
        sh.compute_markers_statistics()
        dx = sh.vecM(x1)
        dz, dy = sh.vecN(sh.Ax(x1)), sh.vecN(y)
        loo, loco = sh.assoc_calc(dz, dy, dx), sh.assoc_calc(dz, dy, dx, chrom=chrom)
    for res, tag in ((loo, ""), (loco, "LOCO_")):
        for k in KEYS:
            got = np.fromfile(out + "d_assoc_%s%s.bin" % (tag, k))
            assert got.shape == (Mt,) and np.all(np.isfinite(got))
            assert np.allclose(got, res[k], rtol=1e-7, atol=0), (tag, k, np.max(np.abs(got / res[k] - 1)))
    assert loo["p"].min() < 1e-3
