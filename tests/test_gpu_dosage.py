"""Compact dense data: 8- / 16-bit dosage codes (X = scale * B) behind the same C ABI as the dense fp64 kind.

The definitions of include/gvamp.h (statistics in code units, products with (b - mu') formed per entry) are restated below in numpy
long double; the kind is tied to the dense fp64 path through dyadic scales and to the oracle through bed data whose hard calls are
written as codes."""
import functools
import itertools
import os
import subprocess
import threading

import numpy as np
import pytest

from gvamp_amd import capi, hostapi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS, VARS = [0.90, 0.07, 0.03], [0, 0.001, 0.01]
LD = np.longdouble
DTYPE = {8: np.uint8, 16: np.uint16}
TEST_SCALE = {8: 1.0 / 127.0, 16: 2.0 ** -14}        # the scales of the restatement tests: one non-dyadic, one dyadic
DYADIC = {8: 2.0 ** -6, 16: 2.0 ** -14}
LAYOUT = {8: 4, 16: 5}


def rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (nb if nb > 0 else 1.0))


def na_mask(N, with_na):
    """(mask4 nibbles, na[N], nonas): every 7th individual from 3 on has no phenotype (the pattern of test_gpu_meth.py)"""
    na = np.ones(N)
    if with_na:
        na[3::7] = 0.0
    mb = (N + 3) // 4
    m4 = np.zeros(mb, dtype=np.uint8)
    for n in range(N):
        if na[n]:
            m4[n >> 2] |= 1 << (n & 3)
    return m4, na, int(na.sum())


def codes_matrix(N, M, bits, seed):
    """synthetic codes over the full range; row 0 constant at a non-zero code, row 1 zeros but for one entry at the maximum code"""
    B = synth.synth_dosage(N, M, seed, bits)
    B[0] = 200 if bits == 8 else 40001                     # (in the top half of the range: a sign extension would show)
    if M >= 2:
        B[1] = 0
        B[1, N // 2] = (1 << bits) - 1
    return B


# ---- long-double restatement of the definitions ---------------------------------------------------------------------------------
def ref_code_stats(B, na, nonas):
    """mu' = (sum_present b) / nonas with the integer sum exact; q = sum_present (b - mu')^2; D = B - mu'"""
    s = (B.astype(np.int64) * na.astype(np.int64)[None, :]).sum(axis=1)
    mu = s.astype(LD) / LD(nonas)
    D = B.astype(LD) - mu[:, None]
    q = ((D * D) * na.astype(LD)[None, :]).sum(axis=1)
    return mu, q, D


def ref_stats(mu, q, nonas, scale, alpha):
    mave = LD(scale) * mu
    sd = LD(scale) * np.sqrt(np.where(q != 0, q, LD(1)) / LD(max(nonas - 1, 1)))
    msig = np.where(q != 0, sd ** LD(-alpha), LD(1))
    return mave, msig


def ref_atx(Dp, msig, scale, N):
    """Dp = D @ p[:N]: out[m] = msig[m] scale sum_j (b - mu') p[j] / sqrt(N)"""
    return msig * LD(scale) * Dp / np.sqrt(LD(N))


def ref_ax(D, msig, scale, v, npad):
    N = D.shape[1]
    out = np.zeros(npad, dtype=LD)
    out[:N] = (D.T @ (msig * LD(scale) * v.astype(LD))) / np.sqrt(LD(N))
    return out


@functools.lru_cache(maxsize=2)
def restatement(bits, N, M, with_na):
    """everything of a case that does not depend on alpha, computed once and left unchanged"""
    B = codes_matrix(N, M, bits, N * 7 + M)
    m4, na, nonas = na_mask(N, with_na)
    rng = np.random.default_rng(N + M)
    npad = 4 * ((((N + 3) // 4) + 63) // 64 * 64)
    x, x2 = rng.standard_normal(M), rng.standard_normal(M)
    p, p2 = np.zeros(npad), np.zeros(npad)
    p[:N], p2[:N] = rng.standard_normal(N), rng.standard_normal(N)
    mu, q, D = ref_code_stats(B, na, nonas)
    out = dict(B=B, m4=m4, na=na, nonas=nonas, x=x, x2=x2, p=p, p2=p2, mu=mu, q=q, D=D, Dp=D @ p[:N].astype(LD))
    for a in (B, x, x2, p, p2):
        a.setflags(write=False)
    return out


SHAPES = [(1, 1), (5, 3), (1003, 700), (4099, 3001), (257, 70001)]
CASES = [(bits, N, M, with_na, alpha) for bits, (N, M), with_na, alpha in
         itertools.product((8, 16), SHAPES, (False, True), (1.0, 0.3))]


@pytest.mark.parametrize("bits,N,M,with_na,alpha", CASES)
def test_products_and_statistics_vs_long_double_restatement(bits, N, M, with_na, alpha):
    c = restatement(bits, N, M, with_na)
    scale, nonas, x, x2, p, p2 = TEST_SCALE[bits], c["nonas"], c["x"], c["x2"], c["p"], c["p2"]
    assert np.any(c["B"] >= (1 << (bits - 1)))               # codes of the top half of the range are in the matrix
    rm, rs = ref_stats(c["mu"], c["q"], nonas, scale, alpha)
    with capi.Shard(N, M) as sh:
        sh.upload_dosage(c["B"], scale)
        assert sh.get_layout() == LAYOUT[bits]
        if with_na:
            sh.set_mask(c["m4"], nonas)
        sh.compute_markers_statistics(alpha)
        mave, msig = sh.marker_stats()
        npad = 4 * sh.mbytes
        assert npad <= p.size
        p, p2 = p[:npad], p2[:npad]
        print("mave max rel %.3e  msig max rel %.3e" % (float(np.max(np.abs(mave - rm) / np.maximum(np.abs(rm), LD(1e-300)))),
                                                        float(np.max(np.abs(msig - rs) / np.abs(rs)))))
        assert np.allclose(mave, rm.astype(np.float64), rtol=1e-13, atol=0)
        assert np.allclose(msig, rs.astype(np.float64), rtol=1e-13, atol=0)
        assert msig[0] == 1.0                                 # the constant row: q == 0 exactly, whatever the scale
        z, w = sh.Ax(x), sh.ATx(p)
        rz = ref_ax(c["D"], rs, scale, x, npad)
        rw = ref_atx(c["Dp"], rs, scale, N)
        print("Ax rel %.3e  ATx rel %.3e" % (rel(z, rz), rel(w, rw)))
        assert rel(z, rz) < 1e-13
        assert rel(w, rw) < 1e-13
        assert np.all(z[N:] == 0.0)                                    # exact zeros at the pad slots
        if with_na and N > 3:
            assert np.all(z[3:N:7] != 0.0)                             # no phenotype mask in Ax, as the dense fp64 kind
        assert np.array_equal(sh.Ax(x), z) and np.array_equal(sh.ATx(p), w)     # bit-reproducible
        # two-vector forms: each slot bit-equal to the one-vector call on that vector
        dx, dx2, dz, dz2 = sh.vecM(x), sh.vecM(x2), sh.vecN(), sh.vecN()
        sh.ax2_dev(dx, dx2, dz, dz2)
        assert np.array_equal(dz.download(), z) and np.array_equal(dz2.download(), sh.Ax(x2))
        dp, dp2, dw, dw2 = sh.vecN(p), sh.vecN(p2), sh.vecM(), sh.vecM()
        sh.atx2_dev(dp, dp2, dw, dw2)
        assert np.array_equal(dw.download(), w) and np.array_equal(dw2.download(), sh.ATx(p2))
        # lmmse_mult: tau A^T A v + gam2 v
        tau, gam2 = 1.7, 0.35
        d = sh.vecM()
        sh.lmmse_mult(dx, tau, gam2, d)
        expect = LD(tau) * ref_atx(c["D"] @ rz[:N], rs, scale, N) + LD(gam2) * x.astype(LD)
        print("lmmse_mult rel %.3e" % rel(d.download(), expect))
        assert rel(d.download(), expect) < 1e-13


@pytest.mark.parametrize("bits", [8, 16])
def test_matches_the_fp64_dense_path_on_a_dyadic_scale(bits):
    """scale * B is exact in fp64 for a dyadic scale, so upload_meth(scale * B) is the same design matrix (no constant rows: in
    value units the fp64 kind's q of a constant row is rounding, not zero)"""
    N, M = 1003, 700
    scale = DYADIC[bits]
    B = synth.synth_dosage(N, M, 31, bits)
    assert np.all(B.min(axis=1) != B.max(axis=1))
    m4, na, nonas = na_mask(N, True)
    rng = np.random.default_rng(8)
    x = rng.standard_normal(M)
    with capi.Shard(N, M) as sd, capi.Shard(N, M) as sm:
        sd.upload_dosage(B, scale)
        sm.upload_meth(B.astype(np.float64) * scale)
        p = np.zeros(4 * sd.mbytes)
        p[:N] = rng.standard_normal(N)
        for s in (sd, sm):
            s.set_mask(m4, nonas)
        for alpha in (1.0, 0.3):
            sd.compute_markers_statistics(alpha)
            sm.compute_markers_statistics(alpha)
            (dm, ds), (mm, ms) = sd.marker_stats(), sm.marker_stats()
            assert np.allclose(dm, mm, rtol=1e-13, atol=0) and np.allclose(ds, ms, rtol=1e-13, atol=0)
            assert rel(sd.Ax(x), sm.Ax(x)) < 1e-12 and rel(sd.ATx(p), sm.ATx(p)) < 1e-12


# ---- tie to the oracle through bed data -----------------------------------------------------------------------------------------
def decode_bed(bed, N, M):
    """PLINK 2-bit rows -> hard calls 0 / 1 / 2 (no missing codes expected)"""
    mb = (N + 3) // 4
    b = np.asarray(bed, dtype=np.uint8).reshape(M, mb)
    codes = np.stack([(b >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(M, 4 * mb)[:, :N]
    assert not np.any(codes == 1)
    return np.choose(codes, [2, 0, 1, 0]).astype(np.int64)


def bed_as_codes(G, bits):
    """hard calls as codes: 64 {0, 1, 2} at scale 2^-6, 16384 {0, 1, 2} at scale 2^-14"""
    return (G * (64 if bits == 8 else 16384)).astype(DTYPE[bits])


_VAMP_KW = dict(iterations=4, CG_max_iter=30, rho=0.5, seed=7, gam1=1e-8, gamw=2.0)


@functools.lru_cache(maxsize=None)
def _bed_runs(fuse):
    """the bed run and the oracle run the dosage runs are held against, once per fuse level"""
    from oracle import gvoracle
    N, M = 1200, 3000
    bed = synth.synth_bed(N, M, seed=17, miss_ppm=0)
    beta, y = gvoracle.sim_phen(bed, N, M, 0.5, 300, 7, nthreads=4)
    ref = gvoracle.infere(bed, N, M, y, PROBS, VARS, **_VAMP_KW)
    with capi.Shard(N, M, anchor=True) as sb:
        sb.upload_bed(bed)
        rb = hostapi.infere_linear(sb, y, PROBS, VARS, fuse_solves=fuse, **_VAMP_KW)
    return N, M, decode_bed(bed, N, M), y, ref, rb


@pytest.mark.parametrize("fuse", [0, 4])
@pytest.mark.parametrize("bits", [8, 16])
def test_vamp_on_codes_of_a_bed_matches_bed_run_and_oracle(oracle, bits, fuse):
    N, M, G, y, ref, rb = _bed_runs(fuse)
    with capi.Shard(N, M) as sd:
        sd.upload_dosage(bed_as_codes(G, bits), DYADIC[bits])
        rd = hostapi.infere_linear(sd, y, PROBS, VARS, fuse_solves=fuse, **_VAMP_KW)
    assert rd.niter == rb.niter == ref.niter
    print("x_hat rel to bed run %.3e, to oracle %.3e" % (rel(rd.x_est, rb.x_est), rel(rd.x_est, ref.x_est)))
    assert rel(rd.x_est, rb.x_est) < 1e-9 and rel(rd.x_est, ref.x_est) < 1e-9
    for it in range(rd.niter):
        t, b, o = rd.trace[it], rb.trace[it], ref.trace[it]
        assert (t["cg_iters"], t["onsager_iters"]) == (b["cg_iters"], b["onsager_iters"]) == (o["cg_iters"], o["onsager_iters"])
        if fuse == 4:
            assert t["n_ax_pass"] < t["n_ax"]          # the two-vector pass over the codes is in use


def test_probit_on_codes_of_a_bed_matches_bed_run(oracle):
    N, M = 1001, 1500
    bed = synth.synth_bed(N, M, seed=11, miss_ppm=0)
    beta, yl = oracle.sim_phen(bed, N, M, 0.6, 100, 11)
    y = (yl > np.median(yl)).astype(np.float64)
    kw = dict(iterations=5, CG_max_iter=30, rho=0.5, seed=3, gam1=1e-8, gamw=1.0, model="bin_class")
    with capi.Shard(N, M, anchor=True) as sb:
        sb.upload_bed(bed)
        rb = hostapi.infere_linear(sb, y, PROBS, VARS, **kw)
    with capi.Shard(N, M) as sd:
        sd.upload_dosage(bed_as_codes(decode_bed(bed, N, M), 8), DYADIC[8])
        rd = hostapi.infere_linear(sd, y, PROBS, VARS, **kw)
    assert rd.niter == rb.niter
    assert rel(rd.x_est, rb.x_est) < 1e-9


# ---- ingest -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
def test_ingest_paths_agree_and_a_short_file_names_the_marker(tmp_path, bits):
    """upload_dosage_file at S*N*bits/8, upload_dosage of the same slice and synth_dosage against synth.synth_dosage: identical"""
    N, Mt, S, M, seed = 1203, 900, 317, 450, 99
    scale = 1.0 / 127.0 if bits == 8 else 1.0 / 16384.0           # what gv_synth_dosage sets
    full = synth.synth_dosage(N, Mt, seed, bits)
    path = str(tmp_path / "codes.bin")
    full.tofile(path)
    rng = np.random.default_rng(1)
    x = rng.standard_normal(M)
    p = np.zeros(4 * ((N + 3) // 4))
    p[:N] = rng.standard_normal(N)
    outs = []
    for how in ("file", "array", "synth"):
        with capi.Shard(N, M, Mt=Mt, S=S) as sh:
            if how == "file":
                sh.upload_dosage_file(path, bits, scale)          # default offset S * N * bits / 8
            elif how == "array":
                sh.upload_dosage(full[S:S + M], scale)
            else:
                sh.synth_dosage(seed, bits)
            assert sh.get_layout() == LAYOUT[bits]
            sh.compute_markers_statistics()
            outs.append(sh.marker_stats() + (sh.Ax(x), sh.ATx(p)))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert np.array_equal(a, b)
    assert np.all(np.isfinite(outs[0][2])) and np.any(outs[0][3] != 0)
    with capi.Shard(N, M, Mt=Mt, S=S) as sh:
        with pytest.raises(capi.GvError, match=r"marker %d .*short file" % (S + M - 1)):
            sh.upload_dosage_file(path, bits, scale, offset=(Mt - M + 1) * N * (bits // 8))
        assert sh.get_layout() == 0                                # nothing half-read stays resident


def test_bad_width_or_scale_is_refused():
    N, M = 64, 8
    codes = np.zeros((M, N), dtype=np.uint8)
    with capi.Shard(N, M) as sh:
        vp = codes.ctypes.data_as(capi.C.c_void_p)
        for bits in (0, 4, 12, 32):
            with pytest.raises(capi.GvError, match="bits must be 8 or 16"):
                sh._ck(sh.L.gv_upload_dosage(sh.h, vp, codes.size, bits, 1.0))
            with pytest.raises(capi.GvError, match="bits must be 8 or 16"):
                sh._ck(sh.L.gv_synth_dosage(sh.h, 1, bits))
            with pytest.raises(capi.GvError, match="bits must be 8 or 16"):
                sh._ck(sh.L.gv_upload_dosage_file(sh.h, b"/nonexistent", 0, bits, 1.0))
        for scale in (0.0, -1.0, float("inf"), float("nan")):
            with pytest.raises(capi.GvError, match="scale must be positive and finite"):
                sh.upload_dosage(codes, scale)
            with pytest.raises(capi.GvError, match="scale must be positive and finite"):
                sh.upload_dosage_file("/nonexistent", 8, scale)
        with pytest.raises(capi.GvError, match="uint8 or uint16"):
            sh.upload_dosage(codes.astype(np.int8), 1.0)
        with pytest.raises(capi.GvError, match="n != M"):
            sh._ck(sh.L.gv_upload_dosage(sh.h, vp, codes.size - 1, 8, 1.0))
        assert sh.get_layout() == 0


def test_every_kind_replaces_the_dataset_held_before():
    N, M = 1203, 450
    bed = synth.synth_bed(N, M, seed=3, miss_ppm=0)
    B8, B16, X = synth.synth_dosage(N, M, 5, 8), synth.synth_dosage(N, M, 6, 16), synth.synth_meth(N, M, 7)
    rng = np.random.default_rng(2)
    x = rng.standard_normal(M)

    def fresh(upload):
        with capi.Shard(N, M) as sh:
            upload(sh)
            sh.compute_markers_statistics()
            return sh.Ax(x)

    steps = [(lambda s: s.upload_bed(bed), (1, 2)), (lambda s: s.upload_dosage(B8, 1.0 / 127.0), (4,)),
             (lambda s: s.upload_meth(X), (3,)), (lambda s: s.upload_dosage(B16, 2.0 ** -14), (5,)),
             (lambda s: s.upload_dosage(B8, 1.0 / 127.0), (4,)), (lambda s: s.upload_bed(bed), (1, 2))]
    with capi.Shard(N, M) as sh:
        for upload, layouts in steps:
            upload(sh)
            assert sh.get_layout() in layouts
            sh.compute_markers_statistics()
            assert np.array_equal(sh.Ax(x), fresh(upload))


# ---- sharding -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
def test_forced_multi_reproduces_one_rank_bit_for_bit(bits):
    N, M = 2049, 1300
    B = synth.synth_dosage(N, M, 4, bits)
    rng = np.random.default_rng(4)
    x, x2 = rng.standard_normal(M), rng.standard_normal(M)
    outs = []
    for transport in (0, 1):
        with capi.Shard(N, M) as sh:
            if transport:
                sh._ck(sh.L.gv_debug_force_multi(sh.h, transport, 0))
            sh.upload_dosage(B, TEST_SCALE[bits])
            sh.compute_markers_statistics()
            dx, dx2, dz, dz2 = sh.vecM(x), sh.vecM(x2), sh.vecN(), sh.vecN()
            sh.ax2_dev(dx, dx2, dz, dz2)
            z = sh.Ax(x)
            d = sh.vecM()
            sh.lmmse_mult(dx, 1.3, 0.2, d)
            outs.append((z, dz.download(), dz2.download(), d.download(), sh.ATx(z)))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)


def test_two_shards_over_host_transport_match_one_shard():
    N, Mt, nshards, bits = 1100, 2500, 2, 8
    full = synth.synth_dosage(N, Mt, 23, bits)
    scale = TEST_SCALE[bits]
    rng = np.random.default_rng(nshards)
    x = rng.standard_normal(Mt)
    p = np.zeros(4 * ((N + 3) // 4))
    p[:N] = rng.standard_normal(N)
    with capi.Shard(N, Mt) as sh:
        sh.upload_dosage(full, scale)
        sh.compute_markers_statistics()
        z1, w1 = sh.Ax(x), sh.ATx(p)
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
                sh.upload_dosage(full[S:S + M], scale)
                sh.comm_init_local(7800 + nshards, nshards, rank)
                sh.compute_markers_statistics()
                z, w = sh.Ax(x[S:S + M]), sh.ATx(p)
                d = sh.vecM()
                sh.lmmse_mult(sh.vecM(x[S:S + M]), 1.3, 0.2, d)
                results[rank] = (z, w, d.download())
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


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 16])
def test_refused_entry_points_name_the_kind(bits):
    N, M = 300, 200
    with capi.Shard(N, M) as sh:
        sh.synth_dosage(1, bits)
        sh.compute_markers_statistics()
        L, h = sh.L, sh.h
        kind = r"compact dosage data \(%d-bit codes\)" % bits

        def refused(call):
            with pytest.raises(capi.GvError, match=kind) as ei:
                call()
            assert "methylation" not in str(ei.value)

        refused(sh.download_bed)
        refused(lambda: sh._ck(L.gv_people_stats(h, None, None, None)))
        st, sb = capi.CgStats(), capi.CgStats()
        v, mu = sh.vecN(np.ones(4 * sh.mbytes)), sh.vecN()
        refused(lambda: sh._ck(L.gv_cg_solve_aat(h, v.h, None, 1.0, 1.0, 10, mu.h, capi.C.byref(st), None)))
        vb, mub, at = sh.vecM(np.ones(M)), sh.vecM(), sh.vecM()
        refused(lambda: sh._ck(L.gv_cg_solve_aat2(h, v.h, None, vb.h, 1.0, 1.0, 10, mu.h, at.h, mub.h, capi.C.byref(st),
                                                  capi.C.byref(sb), None, None, None, None)))
        refused(lambda: sh._ck(L.gv_cg_solve_aat2w(h, v.h, None, vb.h, 1.0, 1.0, 10, mu.h, at.h, mub.h, capi.C.byref(st),
                                                   capi.C.byref(sb), None, None, None, None, None)))
        z1, y, x1 = sh.vecN(), sh.vecN(), sh.vecM()
        pv = np.zeros(M)
        chrom = np.ones(M, dtype=np.int32)
        cp = chrom.ctypes.data_as(capi.C.POINTER(capi.C.c_int))
        refused(lambda: sh._ck(L.gv_pvals_loo(h, z1.h, y.h, x1.h, capi._dp(pv))))
        refused(lambda: sh._ck(L.gv_pvals_loco(h, z1.h, y.h, x1.h, cp, capi._dp(pv))))
        refused(lambda: sh._ck(L.gv_pvals_loco_pred(h, z1.h, y.h, x1.h, cp, capi._dp(pv), capi._dp(np.zeros(4 * sh.mbytes)))))
        refused(lambda: sh._ck(L.gv_set_decomp(h, 0, capi.C.byref(capi.DecompInfo()))))
        refused(lambda: sh._ck(L.gv_set_cg_precond(h, 1, 128)))
        sh._ck(L.gv_set_cg_precond(h, 0, 128))                      # the scalar rule stays available
        # the kernel mode is ignored, as for the dense fp64 kind
        x = np.linspace(-1, 1, M)
        z = sh.Ax(x)
        for mode in (0, 2):
            sh.set_kernel_mode(mode)
            assert np.array_equal(sh.Ax(x), z)


# ---- driver -------------------------------------------------------------------------------------------------------------------------
def test_gvamp_main_real_on_a_dosage8_file_equals_the_host_api_run(tmp_path):
    N, Mt, it = 600, 1500, 3
    B = synth.synth_dosage(N, Mt, 41, 8)
    cfile, pfile = str(tmp_path / "codes.u8"), str(tmp_path / "y.phen")
    B.tofile(cfile)
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
    out = str(tmp_path / "out") + "/"
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
    base = [exe, "--run-mode", "infere", "--geno-format", "dosage8", "--bed-file", cfile, "--phen-files", pfile, "--N", str(N),
            "--Mt", str(Mt), "--out-dir", out, "--out-name", "d", "--iterations", str(it), "--probs", "0.9,0.1", "--vars", "0,0.01",
            "--rho", "0.5", "--CG-max-iter", "20", "--seed", "4"]
    res = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "8-bit codes" in res.stdout
    x_drv = np.fromfile(out + "d_it_%d.bin" % it)
    # data::read_phen: values * sqrt((n - 1) / sum (y - mean)^2), not centred
    y = raw * np.sqrt((N - 1) / np.sum((raw - raw.mean()) ** 2))
    with capi.Shard(N, Mt) as sh:
        sh.upload_dosage_file(cfile, 8, 1.0 / 127.0)
        r = hostapi.infere_linear(sh, y, [0.9, 0.1], [0.0, 0.01], iterations=it, CG_max_iter=20, rho=0.5, seed=4, gam1=1e-6,
                                  gamw=2.0, fuse_solves=4)
    print("driver vs host API rel %.3e" % rel(r.x1[it - 1], x_drv))
    assert rel(r.x1[it - 1], x_drv) < 1e-9
    assert np.all(np.isfinite(x_drv)) and np.any(x_drv != 0)
    # what the dense kinds refuse ends with their FATAL lines
    for extra, msg in ((["--cg-precond", "ld"], "--cg-precond ld is not available for compact dosage data"),
                       (["--use-XXT-denoiser", "1"], "--use-XXT-denoiser 1 is not available for compact dosage data")):
        res = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        assert res.returncode != 0 and "FATAL" in res.stdout and msg in res.stdout, res.stdout[-2000:]
