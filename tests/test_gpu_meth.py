"""Methylation data (type_data == "meth"): the dense fp64 design matrix of gv_dense.hip behind the same C ABI as bed data.

The reference's meth branches are restated in numpy below (data.cpp line numbers cited), and the dense path is tied to the
oracle through bed data: a bed without missing genotypes, decoded to doubles, is the same design matrix."""
import os
import subprocess
import threading

import numpy as np
import pytest

from gvamp_amd import capi, hostapi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBS, VARS = [0.90, 0.07, 0.03], [0, 0.001, 0.01]


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


# ---- numpy restatements of the reference's meth branches ---------------------------------------------------------------------
def ref_stats(X, na, nonas, alpha):
    """compute_markers_statistics, meth branch (data.cpp:487-540): two passes, na_lut factor, alpha_scale power"""
    mave = (X * na).sum(axis=1) / nonas
    d = (X - mave[:, None]) * na
    ss = (d * d).sum(axis=1)
    sd = np.sqrt(np.where(ss != 0, ss, 1.0) / max(nonas - 1.0, 1.0))
    msig = np.where(ss != 0, 1.0 / (sd if alpha == 1.0 else sd ** alpha), 1.0)
    return mave, msig


def ref_atx(X, mave, msig, p):
    """dot_product (data.cpp:783-797) over all N individuals, then ATx's 1/sqrt(N) (:814-835)"""
    N = X.shape[1]
    return msig * ((X - mave[:, None]) @ p[:N]) / np.sqrt(N)


def ref_ax(X, mave, msig, v, npad):
    """data::Ax, meth branch (data.cpp:1013-1045): no phenotype mask, Ax_total[i] /= sqrt(N)"""
    N = X.shape[1]
    out = np.zeros(npad)
    out[:N] = ((X - mave[:, None]).T @ (msig * v)) / np.sqrt(N)
    return out


def na_mask(N, with_na):
    """(mask4 nibbles, na[N], nonas): every 7th individual from 3 on has no phenotype"""
    na = np.ones(N)
    if with_na:
        na[3::7] = 0.0
    mb = (N + 3) // 4
    m4 = np.zeros(mb, dtype=np.uint8)
    for n in range(N):
        if na[n]:
            m4[n >> 2] |= 1 << (n & 3)
    return m4, na, int(na.sum())


def meth_matrix(N, M, seed):
    """methylation-like values: large per-marker means, small spread; marker 0 constant (msig = 1) when M >= 3"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0.2, 0.8, size=(M, 1)) + 0.03 * rng.standard_normal((M, N))
    if M >= 3:
        X[0] = 0.5
    return X


def decode_bed(bed, N, M):
    """PLINK 2-bit rows -> doubles: 00 -> 2, 10 -> 1, 11 -> 0 (no missing codes expected)"""
    mb = (N + 3) // 4
    b = np.asarray(bed, dtype=np.uint8).reshape(M, mb)
    codes = np.stack([(b >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(M, 4 * mb)[:, :N]
    assert not np.any(codes == 1)
    return np.choose(codes, [2.0, -1.0, 1.0, 0.0])


SHAPES = [(1, 1), (5, 3), (1003, 700), (4099, 3001), (257, 70001)]


@pytest.mark.parametrize("N,M", SHAPES)
@pytest.mark.parametrize("with_na", [False, True])
@pytest.mark.parametrize("alpha", [1.0, 0.3])
def test_products_vs_reference_restatement(N, M, with_na, alpha):
    X = meth_matrix(N, M, N * 7 + M)
    m4, na, nonas = na_mask(N, with_na)
    rng = np.random.default_rng(N + M)
    with capi.Shard(N, M) as sh:
        sh.upload_meth(X)
        assert sh.get_layout() == 3
        if with_na:
            sh.set_mask(m4, nonas)
        sh.compute_markers_statistics(alpha)
        mave, msig = sh.marker_stats()
        rm, rs = ref_stats(X, na, nonas, alpha)
        assert np.allclose(mave, rm, rtol=1e-13, atol=0) and np.allclose(msig, rs, rtol=1e-13, atol=0)
        if M >= 3:
            assert msig[0] == 1.0
        npad = 4 * sh.mbytes
        x, x2 = rng.standard_normal(M), rng.standard_normal(M)
        p, p2 = np.zeros(npad), np.zeros(npad)
        p[:N], p2[:N] = rng.standard_normal(N), rng.standard_normal(N)
        z = sh.Ax(x)
        w = sh.ATx(p)
        assert rel(z, ref_ax(X, rm, rs, x, npad)) < 1e-13
        assert rel(w, ref_atx(X, rm, rs, p)) < 1e-13
        assert np.all(z[N:] == 0.0)                                    # exact zeros at the pad slots
        if with_na and N > 3:
            assert np.all(z[3:N:7] != 0.0)                             # unmasked at NA individuals, as the reference's meth Ax
        assert np.array_equal(sh.Ax(x), z) and np.array_equal(sh.ATx(p), w)     # bit-reproducible
        # two-vector forms: each slot bit-equal to the one-vector call on that vector
        dx, dx2, dz, dz2 = sh.vecM(x), sh.vecM(x2), sh.vecN(), sh.vecN()
        sh.ax2_dev(dx, dx2, dz, dz2)
        assert np.array_equal(dz.download(), z) and np.array_equal(dz2.download(), sh.Ax(x2))
        dp, dp2, dw, dw2 = sh.vecN(p), sh.vecN(p2), sh.vecM(), sh.vecM()
        sh.atx2_dev(dp, dp2, dw, dw2)
        assert np.array_equal(dw.download(), w) and np.array_equal(dw2.download(), sh.ATx(p2))
        # lmmse_mult: tau A^T A v + gam2 v (vamp.cpp:1074-1118)
        tau, gam2 = 1.7, 0.35
        d = sh.vecM()
        sh.lmmse_mult(dx, tau, gam2, d)
        A_x = ref_ax(X, rm, rs, x, npad)
        expect = tau * ref_atx(X, rm, rs, A_x) + gam2 * x
        assert rel(d.download(), expect) < 1e-13


def test_ingest_paths_and_dataset_replacement(tmp_path):
    """upload_meth_file at S*N*8, upload_meth of the same slice and synth_meth against synth.synth_meth: identical products"""
    N, Mt, S, M, seed = 1203, 900, 317, 450, 99
    full = synth.synth_meth(N, Mt, seed)
    path = str(tmp_path / "m.bin")
    full.tofile(path)
    rng = np.random.default_rng(1)
    x = rng.standard_normal(M)
    p = np.zeros(4 * ((N + 3) // 4))
    p[:N] = rng.standard_normal(N)
    outs = []
    for how in ("file", "array", "synth"):
        with capi.Shard(N, M, Mt=Mt, S=S) as sh:
            if how == "file":
                sh.upload_meth_file(path)                 # default offset S * N * 8 (data.cpp:259)
            elif how == "array":
                sh.upload_meth(full[S:S + M])
            else:
                sh.synth_meth(seed)
            sh.compute_markers_statistics()
            outs.append(sh.marker_stats() + (sh.Ax(x), sh.ATx(p)))
    for o in outs[1:]:
        for a, b in zip(o, outs[0]):
            assert np.array_equal(a, b)
    mave, msig = ref_stats(full[S:S + M], np.ones(N), N, 1.0)
    assert np.allclose(outs[0][0], mave, rtol=1e-13) and np.allclose(outs[0][1], msig, rtol=1e-13)
    # either kind replaces the other
    bed = synth.synth_bed(N, M, seed=3, miss_ppm=0)
    with capi.Shard(N, M) as sh:
        sh.upload_bed(bed)
        assert sh.get_layout() in (1, 2)
        sh.upload_meth(full[:M])
        assert sh.get_layout() == 3
        sh.compute_markers_statistics()
        z_meth = sh.Ax(x)
        sh.upload_bed(bed)
        assert sh.get_layout() in (1, 2)
        sh.compute_markers_statistics()
        z_bed = sh.Ax(x)
        sh.synth_meth(seed)
        sh.compute_markers_statistics()
        assert np.array_equal(sh.Ax(x), z_meth)
    with capi.Shard(N, M) as sh:
        sh.upload_bed(bed)
        sh.compute_markers_statistics()
        assert np.array_equal(sh.Ax(x), z_bed)
    with capi.Shard(N, M) as sh:
        with pytest.raises(capi.GvError, match="short file"):
            sh.upload_meth_file(path, offset=(Mt - M + 1) * N * 8)


def _bed_case(N, M, seed):
    bed = synth.synth_bed(N, M, seed=seed, miss_ppm=0)
    return bed, decode_bed(bed, N, M)


def test_dense_copy_of_a_bed_matches_the_bed_products():
    N, M = 1501, 2200
    bed, X = _bed_case(N, M, 5)
    rng = np.random.default_rng(2)
    x = rng.standard_normal(M)
    p = np.zeros(4 * ((N + 3) // 4))
    p[:N] = rng.standard_normal(N)
    with capi.Shard(N, M) as sb, capi.Shard(N, M) as sm:
        sb.upload_bed(bed)
        sm.upload_meth(X)
        for alpha in (1.0, 0.3):
            sb.compute_markers_statistics(alpha)
            sm.compute_markers_statistics(alpha)
            (bm, bs), (mm, ms) = sb.marker_stats(), sm.marker_stats()
            assert np.allclose(mm, bm, rtol=1e-14, atol=1e-15) and np.allclose(ms, bs, rtol=1e-14)
            assert rel(sm.Ax(x), sb.Ax(x)) < 1e-12 and rel(sm.ATx(p), sb.ATx(p)) < 1e-12


@pytest.mark.parametrize("fuse", [0, 1, 4])
def test_vamp_on_dense_copy_matches_bed_run_and_oracle(oracle, fuse):
    N, M = 1200, 3000
    bed, X = _bed_case(N, M, 17)
    beta, y = oracle.sim_phen(bed, N, M, 0.5, 300, 7, nthreads=4)
    kw = dict(iterations=4, CG_max_iter=30, rho=0.5, seed=7, gam1=1e-8, gamw=2.0)
    ref = oracle.infere(bed, N, M, y, PROBS, VARS, **kw)
    with capi.Shard(N, M, anchor=True) as sb:
        sb.upload_bed(bed)
        rb = hostapi.infere_linear(sb, y, PROBS, VARS, fuse_solves=fuse, **kw)
    with capi.Shard(N, M) as sm:
        sm.upload_meth(X)
        rm = hostapi.infere_linear(sm, y, PROBS, VARS, fuse_solves=fuse, **kw)
    assert rm.niter == rb.niter == ref.niter
    assert rel(rm.x_est, rb.x_est) < 1e-9 and rel(rm.x_est, ref.x_est) < 1e-9
    for it in range(rm.niter):
        t, b, o = rm.trace[it], rb.trace[it], ref.trace[it]
        assert (t["cg_iters"], t["onsager_iters"]) == (b["cg_iters"], b["onsager_iters"]) == (o["cg_iters"], o["onsager_iters"])
        if fuse == 4:
            assert t["n_ax_pass"] < t["n_ax"]          # the two-vector dense pass is in use


def test_probit_on_dense_copy_matches_bed_run(oracle):
    N, M = 1001, 1500
    bed, X = _bed_case(N, M, 11)
    beta, yl = oracle.sim_phen(bed, N, M, 0.6, 100, 11)
    y = (yl > np.median(yl)).astype(np.float64)
    kw = dict(iterations=5, CG_max_iter=30, rho=0.5, seed=3, gam1=1e-8, gamw=1.0, model="bin_class")
    with capi.Shard(N, M, anchor=True) as sb:
        sb.upload_bed(bed)
        rb = hostapi.infere_linear(sb, y, PROBS, VARS, **kw)
    with capi.Shard(N, M) as sm:
        sm.upload_meth(X)
        rm = hostapi.infere_linear(sm, y, PROBS, VARS, **kw)
    assert rm.niter == rb.niter
    assert rel(rm.x_est, rb.x_est) < 1e-9


def test_forced_multi_reproduces_one_rank_bit_for_bit():
    N, M = 2049, 1300
    X = synth.synth_meth(N, M, 4)
    rng = np.random.default_rng(4)
    x, x2 = rng.standard_normal(M), rng.standard_normal(M)
    outs = []
    for transport in (0, 1):
        with capi.Shard(N, M) as sh:
            if transport:
                sh._ck(sh.L.gv_debug_force_multi(sh.h, transport, 0))
            sh.upload_meth(X)
            sh.compute_markers_statistics()
            dx, dx2, dz, dz2 = sh.vecM(x), sh.vecM(x2), sh.vecN(), sh.vecN()
            sh.ax2_dev(dx, dx2, dz, dz2)
            z = sh.Ax(x)
            d = sh.vecM()
            sh.lmmse_mult(dx, 1.3, 0.2, d)
            outs.append((z, dz.download(), dz2.download(), d.download(), sh.ATx(z)))
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("nshards", [2, 3])
def test_sharded_over_host_transport_matches_one_shard(oracle, nshards):
    """nshards contexts on this GPU joined by the in-process host transport: every product equals the one-shard product to 1e-12;
    x_hat equals the oracle's nshards-shard run on the bed whose dense copy this is (the Hutchinson probe is seeded seed + S per
    shard, as the reference seeds it, so a k-shard run is held against a k-shard reference, not against one shard)."""
    N, Mt = 1100, 2500
    bed, full = _bed_case(N, Mt, 23)
    rng = np.random.default_rng(nshards)
    x = rng.standard_normal(Mt)
    p = np.zeros(4 * ((N + 3) // 4))
    p[:N] = rng.standard_normal(N)
    beta, y = oracle.sim_phen(bed, N, Mt, 0.5, 200, 7, nthreads=4)
    kw = dict(iterations=3, CG_max_iter=30, rho=0.5, seed=7, gam1=1e-8, gamw=2.0)
    with capi.Shard(N, Mt) as sh:
        sh.upload_meth(full)
        sh.compute_markers_statistics()
        z1, w1 = sh.Ax(x), sh.ATx(p)
    ref = oracle.infere(bed, N, Mt, y, PROBS, VARS, nshards=nshards, **kw)
    results, errors = [None] * nshards, []
    size, modu = divmod(Mt, nshards)

    def work(rank):
        try:
            M = size + 1 if rank < modu else size
            S = sum(size + 1 if r < modu else size for r in range(rank))
            with capi.Shard(N, M, Mt=Mt, S=S) as sh:
                sh.upload_meth(full[S:S + M])
                sh.comm_init_local(7700 + nshards, nshards, rank)
                sh.compute_markers_statistics()
                z, w = sh.Ax(x[S:S + M]), sh.ATx(p)
                r = hostapi.infere_linear(sh, y, PROBS, VARS, rank=rank, **kw)
                results[rank] = (z, w, r.x_est, r.trace)
        except Exception as e:   # noqa: BLE001
            errors.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(nshards)]
    for t in th:
        t.start()
    for t in th:
        t.join(timeout=600)
    assert not errors, errors
    for res in results:
        assert rel(res[0], z1) < 1e-12
    assert rel(np.concatenate([res[1] for res in results]), w1) < 1e-12
    assert rel(np.concatenate([res[2] for res in results]), ref.x_est) < 1e-9
    for it in range(len(ref.trace)):
        assert results[0][3][it]["cg_iters"] == ref.trace[it]["cg_iters"]


def test_refused_entry_points_name_the_reason():
    N, M = 300, 200
    with capi.Shard(N, M) as sh:
        sh.synth_meth(1)
        sh.compute_markers_statistics()
        L, h = sh.L, sh.h
        with pytest.raises(capi.GvError, match="methylation"):
            sh.download_bed()
        with pytest.raises(capi.GvError, match="methylation"):
            sh._ck(L.gv_people_stats(h, None, None, None))
        st = capi.CgStats()
        v, mu = sh.vecN(np.ones(4 * sh.mbytes)), sh.vecN()
        with pytest.raises(capi.GvError, match="methylation"):
            sh._ck(L.gv_cg_solve_aat(h, v.h, None, 1.0, 1.0, 10, mu.h, capi.C.byref(st), None))
        vb, mub, at = sh.vecM(np.ones(M)), sh.vecM(), sh.vecM()
        sb = capi.CgStats()
        with pytest.raises(capi.GvError, match="methylation"):
            sh._ck(L.gv_cg_solve_aat2(h, v.h, None, vb.h, 1.0, 1.0, 10, mu.h, at.h, mub.h, capi.C.byref(st), capi.C.byref(sb),
                                      None, None, None, None))
        z1, y, x1 = sh.vecN(), sh.vecN(), sh.vecM()
        pv = np.zeros(M)
        with pytest.raises(capi.GvError, match="methylation"):
            sh._ck(L.gv_pvals_loo(h, z1.h, y.h, x1.h, capi._dp(pv)))
        chrom = np.ones(M, dtype=np.int32)
        with pytest.raises(capi.GvError, match="methylation"):
            sh._ck(L.gv_pvals_loco(h, z1.h, y.h, x1.h, chrom.ctypes.data_as(capi.C.POINTER(capi.C.c_int)), capi._dp(pv)))
        with pytest.raises(capi.GvError, match="methylation"):
            sh._ck(L.gv_set_decomp(h, 0, capi.C.byref(capi.DecompInfo())))
        # the kernel mode is ignored for dense data
        x = np.linspace(-1, 1, M)
        z = sh.Ax(x)
        for mode in (0, 2):
            sh.set_kernel_mode(mode)
            assert np.array_equal(sh.Ax(x), z)


def test_at_scale_20k_by_800k():
    """128 GB of fp64 on one device, generated there: the adjoint identity, sampled ATx rows against the host reproducer, and a
    short VAMP run."""
    N, M, seed = 20000, 800000, 2026
    rng = np.random.default_rng(0)
    with capi.Shard(N, M) as sh:
        sh.synth_meth(seed)
        sh.compute_markers_statistics()
        mave, msig = sh.marker_stats()
        x = rng.standard_normal(M)
        p = np.zeros(4 * sh.mbytes)
        p[:N] = rng.standard_normal(N)
        z, w = sh.Ax(x), sh.ATx(p)
        assert np.all(z[N:] == 0.0)
        lhs, rhs = float(np.dot(z, p)), float(np.dot(x, w))
        assert abs(lhs - rhs) <= 1e-12 * np.linalg.norm(z) * np.linalg.norm(p)
        for m in np.sort(rng.choice(M, 64, replace=False)):
            row = synth.synth_meth(N, 1, seed, S=int(m))
            rm, rs = ref_stats(row, np.ones(N), N, 1.0)
            assert np.isclose(mave[m], rm[0], rtol=1e-13) and np.isclose(msig[m], rs[0], rtol=1e-13)
            assert np.isclose(w[m], ref_atx(row, rm, rs, p)[0], rtol=1e-13, atol=1e-13 * np.abs(w).max())
        beta = np.zeros(M)
        idx = rng.choice(M, 400, replace=False)
        beta[idx] = rng.standard_normal(400) * 0.05
        y = sh.Ax(beta * np.sqrt(N))[:N] + rng.standard_normal(N)
        r = hostapi.infere_linear(sh, y, PROBS, VARS, iterations=3, CG_max_iter=20, rho=0.5, seed=1, gam1=1e-8, gamw=1.0,
                                  history=False, fuse_solves=4)
        assert r.niter >= 1 and np.all(np.isfinite(r.x_est))


def test_gvamp_sim_meth_driver_end_to_end(tmp_path):
    """main_meth_ex.cpp restated: matrix written at S*N*8 and read back as "meth", VAMP, the usual output files; x_hat equal to a
    hostapi run on the same file and phenotype."""
    N, Mt, it = 600, 1500, 3
    mfile = str(tmp_path / "meth.bin")
    out = str(tmp_path / "out") + "/"
    cmd = [os.path.join(ROOT, "gvamp_amd", "gvamp_sim_meth"), "--bed-file", mfile, "--N", str(N), "--Mt", str(Mt),
           "--out-dir", out, "--out-name", "meth", "--iterations", str(it), "--num-mix-comp", "2", "--probs", "0.9,0.1",
           "--vars", "0,0.01", "--rho", "0.5", "--CG-max-iter", "20", "--seed", "7", "--store-pvals", "1"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "p-values: skipped for methylation data" in res.stdout
    assert os.path.getsize(mfile) == N * Mt * 8
    for f in ("meth_beta_true.bin", "meth_y.txt", "meth_y.bin", "meth_gam1s.csv", "meth_gam2s.csv", "meth_it_%d.bin" % it):
        assert os.path.exists(out + f), f
    assert not os.path.exists(out + "meth_pvals.bin")
    x_drv = np.fromfile(out + "meth_it_%d.bin" % it)
    y = np.fromfile(out + "meth_y.bin")
    gamw = 2.0 / Mt / (1e-3 * 0.02)                   # noise_prec_calc(SNR 2, {0, 1e-3}, {0.98, 0.02})
    with capi.Shard(N, Mt) as sh:
        sh.upload_meth_file(mfile)
        r = hostapi.infere_linear(sh, y, [0.9, 0.1], [0.0, 0.01], iterations=it, CG_max_iter=20, rho=0.5, seed=7, gam1=1e-6,
                                  gamw=0.9 * gamw, fuse_solves=4)
    assert rel(r.x1[it - 1], x_drv) < 1e-12
    assert np.all(np.isfinite(x_drv)) and np.any(x_drv != 0)
