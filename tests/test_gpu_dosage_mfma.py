"""The fixed-point i8 MFMA route of 8-bit dosage codes (gv_set_dosage_route(ctx, 1); include/gvamp.h): accuracy
against the long-double restatement of the dosage kind (tests/test_gpu_dosage.py) and the contract bounds, what surrounds the
kernels, bit-identity across segment lengths / vector slots / the order of the individuals, the int32 bound, the fallbacks, and the
whole loop."""
import contextlib
import itertools
import os
import subprocess

import numpy as np
import pytest

import dosage_fixed_restatement as fx
import test_gpu_dosage as gd
from gvamp_amd import capi, hostapi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
SCALE = 1.0 / 127.0
ONE_STEP = 64           # GV_DOSAGE_MFMA_SEG: rounded down to the kernel's K-step, at least one step -- one step in either kernel


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def shard(N, M, seg=None, **env):
    """a context whose GV_DOSAGE_MFMA_SEG (read by gv_create, per context) is seg; the variable is cleared again at once"""
    with _env(GV_DOSAGE_MFMA_SEG=seg, **env):
        return capi.Shard(N, M)


def four_products(sh, x, x2, p, p2):
    dx, dx2, dz, dz2 = sh.vecM(x), sh.vecM(x2), sh.vecN(), sh.vecN()
    sh.ax2_dev(dx, dx2, dz, dz2)
    dp, dp2, dw, dw2 = sh.vecN(p), sh.vecN(p2), sh.vecM(), sh.vecM()
    sh.atx2_dev(dp, dp2, dw, dw2)
    return sh.Ax(x), sh.ATx(p), dz.download(), dz2.download(), dw.download(), dw2.download()


def lmmse_bound(D, msig, scale, N, M, x, z, tau):
    """tau (A^T dz + d_atx(z)): |dz_n| <= the Ax bound, |A_nm| = msig_m scale |b - mu'| / sqrt(N); d_atx: the ATx bound at p = z"""
    bz = fx.ax_bound(N, M, scale, msig, x)
    col = np.abs(D).sum(axis=1).astype(np.float64) * msig * scale / np.sqrt(N)
    return tau * (fx.atx_bound(N, scale, msig, z[:N]) + col * bz)


# ---- 1. accuracy ----------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (5, 3), (63, 17), (1003, 700), (4099, 3001), (257, 70001)]


@pytest.mark.parametrize("N,M,with_na", [(N, M, na) for (N, M), na in itertools.product(SHAPES, (False, True))])
def test_products_vs_long_double_restatement_and_contract(N, M, with_na):
    c = gd.restatement(8, N, M, with_na)
    nonas, x, x2, p, p2 = c["nonas"], c["x"], c["x2"], c["p"], c["p2"]
    _, rs = gd.ref_stats(c["mu"], c["q"], nonas, SCALE, 1.0)
    with capi.Shard(N, M) as sh:
        sh.set_dosage_route(1)
        assert sh.dosage_route() == (1, 0)                  # a request: nothing is resident yet
        sh.upload_dosage(c["B"], SCALE)
        if with_na:
            sh.set_mask(c["m4"], nonas)
        sh.compute_markers_statistics()
        assert sh.dosage_route() == (1, 1)
        msig = sh.marker_stats()[1]
        npad = 4 * sh.mbytes
        p, p2 = p[:npad], p2[:npad]
        z, w, z_a, z_b, w_a, w_b = four_products(sh, x, x2, p, p2)
        rz = gd.ref_ax(c["D"], rs, SCALE, x, npad)
        rw = gd.ref_atx(c["Dp"], rs, SCALE, N)
        ez, ew = np.abs(z.astype(LD) - rz), np.abs(w.astype(LD) - rw)
        bz, bw = fx.ax_bound(N, M, SCALE, msig, x), fx.atx_bound(N, SCALE, msig, p)
        print("Ax rel %.3e  worst error %.3e  bound %.3e" % (gd.rel(z, rz), float(ez.max()), bz))
        print("ATx rel %.3e  worst error / bound %.3e" % (gd.rel(w, rw), float(np.max(ew / np.maximum(bw, 1e-300)))))
        assert np.all(ez <= bz) and np.all(ew <= bw)
        assert gd.rel(z, rz) < 1e-13 and gd.rel(w, rw) < 1e-13
        assert np.all(z[N:] == 0.0)                                    # exact zeros at the pad slots
        if with_na and N > 3:
            assert np.all(z[3:N:7] != 0.0)                             # no phenotype mask in Ax
        # the two-vector forms: each slot bit-equal to the one-vector call, and as accurate
        assert np.array_equal(z_a, z) and np.array_equal(z_b, sh.Ax(x2))
        assert np.array_equal(w_a, w) and np.array_equal(w_b, sh.ATx(p2))
        rz2, rw2 = gd.ref_ax(c["D"], rs, SCALE, x2, npad), gd.ref_atx(c["D"] @ p2[:N].astype(LD), rs, SCALE, N)
        print("second slot: Ax rel %.3e  ATx rel %.3e" % (gd.rel(z_b, rz2), gd.rel(w_b, rw2)))
        assert gd.rel(z_b, rz2) < 1e-13 and gd.rel(w_b, rw2) < 1e-13
        assert np.all(np.abs(z_b.astype(LD) - rz2) <= fx.ax_bound(N, M, SCALE, msig, x2))
        assert np.all(np.abs(w_b.astype(LD) - rw2) <= fx.atx_bound(N, SCALE, msig, p2))
        # lmmse_mult: tau A^T A v + gam2 v
        tau, gam2 = 1.7, 0.35
        d = sh.vecM()
        sh.lmmse_mult(sh.vecM(x), tau, gam2, d)
        expect = LD(tau) * gd.ref_atx(c["D"] @ rz[:N], rs, SCALE, N) + LD(gam2) * x.astype(LD)
        el = np.abs(d.download().astype(LD) - expect)
        bl = lmmse_bound(c["D"], msig, SCALE, N, M, x, z, tau) + 4 * np.finfo(np.float64).eps * np.abs(expect).astype(np.float64)
        print("lmmse_mult rel %.3e  worst error / bound %.3e" % (gd.rel(d.download(), expect), float(np.max(el / np.maximum(bl, 1e-300)))))
        assert np.all(el <= bl) and gd.rel(d.download(), expect) < 1e-13


def test_adversarial_dynamic_range_meets_the_absolute_bound():
    """one entry 2^45 above the rest: ONE exponent per vector, so only the absolute bound applies (as for kernel mode 1)"""
    N, M = 1003, 700
    c = gd.restatement(8, N, M, False)
    _, rs = gd.ref_stats(c["mu"], c["q"], c["nonas"], SCALE, 1.0)
    x, p = c["x"].copy(), c["p"].copy()
    x[M // 3] *= 2.0 ** 45
    p[N // 3] *= 2.0 ** 45
    with capi.Shard(N, M) as sh:
        sh.set_dosage_route(1)
        sh.upload_dosage(c["B"], SCALE)
        sh.compute_markers_statistics()
        msig = sh.marker_stats()[1]
        npad = 4 * sh.mbytes
        z, w = sh.Ax(x), sh.ATx(p[:npad])
    ez = np.abs(z.astype(LD) - gd.ref_ax(c["D"], rs, SCALE, x, npad))
    ew = np.abs(w.astype(LD) - gd.ref_atx(c["D"] @ p[:N].astype(LD), rs, SCALE, N))
    bz, bw = fx.ax_bound(N, M, SCALE, msig, x), fx.atx_bound(N, SCALE, msig, p)
    print("Ax worst error / bound %.3e  ATx worst error / bound %.3e" % (float(ez.max()) / bz, float(np.max(ew / bw))))
    assert np.all(ez <= bz) and np.all(ew <= bw)


# ---- 2. what surrounds the kernels does not depend on the route ---------------------------------------------------------------------
def test_epilogue_and_multi_scale_path_agree_with_route_0():
    N, M = 2049, 1300
    B = synth.synth_dosage(N, M, 4, 8)
    rng = np.random.default_rng(4)
    x, x2 = rng.standard_normal(M), rng.standard_normal(M)
    tau, gam2 = 1.3, 0.2
    outs = {}
    for route, transport in itertools.product((0, 1), (0, 1)):
        with capi.Shard(N, M) as sh:
            if transport:
                sh._ck(sh.L.gv_debug_force_multi(sh.h, transport, 0))
            sh.set_dosage_route(route)
            sh.upload_dosage(B, SCALE)
            sh.compute_markers_statistics()
            assert sh.dosage_route() == (route, route)
            msig = sh.marker_stats()[1]
            dx, dx2, dz, dz2, d = sh.vecM(x), sh.vecM(x2), sh.vecN(), sh.vecN(), sh.vecM()
            sh.ax2_dev(dx, dx2, dz, dz2)
            z = sh.Ax(x)
            sh.lmmse_mult(dx, tau, gam2, d)
            outs[route, transport] = (z, dz.download(), dz2.download(), sh.ATx(z), d.download())
    for a, b in zip(outs[1, 0], outs[1, 1]):               # the multi-rank branch (1.0 inside, 1 / sqrt(N) after the exchange): the same bits
        assert np.array_equal(a, b)
    mu = fx.code_mean(B)
    D = B.astype(np.float64) - mu[:, None]
    z0 = outs[0, 0][0]
    bounds = (fx.ax_bound(N, M, SCALE, msig, x), fx.ax_bound(N, M, SCALE, msig, x), fx.ax_bound(N, M, SCALE, msig, x2),
              fx.atx_bound(N, SCALE, msig, z0[:N]), lmmse_bound(D, msig, SCALE, N, M, x, z0, tau))
    for transport in (0, 1):
        for k, (a, b, bd) in enumerate(zip(outs[0, transport], outs[1, transport], bounds)):
            diff = np.abs(a - b)
            print("transport %d product %d: worst |route 0 - route 1| / (2 bound) %.3e"
                  % (transport, k, float(np.max(diff / np.maximum(2 * bd, 1e-300)))))
            assert np.all(diff <= 2 * bd) and np.any(a != 0)


# ---- 3. bit-identity ------------------------------------------------------------------------------------------------------------
def test_segment_length_changes_no_bit():
    N, M = 4099, 3001
    c = gd.restatement(8, N, M, False)
    outs = []
    for seg in (ONE_STEP, None):
        with shard(N, M, seg) as sh:
            sh.set_dosage_route(1)
            sh.upload_dosage(c["B"], SCALE)
            sh.compute_markers_statistics()
            assert sh.dosage_route() == (1, 1)
            npad = 4 * sh.mbytes
            outs.append(four_products(sh, c["x"], c["x2"], c["p"][:npad], c["p2"][:npad]))
    for a, b in zip(*outs):
        assert np.array_equal(a, b) and np.any(a != 0)


def test_a_segment_beyond_the_int32_bound_is_refused():
    with _env(GV_DOSAGE_MFMA_SEG=fx.SEG_MAX + 1):
        with pytest.raises(capi.GvError, match="GV_DOSAGE_MFMA_SEG"):
            capi.Shard(64, 8)
    with shard(64, 8, fx.SEG_MAX) as sh:
        sh.set_dosage_route(1)


def test_the_order_of_the_individuals_changes_no_bit_of_atx():
    """mirror pairs b, 2c - b: the mean code of a row is the integer c and q a sum of integers, in any order; the products of route 1
    are integer sums, so a permutation of the individuals (the columns of the codes and p together) leaves ATx bit-identical"""
    N, M = 4098, 300
    rng = np.random.default_rng(12)
    cen = rng.integers(20, 236, M)
    half = np.minimum(cen, 255 - cen)
    b = (cen[:, None] + (rng.integers(-10 ** 6, 10 ** 6, (M, N // 2)) % (2 * half[:, None] + 1)) - half[:, None])
    B = np.empty((M, N), dtype=np.uint8)
    B[:, 0::2], B[:, 1::2] = b, 2 * cen[:, None] - b
    assert np.array_equal(B.astype(np.int64).sum(axis=1), cen * N) and np.all(B.min(axis=1) != B.max(axis=1))
    p = rng.standard_normal(N)
    perm = rng.permutation(N)
    outs = []
    for cols in (np.arange(N), perm):
        with capi.Shard(N, M) as sh:
            sh.set_dosage_route(1)
            sh.upload_dosage(np.ascontiguousarray(B[:, cols]), SCALE)
            sh.compute_markers_statistics()
            assert sh.dosage_route() == (1, 1)
            pp = np.zeros(4 * sh.mbytes)
            pp[:N] = p[cols]
            outs.append((sh.marker_stats(), sh.ATx(pp)))
    assert np.array_equal(outs[0][0][0], outs[1][0][0]) and np.array_equal(outs[0][0][1], outs[1][0][1])
    assert np.array_equal(outs[0][1], outs[1][1]) and np.any(outs[0][1] != 0)


# ---- 4. the int32 bound -----------------------------------------------------------------------------------------------------------
def test_atx_past_the_int32_bound_flushes_its_accumulators():
    """N = 140 000 individuals: one digit plane of p is -128 at every entry, a row of code 0 and a row of code 255 are in the matrix
    (tests/test_dosage_fixed_cpu.py asserts that their unsegmented sums leave int32)"""
    N, M, B, p = fx.bound_atx_case()
    mu, q, D = gd.ref_code_stats(B, np.ones(N), N)
    _, rs = gd.ref_stats(mu, q, N, SCALE, 1.0)
    rw = gd.ref_atx(D @ p.astype(LD), rs, SCALE, N)
    outs = []
    for seg in (None, ONE_STEP):
        with shard(N, M, seg) as sh:
            sh.set_dosage_route(1)
            sh.upload_dosage(B, SCALE)
            sh.compute_markers_statistics()
            assert sh.dosage_route() == (1, 1)
            mave, msig = sh.marker_stats()
            pp = np.zeros(4 * sh.mbytes)
            pp[:N] = p
            outs.append(sh.ATx(pp))
    w = outs[0]
    ew, bw = np.abs(w.astype(LD) - rw), fx.atx_bound(N, SCALE, msig, p)
    print("ATx rel %.3e  worst error / bound %.3e  rows of code 0 / 255 (exact value 0): %r %r"
          % (gd.rel(w, rw), float(np.max(ew / bw)), w[3], w[5]))
    assert np.all(ew <= bw) and gd.rel(w, rw) < 1e-13
    assert np.array_equal(outs[0], outs[1])
    # and bit for bit what the integer restatement (unsegmented, exact) gives
    assert np.array_equal(mave, SCALE * fx.code_mean(B))
    assert np.array_equal(w, fx.atx(B, fx.code_mean(B), msig, SCALE, p))


def test_ax_past_the_int32_bound_flushes_its_accumulators():
    """M = 140 000 markers, most of them constant at code 0: one digit plane of the weights c = msig scale x is -128 at every marker"""
    N, M, B, c = fx.bound_ax_case()
    ordinary, _ = fx.bound_ax_rows(M)
    mu, q, D = gd.ref_code_stats(B, np.ones(N), N)
    _, rs = gd.ref_stats(mu, q, N, SCALE, 1.0)
    outs = []
    for seg in (None, ONE_STEP):
        with shard(N, M, seg) as sh:
            sh.set_dosage_route(1)
            sh.upload_dosage(B, SCALE)
            sh.compute_markers_statistics()
            assert sh.dosage_route() == (1, 1)
            mave, msig = sh.marker_stats()
            assert np.all(msig[~ordinary] == 1.0)
            x = c / (msig * SCALE)
            outs.append(sh.Ax(x))
            npad = 4 * sh.mbytes
    cd = msig * SCALE * x                                   # the weights as the device forms them
    d = fx.digits(fx.quantise(cd, fx.exponent(cd)))
    assert fx.exponent(cd) == 0 and np.all(d[fx.BOUND_PLANE] == -128)
    assert ((B.astype(np.int64) - 128).T @ d[fx.BOUND_PLANE]).min() > fx.INT32_MAX
    z = outs[0]
    rz = gd.ref_ax(D, rs, SCALE, x, npad)
    ez, bz = np.abs(z.astype(LD) - rz), fx.ax_bound(N, M, SCALE, msig, x)
    print("Ax rel %.3e  worst error %.3e  bound %.3e" % (gd.rel(z, rz), float(ez.max()), bz))
    assert np.all(ez <= bz) and gd.rel(z, rz) < 1e-13 and np.all(z[N:] == 0.0)
    assert np.array_equal(outs[0], outs[1])
    # and bit for bit what the integer restatement (unsegmented, exact) gives
    assert np.array_equal(mave, SCALE * fx.code_mean(B))
    assert np.array_equal(z[:N], fx.ax(B, fx.code_mean(B), msig, SCALE, x))


# ---- 5. fallbacks -----------------------------------------------------------------------------------------------------------------
def _products(sh, x, p):
    d = sh.vecM()
    sh.lmmse_mult(sh.vecM(x), 1.3, 0.2, d)
    return sh.Ax(x), sh.ATx(p), d.download()


@pytest.mark.parametrize("case", ["16-bit codes", "reserved codes", "GV_DOSAGE_NA_KERNELS=1"])
def test_where_the_route_does_not_apply_nothing_changes_by_a_bit(case):
    N, M = 1003, 700
    rng = np.random.default_rng(3)
    x = rng.standard_normal(M)
    env = {}
    if case == "16-bit codes":
        B, scale, missing = synth.synth_dosage(N, M, 5, 16), 2.0 ** -14, False
    elif case == "reserved codes":
        B, scale, missing = synth.synth_dosage_na(N, M, 5, 8, 20000), SCALE, True
        assert np.any(B == 255)
    else:
        B, scale, missing = synth.synth_dosage_na(N, M, 5, 8, 0), SCALE, True
        env = dict(GV_DOSAGE_NA_KERNELS=1)
    with shard(N, M, None, **env) as sh:
        sh.upload_dosage(B, scale, missing=missing)
        sh.compute_markers_statistics()
        p = np.zeros(4 * sh.mbytes)
        p[:N] = rng.standard_normal(N)
        assert sh.dosage_route() == (0, 0)
        before = _products(sh, x, p)
        sh.set_dosage_route(1)
        assert sh.dosage_route() == (1, 0)
        if case != "16-bit codes":
            assert sh.dosage_info()["na_kernels"]
        for a, b in zip(before, _products(sh, x, p)):
            assert np.array_equal(a, b) and np.any(a != 0)


def test_other_routes_are_refused_and_bed_data_ignore_the_setting():
    N, M = 1003, 700
    bed = synth.synth_bed(N, M, seed=3, miss_ppm=10000)
    rng = np.random.default_rng(5)
    x = rng.standard_normal(M)
    with capi.Shard(N, M) as sh:
        for route in (2, -1, 7):
            with pytest.raises(capi.GvError, match="gv_set_dosage_route"):
                sh.set_dosage_route(route)
        assert sh.dosage_route() == (0, 0)
        sh.upload_bed(bed)
        sh.compute_markers_statistics()
        p = np.zeros(4 * sh.mbytes)
        p[:N] = rng.standard_normal(N)
        before = _products(sh, x, p)
        sh.set_dosage_route(1)
        assert sh.dosage_route() == (1, 0)
        for a, b in zip(before, _products(sh, x, p)):
            assert np.array_equal(a, b) and np.any(a != 0)
        # the request outlives the dataset: 8-bit codes uploaded next run on it, and route 0 brings the VALU kernels back
        B = synth.synth_dosage(N, M, 9, 8)
        sh.upload_dosage(B, SCALE)
        sh.compute_markers_statistics()
        assert sh.dosage_route() == (1, 1)
        z1 = sh.Ax(x)
        sh.set_dosage_route(0)
        assert sh.dosage_route() == (0, 0)
        z0 = sh.Ax(x)
    with capi.Shard(N, M) as sh:
        sh.upload_dosage(B, SCALE)
        sh.compute_markers_statistics()
        assert np.array_equal(sh.Ax(x), z0)
    assert gd.rel(z1, z0) < 1e-13


# ---- 6. the whole loop ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [0, 4])
def test_vamp_on_codes_of_a_bed_under_route_1_matches_the_bed_run(oracle, fuse):
    N, M, G, y, ref, rb = gd._bed_runs(fuse)
    with capi.Shard(N, M) as sd:
        sd.set_dosage_route(1)
        sd.upload_dosage(gd.bed_as_codes(G, 8), gd.DYADIC[8])
        rd = hostapi.infere_linear(sd, y, gd.PROBS, gd.VARS, fuse_solves=fuse, **gd._VAMP_KW)
        assert sd.dosage_route() == (1, 1)
    assert rd.niter == rb.niter
    print("x_hat rel to bed run %.3e" % gd.rel(rd.x_est, rb.x_est))
    assert gd.rel(rd.x_est, rb.x_est) < 1e-9
    for it in range(rd.niter):
        t, b = rd.trace[it], rb.trace[it]
        assert (t["cg_iters"], t["onsager_iters"]) == (b["cg_iters"], b["onsager_iters"])
        if fuse == 4:
            assert t["n_ax_pass"] < t["n_ax"]              # the two-vector pass over the codes is in use


def test_gvamp_main_real_with_dosage_kernels_mfma_equals_the_host_api_run(tmp_path):
    N, Mt, it = 600, 1500, 3
    B = synth.synth_dosage(N, Mt, 41, 8)
    cfile, pfile = str(tmp_path / "codes.u8"), str(tmp_path / "y.phen")
    B.tofile(cfile)
    rng = np.random.default_rng(6)
    beta = rng.standard_normal(Mt) * (rng.random(Mt) < 0.05) * 0.15
    with capi.Shard(N, Mt) as sh:
        sh.upload_dosage(B, SCALE)
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
    res = subprocess.run(base + ["--dosage-kernels", "mfma"], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    assert "dosage kernels: fixed-point i8 MFMA route" in res.stdout
    x_drv = np.fromfile(out + "d_it_%d.bin" % it)
    y = raw * np.sqrt((N - 1) / np.sum((raw - raw.mean()) ** 2))
    with capi.Shard(N, Mt) as sh:
        sh.upload_dosage_file(cfile, 8, SCALE)
        r = hostapi.infere_linear(sh, y, [0.9, 0.1], [0.0, 0.01], iterations=it, CG_max_iter=20, rho=0.5, seed=4, gam1=1e-6,
                                  gamw=2.0, fuse_solves=4)
    print("driver on route 1 vs host API rel %.3e" % gd.rel(r.x1[it - 1], x_drv))
    assert gd.rel(r.x1[it - 1], x_drv) < 1e-9
    assert np.all(np.isfinite(x_drv)) and np.any(x_drv != 0)
    res = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "dosage kernels: fp64 VALU kernels" in res.stdout
