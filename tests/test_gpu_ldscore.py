"""LD scores and banded LD correlations on the GPU (gv_ld_scores / gv_ld_band) against the numpy restatement
of tests/ld_restatement.py: both layouts and both MFMA kernel modes, bit-identity across them and across calls, symmetry,
chromosomes, hand-placed markers, the driver's run mode, the refusals, and the rest of the context left as it was.

Tolerances: the project's Gram bar (section 13's tests hold a Gram to 1e-12 x its largest diagonal; here the diagonal is 1):
|r - ref| <= 1e-12, l2 to 1e-12 relative, npairs and the NaN positions exact."""
import os
import subprocess

import numpy as np
import pytest

from gvamp_amd import capi, synth
import ld_restatement as ldr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = ((1, 1), (2, 1), (1, 2), (2, 2))          # (resident layout: 1 two stripe sets, 2 the tile layout; kernel mode)


def _mask4(na):
    N = na.size
    m = np.zeros((N + 3) // 4, dtype=np.uint8)
    for n in np.nonzero(na)[0]:
        m[n >> 2] |= 1 << (n & 3)
    return m


def _shard(bed, N, M, S=0, layout=2, mode=1, na=None, stats=True):
    sh = capi.Shard(N, M, Mt=S + M + 100, S=S, device=0)
    sh.set_layout(False, layout)
    sh.set_kernel_mode(mode)
    sh.upload_bed(bed)
    if na is not None:
        sh.set_mask(_mask4(na), int(na.sum()))
    if stats:
        sh.compute_markers_statistics()
    return sh


def _check(sh, ref, B, M, na_count, chrom=None, tag=None):
    """band over all rows, scores raw and adjusted against the restatement; returns what must be bit-identical elsewhere"""
    r, poly = ref["r"], ref["poly"]
    band = sh.ld_band(B, 0, M, chrom=chrom)
    want = ldr.band(r, B, 0, M, chrom)
    assert band.shape == want.shape
    print("max |r - ref| = %.3e" % np.max(np.abs(band - want)), tag)
    assert np.max(np.abs(band - want)) <= 1e-12, tag
    assert np.all(band[ldr.band(np.ones((M, M)), B, 0, M, chrom) == 0] == 0), tag          # exact zeros outside the band
    out = [band]
    for adjusted in (False, True):
        l2, n = sh.ld_scores(B, chrom=chrom, adjusted=adjusted)
        rl2, rn = ldr.scores(r, poly, B, chrom, adjusted, float(na_count))
        assert np.array_equal(np.isnan(l2), np.isnan(rl2)) and np.array_equal(np.isnan(l2), ~poly), tag
        assert np.array_equal(n, rn), tag
        ok = ~np.isnan(rl2)
        if ok.any():
            print("max rel l2 = %.3e" % np.max(np.abs(l2[ok] - rl2[ok]) / np.abs(rl2[ok])), tag, adjusted)
            assert np.max(np.abs(l2[ok] - rl2[ok]) / np.abs(rl2[ok])) <= 1e-12, (tag, adjusted)
        out += [l2, n]
    return out


SHAPES = [(1003, 0, 700, 100, False), (1203, 37, 333, 64, True), (998, 5, 200, 1, False), (5, 0, 3, 2, False),
          (2001, 37, 650, 200, False), (1203, 37, 333, 1000, True)]


@pytest.mark.parametrize("N,S,M,B,masked", SHAPES)
def test_band_and_scores_match_restatement_on_both_layouts_and_modes(N, S, M, B, masked):
    bed = synth.synth_bed(N, M, seed=3, miss_ppm=20000, S=S, ld_block=48, ld_ppm=900000)
    na = None
    if masked:
        na = np.ones(N)
        na[::7] = 0.0
    ref = ldr.ld(bed, N, M, B, na=na)
    if (N, M) == (5, 3):
        assert int(ref["poly"].sum()) == 1            # two monomorphic markers among three
    else:
        assert 15 < np.nanmean(ldr.ld(bed, N, M, 48, na=na)["l2"]) < 25   # correlated blocks: a dropped or doubled block shows
    nac = N if na is None else int(na.sum())
    outs = []
    for layout, mode in COMBOS:
        with _shard(bed, N, M, S=S, layout=layout, mode=mode, na=na) as sh:
            assert sh.get_layout() == layout
            first = _check(sh, ref, B, M, nac, tag=(layout, mode))
            again = _check(sh, ref, B, M, nac, tag=(layout, mode, "again"))
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(first, again))
            info = sh.ld_info()
            assert info["seconds"] > 0 and info["block_pairs"] > 0 and info["scratch_bytes"] > 0
            j = np.arange(M)
            entries = (np.minimum(j + B, M - 1) - np.maximum(j - B, 0) + 1).sum()
            assert info["useful_macs"] == 4.0 * N * entries
            outs.append(first)
    for o in outs[1:]:               # layouts and kernel modes agree bit for bit
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(outs[0], o))
    band = outs[0][0]                # symmetry: band[j][B + d] == band[j + d][B - d], bit for bit
    for d in range(1, min(B, M - 1) + 1):
        assert np.array_equal(band[:M - d, B + d], band[d:, B - d]), d
    assert np.array_equal(band[:, B], ref["poly"].astype(np.float64))


def test_partial_band_rows_equal_the_full_band():
    N, S, M, B = 1003, 0, 700, 100
    bed = synth.synth_bed(N, M, seed=3, miss_ppm=20000, S=S, ld_block=48, ld_ppm=900000)
    with _shard(bed, N, M, S=S) as sh:
        full = sh.ld_band(B, 0, M)
        for j0, nj in ((0, 1), (63, 2), (130, 200), (699, 1), (640, 60), (5, 0)):
            assert np.array_equal(sh.ld_band(B, j0, nj), full[j0:j0 + nj]), (j0, nj)


def test_chromosome_boundaries():
    N, M, B = 1003, 700, 100
    bed = synth.synth_bed(N, M, seed=3, miss_ppm=20000, ld_block=48, ld_ppm=900000)
    chrom = np.zeros(M, dtype=np.int32)
    for k, edge in enumerate((0, 50, 64, 200, 333)):
        chrom[edge:] = k + 1
    ref = ldr.ld(bed, N, M, B)
    outs = []
    for layout in (1, 2):
        with _shard(bed, N, M, layout=layout) as sh:
            outs.append(_check(sh, ref, B, M, N, chrom=chrom, tag=layout))
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(*outs))
    band = outs[0][0]
    j = np.arange(M)
    for d in range(-B, B + 1):       # no pair across a boundary is non-zero
        k = j + d
        ok = (k >= 0) & (k < M)
        cross = ok.copy()
        cross[ok] = chrom[j[ok]] != chrom[k[ok]]
        assert np.all(band[cross, B + d] == 0), d
    free, _ = ldr.scores(ref["r"], ref["poly"], B)
    assert np.nanmax(np.abs(outs[0][1] - free)) > 0.1          # the boundaries cut real LD


def test_hand_placed_markers():
    N, M, B = 300, 130, 70
    rng = np.random.default_rng(4)
    g = rng.integers(0, 3, size=(N, M))
    g[rng.random((N, M)) < 0.02] = -1
    na = np.ones(N)
    na[::9] = 0.0
    g[:, 10] = 0                         # all zero
    g[:, 20] = -1                        # missing everywhere
    g[:, 31] = g[:, 30]                  # equal to its neighbour
    g[:, 41] = np.where(g[:, 40] >= 0, 2 - g[:, 40], -1)     # 2 - its neighbour
    g[:, 50] = np.abs(g[:, 50])          # complete, then missing at masked individuals only
    g[::9, 50] = -1
    for j, src in ((63, 5), (64, 5), (M - 1, 100)):      # both sides of a row-group edge and the last marker: copies, partly missing
        g[:, j] = g[:, src]
        g[rng.random(N) < 0.05, j] = -1
    bed = ldr.encode(g)
    ref = ldr.ld(bed, N, M, B, na=na)
    assert list(np.nonzero(~ref["poly"])[0]) == [10, 20]
    outs = []
    for layout in (1, 2):
        with _shard(bed, N, M, layout=layout, na=na) as sh:
            outs.append(_check(sh, ref, B, M, int(na.sum()), tag=layout))
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(*outs))
    band, l2, n = outs[0][:3]
    assert np.all(band[10] == 0) and np.all(band[20] == 0) and np.isnan(l2[[10, 20]]).all() and n[10] == 0 and n[20] == 0
    assert abs(band[30, B + 1] - 1) <= 1e-12 and abs(band[31, B - 1] - 1) <= 1e-12
    assert abs(band[40, B + 1] + 1) <= 1e-12
    g2 = g.copy()
    g2[::9, 50] = 0                      # what sits at a masked individual does not count
    with _shard(ldr.encode(g2), N, M, na=na) as sh:
        assert np.array_equal(sh.ld_band(B, 0, M), band)
    assert band[63, B + 1] > 0.8 and band[64, B - 1] == band[63, B + 1] and band[M - 1, B + 100 - (M - 1)] > 0.8
    assert band[5, B + 58] > 0.8 and band[5, B + 59] > 0.8
    assert np.all(band[M - 1, B + 1:] == 0)


def test_driver_ldscore_mode_equals_the_binding_and_refuses_dosage(tmp_path):
    N, Mt, B = 403, 300, 40
    bed = synth.synth_bed(N, Mt, seed=3, miss_ppm=20000, ld_block=48, ld_ppm=900000)
    bfile, pfile, bim = str(tmp_path / "g.bed"), str(tmp_path / "y.phen"), str(tmp_path / "g.bim")
    synth.write_bed(bfile, bed)
    chrom = np.where(np.arange(Mt) < 130, 1, 2).astype(np.int32)
    with open(bim, "w") as f:
        for i, ch in enumerate(chrom):
            f.write("%d\trs%d\t0\t%d\tA\tG\n" % (ch, i, i + 1))
    na = np.ones(N)
    na[::11] = 0.0
    y = np.random.default_rng(3).standard_normal(N)
    with open(pfile, "w") as f:
        for i in range(N):
            f.write("F%d I%d %s\n" % (i, i, repr(float(y[i])) if na[i] else "NA"))
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
    out = str(tmp_path / "out") + "/"
    base = [exe, "--run-mode", "ldscore", "--bed-file", bfile, "--bim-file", bim, "--phen-files", pfile, "--N", str(N), "--Mt", str(Mt),
            "--out-dir", out, "--out-name", "g", "--ld-window", str(B)]
    for adjust in (0, 1):
        res = subprocess.run(base + ["--ld-adjust", str(adjust)], capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        assert "LD scores: window %d" % B in res.stdout and "seconds" in res.stdout
        with _shard(bed, N, Mt, layout=3, na=na) as sh:
            l2, n = sh.ld_scores(B, chrom=chrom, adjusted=bool(adjust))
        assert np.array_equal(np.fromfile(out + "g_ldscore.bin"), l2, equal_nan=True)
        assert np.array_equal(np.fromfile(out + "g_ldscore_n.bin"), n)
        for f in ("g_ldscore.bin", "g_ldscore_n.bin"):
            os.remove(out + f)
    codes = str(tmp_path / "codes.u8")
    synth.synth_dosage(N, Mt, 1, 8).tofile(codes)
    cmd = [a if a != bfile else codes for a in base] + ["--geno-format", "dosage8"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "FATAL" in res.stdout and "dosage8" in res.stdout
    assert not os.path.exists(out + "g_ldscore.bin")


def test_refusals():
    N, M = 600, 256
    bed = synth.synth_bed(N, M, seed=1, miss_ppm=5000)
    with capi.Shard(N, M, device=0) as sh:        # methylation data
        sh.synth_meth(3)
        sh.compute_markers_statistics()
        with pytest.raises(capi.GvError, match="meth"):
            sh.ld_scores(10)
        with pytest.raises(capi.GvError, match="meth"):
            sh.ld_band(10, 0, 5)
    for dtype, bits in ((np.uint8, 8), (np.uint16, 16)):       # compact dosage data, by width
        with capi.Shard(N, M, device=0) as sh:
            sh.upload_dosage(synth.synth_dosage(N, M, 2, bits).astype(dtype), 1.0 / 127.0)
            sh.compute_markers_statistics()
            with pytest.raises(capi.GvError, match="%d-bit codes" % bits):
                sh.ld_scores(10)
            with pytest.raises(capi.GvError, match="%d-bit codes" % bits):
                sh.ld_band(10, 0, 5)
    with capi.Shard(N, M, device=0) as sh:        # raw rows only
        sh.set_layout(True, 0)
        sh.upload_bed(bed)
        sh.set_kernel_mode(0)
        sh.compute_markers_statistics()
        with pytest.raises(capi.GvError, match="re-encoded"):
            sh.ld_scores(10)
    with _shard(bed, N, M, stats=False) as sh:    # statistics not computed
        with pytest.raises(capi.GvError, match="statistics must be computed first"):
            sh.ld_scores(10)
        sh.compute_markers_statistics()
        sh.ld_scores(10)
        sh.set_mask(_mask4(np.ones(N)), N)        # a new mask drops them
        with pytest.raises(capi.GvError, match="statistics must be computed first"):
            sh.ld_band(10, 0, 5)
    with _shard(bed, N, M) as sh:
        for w in (0, 8193):
            with pytest.raises(capi.GvError, match="window must be in"):
                sh.ld_scores(w)
            with pytest.raises(capi.GvError, match="window must be in"):
                sh.ld_band(w, 0, 5)
        for j0, nj in ((-1, 5), (0, M + 1), (M, 1), (250, 7), (5, -1)):
            with pytest.raises(capi.GvError, match="outside the shard's markers"):
                sh.ld_band(10, j0, nj)
        assert sh.ld_band(8192, M - 1, 1).shape == (1, 2 * 8192 + 1)
    na = np.zeros(N)
    na[[3, 77]] = 1.0
    with _shard(bed, N, M, na=na) as sh:          # the adjusted estimator divides by n - 2
        with pytest.raises(capi.GvError, match="at least 3 phenotyped"):
            sh.ld_scores(10, adjusted=True)
        sh.ld_scores(10)


def test_the_context_is_left_as_it_was():
    N, M, S, W = 1203, 333, 37, 64
    bed = synth.synth_bed(N, M, seed=3, miss_ppm=20000, S=S, ld_block=48, ld_ppm=900000)
    x = np.random.default_rng(1).standard_normal(M)
    for layout, mode in ((1, 1), (2, 2)):
        with _shard(bed, N, M, S=S, layout=layout, mode=mode) as sh:
            sh.set_cg_precond("ld", W)
            z = sh.Ax(x)
            w = sh.ATx(z)
            info = sh.precond_info()
            grams = [sh.precond_window_gram(g, info["first_window"][g] + 1) for g in (0, 1)]
            sh.ld_scores(100)
            sh.ld_band(100, 10, 50)
            assert np.array_equal(sh.Ax(x), z) and np.array_equal(sh.ATx(z), w)
            for g in (0, 1):
                assert np.array_equal(sh.precond_window_gram(g, info["first_window"][g] + 1), grams[g])
            sh.set_cg_precond("scalar", W)            # ... and after the Grams were dropped and rebuilt
            sh.set_cg_precond("ld", W)
            sh.ld_scores(7, adjusted=True)
            for g in (0, 1):
                assert np.array_equal(sh.precond_window_gram(g, info["first_window"][g] + 1), grams[g])
