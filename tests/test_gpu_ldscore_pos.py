"""LD scores over a window of positions, partitioned by annotation category, on the GPU (gv_ld_scores_pos) against
the numpy restatement of tests/ld_pos_restatement.py: both layouts and both MFMA kernel modes, uniform / clustered / tied positions,
chromosomes, annotations of 1, 3 and 70 categories, bit-identity with gv_ld_scores, across calls, layouts, kernel modes and pass
counts, the count of the blocks launched, the refusals, the driver, and the rest of the context left as it was.

Tolerance: section 16's bar for l2, 1e-12 relative, scaled by the entry's own term magnitudes because signed annotations cancel:
|l - ref| <= 1e-12 (|a_jc| + sum_k |f_jk| |a_kc|).  npairs and the NaN positions are exact."""
import os
import subprocess

import numpy as np
import pytest

from gvamp_amd import capi, synth
import ld_pos_restatement as lpr
import ld_restatement as ldr
import precond_restatement as pr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMBOS = ((2, 1), (1, 1), (2, 2), (1, 2))          # (resident layout: 1 two stripe sets, 2 the tile layout; kernel mode)
N, S = 333, 37                                     # no multiple of 256 or 128: a masked tail; a few individuals without a phenotype


def _mask4(na):
    m = np.zeros((na.size + 3) // 4, dtype=np.uint8)
    for n in np.nonzero(na)[0]:
        m[n >> 2] |= 1 << (n & 3)
    return m


def _shard(bed, n, M, s=0, layout=2, mode=1, na=None, stats=True):
    sh = capi.Shard(n, M, Mt=s + M + 100, S=s, device=0)
    sh.set_layout(False, layout)
    sh.set_kernel_mode(mode)
    sh.upload_bed(bed)
    if na is not None:
        sh.set_mask(_mask4(na), int(na.sum()))
    if stats:
        sh.compute_markers_statistics()
    return sh


_DATA = {}


def _data(M):
    """genotypes with LD blocks and missing entries, hand-placed markers, the mask, and r / poly of the restatement -- once per M"""
    if M not in _DATA:
        a, b = pr.decode(synth.synth_bed(N, M, seed=5, miss_ppm=20000, S=S, ld_block=48, ld_ppm=900000), N, M)
        g = np.where(b > 0, a, -1).astype(np.int64)
        g[:, 10] = 0                         # all zero
        g[:, 20] = -1                        # missing everywhere
        g[:, 31] = g[:, 30]                  # equal to its neighbour
        g[:, 63] = g[:, 5]                   # a copy across the row-group edge ...
        g[::17, 63] = -1                     # ... partly missing
        na = np.ones(N)
        na[::13] = 0.0
        bed = ldr.encode(g)
        a, b = pr.decode(bed, N, M)
        mave, msig = pr.marker_stats(a, b, na)
        r, poly = ldr.corr(ldr.gram(a, b, na, mave, msig))
        assert list(np.nonzero(~poly)[0]) == [10, 20] and abs(r[30, 31] - 1) < 1e-12
        _DATA[M] = dict(bed=bed, na=na, r=r, poly=poly, nac=float(na.sum()), mave=mave)
    return _DATA[M]


@pytest.fixture(scope="module")
def shards():
    """one context per (M, layout, kernel mode), opened on first use and closed with the module"""
    held = {}

    def get(M, layout=2, mode=1):
        if (M, layout, mode) not in held:
            d = _data(M)
            held[(M, layout, mode)] = _shard(d["bed"], N, M, s=S, layout=layout, mode=mode, na=d["na"])
            assert held[(M, layout, mode)].get_layout() == layout
        return held[(M, layout, mode)]

    yield get
    for sh in held.values():
        sh.close()


def _positions(M):
    """name -> (pos, chrom or None, radius)"""
    j = np.arange(M)
    out = {"arange": (S + j * 1.0, None, 70.0)}
    if M == 300:
        # clustered: 0..39 alone (10 apart), 40..63 three to a radius, 64..279 two hundred to a radius (a reach across two block
        # boundaries and more), 280..299 alone again -- row groups 0 and 4 reach no other, row group 1 reaches three ahead
        gaps = np.where(j < 40, 10.0, np.where(j < 64, 0.3, np.where(j < 280, 0.005, 10.0)))
        gaps[40] = gaps[64] = gaps[280] = 10.0
        out["clustered"] = (np.cumsum(gaps), None, 1.0)
    else:
        gaps = np.where(j < 20, 10.0, 0.02)
        out["clustered"] = (np.cumsum(gaps), None, 1.0)
    ties = ((j + 6) // 7) * 1.0               # runs of seven equal positions: 57..63 | 64..70 are two runs, 1.0 apart
    out["ties, radius 0"] = (ties, None, 0.0)
    ties2 = ((j + 3) // 7) * 1.0              # 60..66 is one run straddling 63 / 64
    out["ties straddling 63 / 64, radius 0"] = (ties2, None, 0.0)
    out["ties straddling 63 / 64, radius 2"] = (ties2, None, 2.0)
    if M == 300:
        rng = np.random.default_rng(8)
        walk = np.cumsum(rng.exponential(1.0, M))
        ch2 = np.where(j < 100, 7, 3)
        out["two chromosomes, break at 100"] = (np.where(j < 100, walk, walk - walk[100]), ch2, 25.0)
        ch3 = np.repeat([2, 9, 4], [64, M - 65, 1])
        out["three chromosomes, breaks at 64 and M - 1"] = (walk, ch3, 90.0)
    return out


def _annots(M):
    rng = np.random.default_rng(9)
    a3 = rng.standard_normal((M, 3))
    a3[rng.random((M, 3)) < 0.4] = 0.0
    a3[:, 2] = -np.abs(a3[:, 2])
    a70 = (rng.random((M, 70)) < 0.3).astype(np.float64)
    a70[:, 1::5] *= rng.standard_normal((M, 14))
    return {"none": None, "ones": np.ones((M, 1)), "three": a3, "seventy": a70}


def _hold(got, want, tag):
    l2, n = got
    rl2, rn, mag = want
    assert l2.shape == rl2.shape, tag
    assert np.array_equal(np.isnan(l2), np.isnan(rl2)), tag
    assert np.array_equal(n, rn), tag
    ok = ~np.isnan(rl2)
    err, bar = np.abs(l2[ok] - rl2[ok]), mag[ok]          # (an entry whose annotation values are all zero is held to 0)
    print("max |l - ref| / (|a| + sum |f| |a|) = %.3e" % (err[bar > 0] / bar[bar > 0]).max(), tag)
    assert np.all(err <= 1e-12 * bar), tag


@pytest.mark.parametrize("M", [300, 64])
def test_scores_match_restatement_on_both_layouts_and_modes(shards, M):
    d = _data(M)
    annots = _annots(M)
    for pname, (pos, chrom, radius) in _positions(M).items():
        hi = lpr.window_hi(pos, radius, chrom)
        if M == 300 and pname == "clustered":
            reach = hi - np.arange(M)
            assert (reach[:40] == 0).all() and reach.max() > 128 and lpr.dmax_of(hi) >= 3
            assert hi[63] == 63 and hi[299] == 299                   # row groups 0 and 4 reach no other
        for aname, annot in annots.items():
            for adjusted in (False, True):
                want = lpr.scores_pos(d["r"], d["poly"], pos, radius, chrom, adjusted, d["nac"], annot, scale=True)
                assert np.array_equal(np.isnan(want[0]).reshape(M, -1).all(1), ~d["poly"])
                outs = []
                for layout, mode in COMBOS:
                    sh = shards(M, layout, mode)
                    got = sh.ld_scores_pos(pos, radius, chrom=chrom, adjusted=adjusted, annot=annot)
                    _hold(got, want, (pname, aname, adjusted, layout, mode))
                    outs.append(got)
                    if (layout, mode) == COMBOS[0]:
                        # 3. the blocks computed are those an in-band pair lies in; the useful MACs are the band's entries
                        info = sh.ld_info()
                        assert info["block_pairs"] == lpr.block_pairs(hi), (pname, info)
                        assert info["useful_macs"] == 4.0 * N * lpr.entries(pos, radius, chrom), (pname, info)
                        assert info["seconds"] > 0 and info["scratch_bytes"] > 0 and sh.ld_last_passes() == 1
                        again = sh.ld_scores_pos(pos, radius, chrom=chrom, adjusted=adjusted, annot=annot)          # two calls
                        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(got, again))
                for o in outs[1:]:               # layouts and kernel modes agree bit for bit
                    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(outs[0], o)), (pname, aname, adjusted)
            # a ones column is no annotation, bit for bit
            sh = shards(M)
            a = sh.ld_scores_pos(pos, radius, chrom=chrom)
            b = sh.ld_scores_pos(pos, radius, chrom=chrom, annot=annots["ones"])
            assert b[0].shape == (M, 1) and np.array_equal(a[0], b[0][:, 0], equal_nan=True) and np.array_equal(a[1], b[1])
    if M == 300:        # only the blocks that hold an in-band pair are launched: fewer than the rectangle (row groups, dmax + 1)
        pos, chrom, radius = _positions(M)["clustered"]
        hi = lpr.window_hi(pos, radius, chrom)
        assert lpr.block_pairs(hi) == 1 + 4 + 3 + 2 + 1 and lpr.block_pairs(hi) < sum(min(3, 4 - I) + 1 for I in range(5))


@pytest.mark.parametrize("B", [1, 63, 64, 200])
def test_index_positions_give_the_bits_of_gv_ld_scores(shards, B):
    M = 300
    j = np.arange(M)
    chroms = (None, np.repeat([5, 1, 8, 2], [50, 14, 136, 100]).astype(np.int32))
    for layout, mode in COMBOS:
        sh = shards(M, layout, mode)
        for chrom in chroms:
            for adjusted in (False, True):
                want = sh.ld_scores(B, chrom=chrom, adjusted=adjusted)
                got = sh.ld_scores_pos(S + j * 1.0, float(B), chrom=chrom, adjusted=adjusted)
                assert got[0].shape == (M,)
                assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1]), (layout, mode, adjusted)
    sh = shards(64)
    want = sh.ld_scores(B)
    got = sh.ld_scores_pos(S + np.arange(64.0), float(B))
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1])


def test_the_longest_reach_and_the_reach_refusal():
    """8193 markers at one position: every marker reaches the last one, marker 0 exactly 8192 ahead (dmax = 128), and the scores are
    those of the widest index window bit for bit; one marker more is refused by name"""
    n, M = 40, 8194
    bed = synth.synth_bed(n, M, seed=2, miss_ppm=20000, ld_block=48, ld_ppm=900000)
    with _shard(bed, n, M) as sh:
        with pytest.raises(capi.GvError, match=r"marker 0 reaches 8193 markers ahead"):
            sh.ld_scores_pos(np.zeros(M), 0.0)
        pos = np.zeros(M)
        pos[-1] = 1.0
        got = sh.ld_scores_pos(pos, 0.5)
        info = sh.ld_info()
        chrom = np.zeros(M, dtype=np.int32)
        chrom[-1] = 1
        want = sh.ld_scores(8192, chrom=chrom)
        assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1])
        assert got[1][0] <= 8193 and got[1][-1] == 1.0
        hi = np.full(M, M - 2)
        hi[-1] = M - 1
        assert np.array_equal(hi, lpr.window_hi(pos, 0.5)) and lpr.dmax_of(hi) == 128
        assert info["block_pairs"] == lpr.block_pairs(hi)
        assert info["useful_macs"] == 4.0 * n * ((M - 1) ** 2 + 1)


def test_the_passes_change_no_bit(monkeypatch):
    M, C_ = 300, 70
    d = _data(M)
    pos, chrom, radius = _positions(M)["clustered"]
    annot = _annots(M)["seventy"]
    dmax = lpr.dmax_of(lpr.window_hi(pos, radius, chrom))
    per_rg = (2 * dmax + 1) * 64 * (8 * C_ + 4)          # one row group's worth of slots, bytes
    assert dmax == 3 and (M + 63) // 64 == 5
    outs = {}
    for rgs, passes in ((5, 1), (4, 2), (2, 3), (1, 5)):      # row groups that fit the budget -> passes over the five
        monkeypatch.setenv("GV_LD_PART_MB", "%.6f" % ((rgs * per_rg + 2000) / 2.0 ** 20))
        with _shard(d["bed"], N, M, s=S, na=d["na"]) as sh:
            monkeypatch.delenv("GV_LD_PART_MB")
            for adjusted in (False, True):
                outs[(passes, adjusted)] = sh.ld_scores_pos(pos, radius, chrom=chrom, adjusted=adjusted, annot=annot)
                assert sh.ld_last_passes() == passes
            outs[(passes, "plain")] = sh.ld_scores_pos(pos, radius)
            # (one category: five row groups of 7 * 64 * 12 bytes fit every one of these budgets)
            assert sh.ld_last_passes() == 1
            sh.ld_scores(64)
            assert sh.ld_last_passes() == 1
    for key in (False, True, "plain"):
        for passes in (2, 3, 5):
            assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(outs[(1, key)], outs[(passes, key)])), (passes, key)
    want = lpr.scores_pos(d["r"], d["poly"], pos, radius, chrom, False, d["nac"], annot, scale=True)
    _hold(outs[(5, False)], want, "five passes")
    # several passes of one category: 2 row groups' worth of 7 * 64 * 12 bytes
    monkeypatch.setenv("GV_LD_PART_MB", "%.6f" % ((2 * 7 * 64 * 12 + 100) / 2.0 ** 20))
    with _shard(d["bed"], N, M, s=S, na=d["na"]) as sh:
        got = sh.ld_scores_pos(pos, radius)
        assert sh.ld_last_passes() == 3
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(got, outs[(1, "plain")]))
        with pytest.raises(capi.GvError, match="GV_LD_PART_MB.*cannot hold one row group"):        # a budget below one row group's worth
            sh.ld_scores_pos(pos, radius, annot=annot)
    for bad in ("0", "-3", "lots", "nan"):
        monkeypatch.setenv("GV_LD_PART_MB", bad)
        with pytest.raises(capi.GvError, match="GV_LD_PART_MB"):
            capi.Shard(N, M, device=0)


def test_refusals(shards):
    M = 300
    d = _data(M)
    pos = np.arange(M) * 1.0
    n2, M2 = 600, 256
    with capi.Shard(n2, M2, device=0) as sh:        # methylation data
        sh.synth_meth(3)
        sh.compute_markers_statistics()
        with pytest.raises(capi.GvError, match="meth"):
            sh.ld_scores_pos(np.arange(M2) * 1.0, 3.0)
    for dtype, bits in ((np.uint8, 8), (np.uint16, 16)):       # compact dosage data, by width, with and without gv_set_ld_dosage
        with capi.Shard(n2, M2, device=0) as sh:
            sh.upload_dosage(synth.synth_dosage(n2, M2, 2, bits).astype(dtype), 1.0 / 127.0)
            sh.set_mask(_mask4(np.ones(n2)), n2)
            sh.compute_markers_statistics()
            for on in (0, 1):
                sh.set_ld_dosage(on)
                with pytest.raises(capi.GvError, match=r"bed data only.*%d-bit codes.*gv_set_ld_dosage" % bits):
                    sh.ld_scores_pos(np.arange(M2) * 1.0, 3.0)
            if bits == 8:
                sh.ld_scores(10)                      # (the index window serves them under the option)
    with capi.Shard(N, M, device=0) as sh:        # raw rows only
        sh.set_layout(True, 0)
        sh.upload_bed(d["bed"])
        sh.set_kernel_mode(0)
        sh.compute_markers_statistics()
        with pytest.raises(capi.GvError, match="re-encoded"):
            sh.ld_scores_pos(pos, 3.0)
    with _shard(d["bed"], N, M, stats=False) as sh:    # statistics not computed
        with pytest.raises(capi.GvError, match="statistics must be computed first"):
            sh.ld_scores_pos(pos, 3.0)
    sh = shards(M)
    with pytest.raises(capi.GvError, match="pos is NULL"):
        sh.ld_scores_pos(None, 3.0)
    for radius in (-1.0, float("nan"), float("inf")):
        with pytest.raises(capi.GvError, match="radius must be finite and >= 0"):
            sh.ld_scores_pos(pos, radius)
    bad = pos.copy()
    bad[5] = np.nan
    with pytest.raises(capi.GvError, match=r"pos\[5\] is not finite"):
        sh.ld_scores_pos(bad, 3.0)
    bad = pos.copy()
    bad[200] = np.inf
    with pytest.raises(capi.GvError, match=r"pos\[200\] is not finite"):
        sh.ld_scores_pos(bad, 3.0)
    bad = pos.copy()
    bad[77] = 75.5
    with pytest.raises(capi.GvError, match=r"pos\[77\] = 75.5 is below pos\[76\] = 76 .*must not decrease"):
        sh.ld_scores_pos(bad, 3.0)
    sh.ld_scores_pos(bad, 3.0, chrom=np.where(np.arange(M) < 77, 1, 2))          # (a new chromosome may start lower)
    with pytest.raises(capi.GvError, match="chromosome id 1 reappears at marker 100"):
        sh.ld_scores_pos(pos, 3.0, chrom=np.repeat([1, 2, 1], [50, 50, 200]))
    sh.ld_scores(3, chrom=np.repeat([1, 2, 1], [50, 50, 200]))                   # (the index window serves that layout)
    for ncat in (0, 513):
        with pytest.raises(capi.GvError, match=r"ncat must be in \[1, 512\]"):
            sh.ld_scores_pos(pos, 3.0, annot=np.ones((M, ncat)))
    assert sh.ld_scores_pos(pos, 3.0, annot=np.ones((M, 512)))[0].shape == (M, 512)
    na = np.zeros(N)
    na[[3, 77]] = 1.0
    with _shard(d["bed"], N, M, na=na) as sh2:          # the adjusted estimator divides by n - 2
        with pytest.raises(capi.GvError, match="at least 3 phenotyped"):
            sh2.ld_scores_pos(pos, 3.0, adjusted=True)
        sh2.ld_scores_pos(pos, 3.0)


def test_the_context_is_left_as_it_was():
    M = 300
    d = _data(M)
    x = np.random.default_rng(1).standard_normal(M)
    pos, chrom, radius = _positions(M)["clustered"]
    for layout, mode in ((1, 1), (2, 2)):
        with _shard(d["bed"], N, M, s=S, layout=layout, mode=mode, na=d["na"]) as sh:
            z = sh.Ax(x)
            w = sh.ATx(z)
            l2 = sh.ld_scores(100, adjusted=True)
            band = sh.ld_band(100, 10, 50)
            sh.ld_scores_pos(pos, radius, annot=_annots(M)["three"], adjusted=True)
            sh.ld_scores_pos(S + np.arange(M) * 1.0, 100.0)
            assert np.array_equal(sh.Ax(x), z) and np.array_equal(sh.ATx(z), w)
            again = sh.ld_scores(100, adjusted=True)
            assert np.array_equal(again[0], l2[0], equal_nan=True) and np.array_equal(again[1], l2[1])
            assert np.array_equal(sh.ld_band(100, 10, 50), band)


def test_driver_windows_by_distance_and_annotation(tmp_path):
    n, Mt = 203, 150
    a, b = pr.decode(synth.synth_bed(n, Mt, seed=3, miss_ppm=20000, ld_block=48, ld_ppm=900000), n, Mt)
    g = np.where(b > 0, a, -1).astype(np.int64)
    g[:, 12] = 2                              # monomorphic: no score, and not counted in the category sums
    g[:, 40] = np.where(np.arange(n) == 5, 1, 0)          # a rare allele: below the frequency bar of the second line
    bed = ldr.encode(g)
    bfile, pfile, bim, afile = (str(tmp_path / f) for f in ("g.bed", "y.phen", "g.bim", "g.annot"))
    synth.write_bed(bfile, bed)
    rng = np.random.default_rng(6)
    j = np.arange(Mt)
    chrom = np.where(j < 90, 1, 2).astype(np.int32)
    bp = np.cumsum(rng.integers(1, 4000, Mt))
    bp = np.where(j < 90, bp, bp - bp[90] + 500)
    cm = bp * 1.3e-4
    annot = np.ones((Mt, 3))
    annot[:, 1] = rng.random(Mt) < 0.3
    annot[:, 2] = np.round(rng.standard_normal(Mt), 3)
    with open(bim, "w") as f:
        for i in range(Mt):
            f.write("%d\trs%d\t%s\t%d\tA\tG\n" % (chrom[i], i, repr(float(cm[i])), bp[i]))
    with open(afile, "w") as f:
        f.write("CHR BP SNP CM base coding cont\n")
        for i in range(Mt):
            f.write("%d %d rs%d %s %d %d %s\n" % (chrom[i], bp[i], i, repr(float(cm[i])), 1, annot[i, 1], repr(float(annot[i, 2]))))
    na = np.ones(n)
    na[::11] = 0.0
    y = rng.standard_normal(n)
    with open(pfile, "w") as f:
        for i in range(n):
            f.write("F%d I%d %s\n" % (i, i, repr(float(y[i])) if na[i] else "NA"))
    a, b = pr.decode(bed, n, Mt)
    mave, msig = pr.marker_stats(a, b, na)
    r, poly = ldr.corr(ldr.gram(a, b, na, mave, msig))
    assert not poly[12] and poly.sum() == Mt - 1
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
    out = str(tmp_path / "out") + "/"
    base = [exe, "--run-mode", "ldscore", "--bed-file", bfile, "--phen-files", pfile, "--N", str(n), "--Mt", str(Mt), "--out-dir", out,
            "--out-name", "g"]
    files = ("g_ldscore.bin", "g_ldscore_n.bin", "g_ldscore_M.txt", "g_ldscore_cats.txt")
    for flag, value, pos, radius in (("--ld-wind-kb", "20", bp * 1.0, 20000.0), ("--ld-wind-cm", "2.5", cm, 2.5)):
        for with_annot in (False, True):
            cmd = base + ["--bim-file", bim, flag, value, "--ld-adjust", "1"] + (["--ld-annot", afile] if with_annot else [])
            res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
            assert "LD scores: window %s %s (adjusted)" % (value, "kb" if "kb" in flag else "cM") in res.stdout
            want = lpr.scores_pos(r, poly, pos, radius, chrom, True, float(na.sum()), annot if with_annot else None, scale=True)
            l2 = np.fromfile(out + files[0])
            _hold((l2.reshape(Mt, 3) if with_annot else l2, np.fromfile(out + files[1])), want, (flag, with_annot))
            assert os.path.exists(out + files[2]) == with_annot and os.path.exists(out + files[3]) == with_annot
            if with_annot:
                with open(out + files[3]) as f:
                    assert f.read().split() == ["base", "coding", "cont"]
                tot = np.loadtxt(out + files[2])
                maf = np.minimum(mave / 2.0, 1.0 - mave / 2.0)
                assert maf[40] < 0.05 < np.median(maf)
                assert tot.shape == (2, 3)
                assert np.allclose(tot[0], annot[poly].sum(0), rtol=1e-13, atol=1e-13)
                assert np.allclose(tot[1], annot[poly & (maf > 0.05)].sum(0), rtol=1e-13, atol=1e-13)
                assert tot[0, 0] == Mt - 1 and tot[1, 0] < tot[0, 0]
            for f in files:
                if os.path.exists(out + f):
                    os.remove(out + f)
    # the FATAL lines
    res = subprocess.run(base + ["--bim-file", bim, "--ld-wind-kb", "20", "--ld-window", "50"], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "FATAL: exactly one of --ld-window, --ld-wind-kb and --ld-wind-cm" in res.stdout
    res = subprocess.run(base + ["--ld-wind-cm", "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "FATAL: --ld-wind-cm needs --bim-file" in res.stdout
    short = str(tmp_path / "short.annot")
    with open(afile) as f, open(short, "w") as fo:
        fo.writelines(f.readlines()[:-2])
    res = subprocess.run(base + ["--bim-file", bim, "--ld-wind-kb", "20", "--ld-annot", short], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "FATAL: annotation file" in res.stdout and "ends after line 149: 148 rows for 150 markers" in res.stdout
    notfinite = str(tmp_path / "nan.annot")          # a non-finite annotation value is refused, naming the line
    with open(afile) as f, open(notfinite, "w") as fo:
        lines = f.readlines()
        lines[7] = lines[7].rsplit(" ", 1)[0] + " nan\n"
        fo.writelines(lines)
    res = subprocess.run(base + ["--bim-file", bim, "--ld-wind-kb", "20", "--ld-annot", notfinite], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "FATAL: line 8 of annotation file" in res.stdout and "is not finite" in res.stdout
    assert not os.path.exists(out + files[0])
