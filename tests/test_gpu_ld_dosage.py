"""LD scores and banded LD correlations of 8-bit dosage codes on the GPU (gv_set_ld_dosage) against the integer
restatement of tests/ld_dosage_restatement.py: the one-product kernel at both block edges and the forced four-product kernel, plain
codes, a phenotype mask, missing entries; bit-identity across instantiations, calls, mirror images and segment lengths; chromosomes,
hand-placed rows, the int32 bound, the driver, the refusals, and the rest of the context left as it was.

Bars (from the definition, not from the kernel): r is four correctly rounded operations (a product, a square root, a quotient, on
correctly rounded integers), doubled in case the device sqrt or / is off by an ulp: |r - ref| <= 16 * 2^-53.  l_j adds at most 2B terms
f(r^2), each within 16 * 2^-53 relative of its reference, one rounding per addition and the 1:
|l2 - ref| <= (16 + 2B + 1) * 2^-53 * (1 + sum |f(r^2)|).  npairs, the NaN positions and the zeros outside the band are exact."""
import contextlib
import functools
import os
import subprocess

import numpy as np
import pytest

from gvamp_amd import capi, synth
import ld_dosage_restatement as ldd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53
INSTS = ("uniform128", "uniform64", "forced4")       # the one-product kernel at either edge; GV_DOSAGE_NA_KERNELS=1: four products
ENV = {"uniform128": dict(GV_LD_DOSAGE_EDGE=128), "uniform64": dict(GV_LD_DOSAGE_EDGE=64), "forced4": dict(GV_DOSAGE_NA_KERNELS=1)}


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    for k, v in kv.items():
        os.environ[k] = str(v)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _mask4(na):
    m = np.zeros((na.size + 3) // 4, dtype=np.uint8)
    for n in np.nonzero(na)[0]:
        m[n >> 2] |= 1 << (n & 3)
    return m


def _shard(codes, na=None, missing=False, inst="uniform128", seg=None, on=True):
    """a context with the codes resident; the development switches are read by gv_create, per context, and cleared again at once"""
    M, N = codes.shape
    env = dict(ENV[inst])
    if seg is not None:
        env["GV_DOSAGE_MFMA_SEG"] = seg
    with _env(**env):
        sh = capi.Shard(N, M, device=0)
    sh.upload_dosage(codes, 1.0 / 127.0, missing=missing)
    if na is not None:
        sh.set_mask(_mask4(na), int(na.sum()))
    if on:
        sh.set_ld_dosage(1)
    return sh


def _check(sh, ref, B, nonas, chrom=None, tag=None):
    """band over all rows, scores raw and adjusted against the restatement; returns what must be bit-identical elsewhere"""
    r, poly = ref["r"], ref["poly"]
    M = r.shape[0]
    got = sh.ld_band(B, 0, M, chrom=chrom)
    want = ldd.band(r, B, 0, M, chrom)
    assert got.shape == want.shape
    print("max |r - ref| / 2^-53 = %.3f" % (np.max(np.abs(got - want)) / U), tag)
    assert np.max(np.abs(got - want)) <= 16 * U, tag
    assert np.all(got[ldd.band(np.ones((M, M)), B, 0, M, chrom) == 0] == 0), tag          # exact zeros outside the band
    out = [got]
    for adjusted in (False, True):
        if adjusted and nonas < 3:
            continue
        l2, n = sh.ld_scores(B, chrom=chrom, adjusted=adjusted)
        rl2, rn = ldd.scores(r, poly, B, chrom, adjusted, float(nonas))
        assert np.array_equal(np.isnan(l2), np.isnan(rl2)) and np.array_equal(np.isnan(l2), ~poly), tag
        assert np.array_equal(n, rn), tag
        ok = ~np.isnan(rl2)
        if ok.any():
            bar = (16 + 2 * B + 1) * U * (1.0 + ldd.abs_terms(r, poly, B, chrom, adjusted, float(nonas)))
            print("max |l2 - ref| / bar = %.3e" % np.max(np.abs(l2[ok] - rl2[ok]) / bar[ok]), tag, adjusted)
            assert np.all(np.abs(l2[ok] - rl2[ok]) <= bar[ok]), (tag, adjusted)
        out += [l2, n]
    return out


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


SHAPES = {(5, 3): (1, 2), (70, 1): (1,), (403, 300): (1, 40, 64, 65), (1003, 257): (128, 129, 300), (4099, 130): (8192,)}
CASES = ("plain", "masked", "missing")


@functools.lru_cache(maxsize=None)
def _case(N, M, case):
    """(codes, na, missing, reference): computed once and shared.  plain and masked codes hold no 255 (clamped), so that the same
    data serve the one-product kernel and the forced four-product kernel, which reads 255 as missing"""
    codes = synth.synth_dosage_na(N, M, 11, 8, 20000 if case == "missing" else 0)
    na = None
    if case != "plain":
        na = np.ones(N)
        na[::7] = 0.0
    missing = case == "missing"
    if not missing:
        assert not np.any(codes == 255)
    return codes, na, missing, ldd.ld(codes, na, missing)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("N,M", list(SHAPES))
def test_band_and_scores_match_the_restatement_in_every_instantiation(N, M, case):
    codes, na, missing, ref = _case(N, M, case)
    nonas = N if na is None else int(na.sum())
    outs = {}
    for inst in INSTS:
        # the forced kernel needs the codes uploaded under the missing option; without a reserved code that changes no value
        with _shard(codes, na, missing or inst == "forced4", inst) as sh:
            assert sh.get_ld_dosage() == 1
            info = sh.dosage_info()
            four = inst == "forced4" or bool(np.any(codes == 255))             # what dosage_na_kernels() decides
            assert info["na_kernels"] == four, (inst, info)
            res = []
            for B in SHAPES[(N, M)]:
                first = _check(sh, ref, B, nonas, tag=(N, M, case, inst, B))
                st = sh.ld_info()
                j = np.arange(M)
                entries = (np.minimum(j + B, M - 1) - np.maximum(j - B, 0) + 1).sum()
                assert st["useful_macs"] == (4.0 if four else 1.0) * N * entries, (inst, B)
                assert st["seconds"] > 0 and st["block_pairs"] > 0 and st["scratch_bytes"] > 0
                again = _check(sh, ref, B, nonas, tag=(N, M, case, inst, B, "again"))
                assert _same(first, again)                                    # two calls on the same context
                band = first[0]
                for d in range(1, min(B, M - 1) + 1):                         # r_jk and r_kj are the same bits
                    assert np.array_equal(band[:M - d, B + d], band[d:, B - d]), d
                assert np.array_equal(band[:, B], ref["poly"].astype(np.float64))
                res += first
            outs[inst] = res
    # data without a reserved code: the one-product and the four-product kernel agree bit for bit; with one, every context ran the
    # four-product kernel
    for inst in INSTS[1:]:
        assert _same(outs[INSTS[0]], outs[inst]), inst


def test_marker_statistics_do_not_matter_and_partial_rows_equal_the_full_band():
    N, M, B = 403, 300, 65
    codes, na, missing, ref = _case(N, M, "masked")
    with _shard(codes, na) as sh:
        full = sh.ld_band(B, 0, M)
        l2 = sh.ld_scores(B)
        sh.compute_markers_statistics()
        assert np.array_equal(sh.ld_band(B, 0, M), full) and _same(sh.ld_scores(B), l2)
        for j0, nj in ((0, 1), (63, 2), (127, 2), (130, 100), (299, 1), (240, 60), (5, 0)):
            assert np.array_equal(sh.ld_band(B, j0, nj), full[j0:j0 + nj]), (j0, nj)


@pytest.mark.parametrize("case", ["masked", "missing"])
def test_a_short_segment_changes_no_bit(case):
    N, M, B = 1003, 257, 129
    codes, na, missing, ref = _case(N, M, case)
    nonas = int(na.sum())
    outs = []
    for seg in (None, 64):          # 64: rounded down to the kernel's K-step, at least one step -- every step flushes
        with _shard(codes, na, missing, seg=seg) as sh:
            outs.append(_check(sh, ref, B, nonas, tag=(case, seg)))
    assert _same(*outs)


@pytest.mark.parametrize("inst", INSTS)
def test_chromosome_boundaries_off_the_block_edges(inst):
    N, M, B = 403, 300, 65
    codes, na, missing, ref = _case(N, M, "masked")
    chrom = np.zeros(M, dtype=np.int32)
    for k, edge in enumerate((0, 50, 100, 130, 200)):
        chrom[edge:] = k + 1
    with _shard(codes, na, inst == "forced4", inst) as sh:
        out = _check(sh, ref, B, int(na.sum()), chrom=chrom, tag=inst)
    band = out[0]
    j = np.arange(M)
    for d in range(-B, B + 1):       # no pair across a boundary is non-zero
        k = j + d
        ok = (k >= 0) & (k < M)
        cross = ok.copy()
        cross[ok] = chrom[j[ok]] != chrom[k[ok]]
        assert np.all(band[cross, B + d] == 0), d
    free, _ = ldd.scores(ref["r"], ref["poly"], B)
    assert np.nanmax(np.abs(out[1] - free)) > 1e-3            # the boundaries cut real terms


EDGE_ROWS = (62, 63, 64, 65, 126, 127, 128, 129)


def _hand_placed(missing):
    """rows at the 63 / 64 and 127 / 128 block edges and at M - 1"""
    N, M = 300, 200
    rng = np.random.default_rng(4)
    codes = synth.synth_dosage_na(N, M, 5, 8, 20000 if missing else 0)
    na = np.ones(N)
    na[::9] = 0.0
    rare = np.where(rng.random((3, N)) < 0.02, 254, 253).astype(np.uint8)
    codes[63] = 77                                   # constant
    codes[64] = codes[62]                            # equal to a neighbour across nothing ...
    codes[128] = codes[127]                          # ... and across a block edge
    codes[65], codes[126], codes[M - 1] = rare       # rare-variant rows
    if missing:
        codes[127][rng.random(N) < 0.05] = 255
        codes[128] = codes[127]
        codes[129] = 255                             # missing everywhere
        codes[M - 2] = np.where(codes[M - 2] == 255, 17, codes[M - 2])      # complete, then missing at masked individuals only
        base = codes[M - 2].copy()
        codes[M - 2][::9] = 255
    else:
        codes[129] = 255 - codes[128]                # 255 is the value 255
        codes[M - 2] = 255 - codes[M - 1]
        base = None
    return codes, na, base


@pytest.mark.parametrize("missing", [False, True])
def test_hand_placed_rows(missing):
    B = 70
    codes, na, base = _hand_placed(missing)
    M, N = codes.shape
    ref = ldd.ld(codes, na, missing)
    mono = [63, 129] if missing else [63]
    assert list(np.nonzero(~ref["poly"])[0]) == mono
    outs = []
    for inst in (("uniform128", "forced4") if missing else ("uniform128", "uniform64")):
        with _shard(codes, na, missing, inst) as sh:
            outs.append(_check(sh, ref, B, int(na.sum()), tag=(missing, inst)))
            if missing:
                c2 = codes.copy()
                c2[M - 2] = base                     # what sits at a masked individual does not count
                with _shard(c2, na, missing, inst) as s2:
                    assert np.array_equal(s2.ld_band(B, 0, M), outs[-1][0])
    assert _same(*outs)
    band, l2, n = outs[0][:3]
    for j in mono:
        assert np.all(band[j] == 0) and np.isnan(l2[j]) and n[j] == 0
    assert abs(band[62, B + 2] - 1) <= 16 * U and abs(band[127, B + 1] - 1) <= 16 * U and band[128, B - 1] == band[127, B + 1]
    if not missing:
        assert abs(band[128, B + 1] + 1) <= 16 * U and abs(band[M - 2, B + 1] + 1) <= 16 * U
    assert np.all(band[M - 1, B + 1:] == 0)


@pytest.mark.parametrize("seg", [None, 64])
def test_the_int32_bound(seg):
    """N = 140 000 > 131 071: the segmented instantiation at the default cap too; tests/test_ld_dosage_cpu.py shows that these rows wrap
    an unsegmented int32 sum"""
    codes = ldd.bound_case()
    M, N = codes.shape
    ref = _bound_ref()
    B = M - 1
    for inst in ("uniform128", "uniform64"):
        with _shard(codes, inst=inst, seg=seg) as sh:
            band, l2, n = _check(sh, ref, B, N, tag=("bound", inst, seg))[:3]
        assert abs(band[0, B + 1] + 1.0) <= 16 * U and band[1, B - 1] == band[0, B + 1] and ref["r"][0, 1] == -1.0
        assert np.all(np.isfinite(band)) and np.all(np.isfinite(l2)) and np.all(n == M)


@functools.lru_cache(maxsize=None)
def _bound_ref():
    return ldd.ld(ldd.bound_case())


def _driver_files(tmp_path, codes, na, chrom):
    M, N = codes.shape
    cfile, pfile, bim = str(tmp_path / "codes.u8"), str(tmp_path / "y.phen"), str(tmp_path / "g.bim")
    codes.tofile(cfile)
    with open(bim, "w") as f:
        for i, ch in enumerate(chrom):
            f.write("%d\trs%d\t0\t%d\tA\tG\n" % (ch, i, i + 1))
    y = np.random.default_rng(3).standard_normal(N)
    with open(pfile, "w") as f:
        for i in range(N):
            f.write("F%d I%d %s\n" % (i, i, repr(float(y[i])) if na[i] else "NA"))
    out = str(tmp_path / "out") + "/"
    exe = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
    return [exe, "--run-mode", "ldscore", "--bed-file", cfile, "--bim-file", bim, "--phen-files", pfile, "--N", str(N), "--Mt", str(M),
            "--out-dir", out, "--out-name", "g", "--ld-window", "40"], out


@pytest.mark.parametrize("missing", [0, 1])
def test_driver_ldscore_mode_equals_the_binding(tmp_path, missing):
    N, M, B = 403, 300, 40
    codes, na, _, _ = _case(N, M, "missing" if missing else "masked")
    chrom = np.where(np.arange(M) < 130, 1, 2).astype(np.int32)
    base, out = _driver_files(tmp_path, codes, na, chrom)
    for adjust in (0, 1):
        cmd = base + ["--geno-format", "dosage8", "--ld-dosage", "1", "--dosage-missing", str(missing), "--ld-adjust", str(adjust)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
        assert "LD scores: window %d" % B in res.stdout
        with _shard(codes, na, bool(missing)) as sh:
            l2, n = sh.ld_scores(B, chrom=chrom, adjusted=bool(adjust))
        assert np.array_equal(np.fromfile(out + "g_ldscore.bin"), l2, equal_nan=True)
        assert np.array_equal(np.fromfile(out + "g_ldscore_n.bin"), n)
        for f in ("g_ldscore.bin", "g_ldscore_n.bin"):
            os.remove(out + f)


def test_driver_refusals(tmp_path):
    N, M = 403, 300
    codes, na, _, _ = _case(N, M, "masked")
    base, out = _driver_files(tmp_path, codes, na, np.ones(M, dtype=np.int32))
    runs = [(base + ["--geno-format", "dosage8"], {}, "dosage8"),                                   # without the flag
            (base + ["--geno-format", "dosage8", "--ld-dosage", "0"], {}, "dosage8"),
            (base + ["--geno-format", "dosage16", "--ld-dosage", "1"], {}, "dosage16"),
            (base + ["--geno-format", "dosage8", "--ld-dosage", "1"], {"WORLD_SIZE": "2", "RANK": "0"}, "one rank")]
    for cmd, env, word in runs:
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(os.environ, **env))
        assert res.returncode != 0 and "FATAL" in res.stdout and word in res.stdout, (word, res.stdout[-2000:])
        assert not os.path.exists(out + "g_ldscore.bin")


def test_refusals():
    N, M = 600, 256
    codes = synth.synth_dosage(N, M, 2, 8)
    with capi.Shard(N, M, device=0) as sh:
        assert sh.get_ld_dosage() == 0                  # the default
        sh.upload_dosage(codes, 1.0 / 127.0)
        with pytest.raises(capi.GvError, match="8-bit codes"):
            sh.ld_scores(10)
        sh.set_ld_dosage(1)
        sh.ld_scores(10)
        sh.ld_band(10, 0, 5)
        sh.set_ld_dosage(0)                             # off again: the refusal of before
        assert sh.get_ld_dosage() == 0
        with pytest.raises(capi.GvError, match="not available for compact dosage data \\(8-bit codes\\)"):
            sh.ld_scores(10)
        with pytest.raises(capi.GvError, match="not available for compact dosage data \\(8-bit codes\\)"):
            sh.ld_band(10, 0, 5)
        with pytest.raises(capi.GvError, match="gv_set_ld_dosage"):
            sh.set_ld_dosage(2)
        sh.set_ld_dosage(1)
        for w in (0, 8193):
            with pytest.raises(capi.GvError, match="window must be in"):
                sh.ld_scores(w)
            with pytest.raises(capi.GvError, match="window must be in"):
                sh.ld_band(w, 0, 5)
        for j0, nj in ((-1, 5), (0, M + 1), (M, 1), (250, 7), (5, -1)):
            with pytest.raises(capi.GvError, match="outside the shard's markers"):
                sh.ld_band(10, j0, nj)
        with pytest.raises(capi.GvError, match="adjusted must be 0 or 1"):
            sh._ck(sh.L.gv_ld_scores(sh.h, 10, None, 2, capi._dp(np.zeros(M)), None))
    with capi.Shard(N, M, device=0) as sh:              # 16-bit codes
        sh.set_ld_dosage(1)
        sh.upload_dosage(synth.synth_dosage(N, M, 2, 16), 1.0 / 16384.0)
        with pytest.raises(capi.GvError, match="16-bit codes"):
            sh.ld_scores(10)
        with pytest.raises(capi.GvError, match="16-bit codes"):
            sh.ld_band(10, 0, 5)
    with capi.Shard(N, M, device=0) as sh:              # methylation data
        sh.set_ld_dosage(1)
        sh.synth_meth(3)
        sh.compute_markers_statistics()
        with pytest.raises(capi.GvError, match="meth"):
            sh.ld_scores(10)
    na = np.zeros(N)
    na[[3, 77]] = 1.0
    with _shard(codes, na) as sh:                       # the adjusted estimator divides by n - 2
        with pytest.raises(capi.GvError, match="at least 3 phenotyped"):
            sh.ld_scores(10, adjusted=True)
        sh.ld_scores(10)


def test_bed_data_ignore_the_option():
    N, M = 600, 256
    bed = synth.synth_bed(N, M, seed=1, miss_ppm=5000)
    outs = []
    for on in (0, 1):
        with capi.Shard(N, M, device=0) as sh:
            sh.set_ld_dosage(on)
            sh.upload_bed(bed)
            sh.compute_markers_statistics()
            outs.append(list(sh.ld_scores(50)) + [sh.ld_band(50, 0, M)])
    assert _same(*outs)


@pytest.mark.parametrize("case", ["masked", "missing"])
def test_the_context_is_left_as_it_was(case):
    N, M = 1003, 257
    codes, na, missing, _ = _case(N, M, case)
    rng = np.random.default_rng(1)
    x = rng.standard_normal(M)
    with _shard(codes, na, missing, on=False) as sh:
        sh.compute_markers_statistics()
        z = sh.Ax(x)
        w = sh.ATx(z)
        y = np.zeros(z.size)
        y[:N] = rng.standard_normal(N)
        dz, dy, dx = sh.vecN(z), sh.vecN(y), sh.vecM(x)
        loo = sh.assoc_calc(dz, dy, dx)
        sh.set_ld_dosage(1)
        sh.ld_scores(100)
        sh.ld_band(100, 10, 50)
        assert np.array_equal(sh.Ax(x), z) and np.array_equal(sh.ATx(z), w)
        again = sh.assoc_calc(dz, dy, dx)
        assert all(np.array_equal(loo[k], again[k], equal_nan=True) for k in loo)
