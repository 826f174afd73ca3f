"""gvamp_main_real --run-mode score on a toy .bed: N = 301 individuals x Mt = 703 markers, ~2 % missing genotypes,
a monomorphic and an all-missing marker.

* std units: <out>_scores.bin equals Shard.Ax of the columns scaled by sqrt(N), bit for bit;
* allele units: every entry is within a DERIVED tolerance of a dense score on mean-imputed allele counts computed in long double:
  the Ax bound of gvamp.h, M 2^-50 max|msig x| / sqrt(N) with msig x / sqrt(N) = w up to the two roundings of the conversion, plus
  gamma_M sum |mave_j w_j| for the constant, plus one rounding of the final sum;
* clumping and thresholding with three cut-offs equals the std run of the three masked columns bit for bit;
* the FATAL lines of a short score file and of inconsistent flags."""
import math
import os
import subprocess

import numpy as np
import pytest

import score_restatement as sr
from gvamp_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
N, MT, C = 301, 703, 5
MONO, ALLMISS = 17, 40
U = 2.0 ** -53


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    d = tmp_path_factory.mktemp("scoredrv")
    rng = np.random.default_rng(21)
    code = rng.choice(np.array([0, 2, 3, 1], dtype=np.uint8), size=(MT, N), p=[0.25, 0.48, 0.25, 0.02])      # PLINK: 1 = missing
    code[MONO] = 0
    code[ALLMISS] = 1
    pad = np.zeros((MT, 4 * ((N + 3) // 4)), dtype=np.uint8)
    pad[:, :N] = code
    rows = (pad.reshape(MT, -1, 4) << (2 * np.arange(4, dtype=np.uint8))).sum(axis=2).astype(np.uint8)
    bed = str(d / "toy.bed")
    with open(bed, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(rows.tobytes())
    W = rng.standard_normal((C, MT)) * 10.0 ** rng.integers(-3, 3, (C, 1))
    W[3] = 0.0
    return dict(dir=d, bed=bed, rows=rows, code=code, W=W)


def _run(toy, name, extra, wfile=None, cols=C):
    out = str(toy["dir"] / name) + "/"
    if wfile is None:
        wfile = str(toy["dir"] / "w.bin")
        toy["W"].tofile(wfile)
    cmd = [EXE, "--run-mode", "score", "--bed-file-test", toy["bed"], "--N-test", str(N), "--Mt-test", str(MT), "--out-dir", out,
           "--out-name", "t", "--score-file", wfile, "--score-cols", str(cols)] + extra
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    return res, out + "t_scores.bin"


def _shard(toy):
    sh = capi.Shard(N, MT)
    sh.upload_bed(toy["rows"])
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    for n in range(N):
        m4[n >> 2] |= 1 << (n & 3)
    sh.set_mask(m4, N)
    sh.compute_markers_statistics()
    return sh


def test_std_units_equal_the_one_vector_products(toy):
    res, path = _run(toy, "std", [])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    got = np.fromfile(path).reshape(C, N)
    with _shard(toy) as sh:
        for k in range(C):
            want = sh.Ax(toy["W"][k] * math.sqrt(N))[:N]
            assert np.array_equal(got[k].view(np.uint64), want.view(np.uint64)), k
    assert np.all(got[3] == 0.0) and np.any(got[0] != 0.0)
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("scores: ")]
    assert len(line) == 1 and "5 columns (std units) x 301 individuals" in line[0] and " passes, " in line[0]
    assert ("kernel path" in line[0]) or ("fallback path" in line[0])


def test_allele_units_within_the_derived_tolerance_of_a_dense_score(toy):
    res, path = _run(toy, "allele", ["--score-units", "allele"])
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    got = np.fromfile(path).reshape(C, N)
    with _shard(toy) as sh:
        mave, msig = sh.marker_stats()
    assert mave[MONO] == 2.0 and msig[MONO] == 1.0 and mave[ALLMISS] == 0.0 and msig[ALLMISS] == 1.0
    a = np.array([2.0, np.nan, 1.0, 0.0])[toy["code"]]
    a = np.where(np.isnan(a), mave[:, None], a).astype(np.longdouble)          # a missing genotype counts as the marker's mean
    gam = MT * U / (1 - MT * U)
    for k in range(C):
        w = toy["W"][k]
        want = (w.astype(np.longdouble)[:, None] * a).sum(axis=0)
        tol = MT * 2.0 ** -50 * np.max(np.abs(w)) * (1 + 4 * U) + gam * float(np.sum(np.abs(mave * w))) \
            + U * float(np.max(np.abs(want))) * (1 + 2.0 ** -40)
        err = float(np.max(np.abs(got[k].astype(np.longdouble) - want)))
        print("column %d: max error %.3e, tolerance %.3e" % (k, err, tol))
        assert err <= tol, (k, err, tol)
    assert np.all(got[3] == 0.0)
    # the constant alone at the monomorphic marker: a weight there moves every score by 2 w
    assert "allele units" in res.stdout


def test_thresholding_equals_the_std_run_of_the_masked_columns(toy):
    rng = np.random.default_rng(8)
    w0 = toy["W"][0]
    p = rng.random(MT) * 0.1
    idx = np.where(rng.random(MT) < 0.3, np.arange(MT), rng.integers(0, MT, MT)).astype(np.float64)
    idx[rng.random(MT) < 0.2] = -1.0
    idx[5], p[5] = 5.0, 0.01                            # a tie exactly at a cut-off is in
    idx[6], p[6] = 6.0, np.nextafter(0.01, 1.0)
    thr = [0.001, 0.01, 0.05]
    files = {n: str(toy["dir"] / n) for n in ("w0.bin", "p.bin", "idx.bin", "masked.bin")}
    w0.tofile(files["w0.bin"])
    p.tofile(files["p.bin"])
    idx.tofile(files["idx.bin"])
    masked = np.array(sr.threshold_columns(w0, idx.astype(np.int64), p, thr))
    assert masked[1][5] == w0[5] and masked[1][6] == 0.0 and masked[2][6] == w0[6]
    masked.tofile(files["masked.bin"])
    res, path = _run(toy, "ct", ["--score-clump-index", files["idx.bin"], "--score-p-file", files["p.bin"], "--score-p-thresholds",
                                 "0.001,0.01,0.05"], wfile=files["w0.bin"], cols=1)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    ref, rpath = _run(toy, "ctref", [], wfile=files["masked.bin"], cols=3)
    assert ref.returncode == 0, ref.stdout[-3000:] + ref.stderr[-3000:]
    got, want = np.fromfile(path), np.fromfile(rpath)
    assert got.size == 3 * N and np.array_equal(got.view(np.uint64), want.view(np.uint64)) and np.any(got != 0)


def test_fatal_lines(toy):
    short = str(toy["dir"] / "short.bin")
    toy["W"][:, :-1].tofile(short)
    res, _ = _run(toy, "f1", [], wfile=short)
    assert res.returncode != 0 and "FATAL: the score file" in res.stdout
    assert "holds %d bytes, fewer than the %d of %d float64 values" % (8 * C * (MT - 1), 8 * C * MT, C * MT) in res.stdout
    res, _ = _run(toy, "f2", ["--score-p-thresholds", "0.01"])
    assert res.returncode != 0 and "--score-clump-index, --score-p-file and --score-p-thresholds go together" in res.stdout
    files = [str(toy["dir"] / n) for n in ("p.bin", "idx.bin")]
    np.zeros(MT).tofile(files[0])
    np.arange(MT, dtype=np.float64).tofile(files[1])
    res, _ = _run(toy, "f3", ["--score-clump-index", files[1], "--score-p-file", files[0], "--score-p-thresholds", "0.01"])
    assert res.returncode != 0 and "it needs --score-cols 1, not 5" in res.stdout
    res, _ = _run(toy, "f4", ["--score-units", "grams"])
    assert res.returncode != 0 and "--score-units has to be std or allele" in res.stdout
    cmd = [EXE, "--run-mode", "score", "--bed-file-test", toy["bed"], "--N-test", str(N), "--Mt-test", str(MT)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "--run-mode score needs --score-file" in res.stdout
