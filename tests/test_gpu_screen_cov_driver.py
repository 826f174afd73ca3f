"""gvamp_main_real --run-mode screen --cov-file F --C K: the loop king -> pca -> screen(cov) closed on the
command line, on the `four` shape of tests/pca_restatement.py (five populations).  --run-mode pca --pca-k 3 writes its eigenvector file;
the screen reads it as covariates and writes <out>_screen_{r,t,p,beta,se}.bin, which equal capi.Shard.screen_cov on the same inputs bit for bit: masking, centring and every later
step run on the device in both routes, and the text file carries the eigenvectors with 17 significant digits.  One covariate entry is
made non-finite: that individual is masked together with the NA phenotypes (complete cases).  A run without --cov-file writes exactly
the three files of section 23."""
import os
import subprocess

import numpy as np
import pytest

import pca_restatement as pr
from gvamp_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
NAMES = ("r", "t", "p", "beta", "se")


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    for k in ("GV_ATXM_COLS", "GV_ATXM_KS", "GV_ATXM_KERNEL"):
        monkeypatch.delenv(k, raising=False)


def _run(args):
    res = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


def test_pca_then_the_adjusted_screen_equals_the_python_result(tmp_path):
    cs = pr.case("four")
    N, M = cs["N"], cs["M"]
    mb = (N + 3) // 4
    rng = np.random.default_rng(19)
    pop = np.arange(N) % 5                                           # the populations, dealt in turn: a confounder the components carry
    Y = rng.standard_normal((3, N)) * np.array([[1.0], [30.0], [1e-2]]) + np.array([0.0, 1.0, -0.5, 2.0, 0.3])[pop] * np.array([[1.0], [20.0], [0.0]])
    Y[0] += 0.2 * np.where(cs["a"][23] < 0, 1.0, cs["a"][23])
    Y[:, ~cs["present"]] = np.nan
    bed = str(tmp_path / "toy.bed")
    with open(bed, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(np.asarray(cs["bed"], dtype=np.uint8).reshape(M, mb).tobytes())
    files = []
    for k, y in enumerate(Y):
        path = str(tmp_path / ("p%d.phen" % k))
        with open(path, "w") as f:
            for n in range(N):
                f.write("f%d i%d %s\n" % (n, n, "NA" if np.isnan(y[n]) else repr(float(y[n]))))
        files.append(path)
    out = str(tmp_path / "out") + "/"
    os.makedirs(out, exist_ok=True)
    common = ["--bed-file", bed, "--N", str(N), "--Mt", str(M), "--out-dir", out]
    _run(["--run-mode", "pca", "--pca-k", "3", "--pca-block", "12", "--pca-tol", "1e-6", "--phen-files", files[0], "--out-name", "pc"] + common)
    evec = out + "pc_pca_eigenvec.txt"
    Cov = np.loadtxt(evec).T.copy()
    assert Cov.shape == (3, N)
    # one individual with a phenotype loses a covariate: the screen masks it
    gone = int(np.nonzero(cs["present"])[0][5])
    lines = open(evec).read().splitlines()
    lines[gone] = "nan " + lines[gone].split(" ", 1)[1]
    cov_file = str(tmp_path / "cov.txt")
    with open(cov_file, "w") as f:
        f.write("\n".join(lines) + "\n")
    Cov[0, gone] = np.nan
    stdout = _run(["--run-mode", "screen", "--phen-files", ",".join(files), "--cov-file", cov_file, "--C", "3", "--screen-cols", "2",
                   "--out-name", "adj"] + common)
    merged = cs["present"].copy()
    merged[gone] = False
    assert "adjusted for 3 covariates, %d complete cases" % int(merged.sum()) in stdout
    m4 = np.zeros(mb, dtype=np.uint8)
    idx = np.nonzero(merged)[0]
    np.bitwise_or.at(m4, idx >> 2, (1 << (idx & 3)).astype(np.uint8))
    with capi.Shard(N, M) as sh:
        sh.set_layout(False, 2)
        sh.upload_bed(cs["bed"])
        sh.set_mask(m4, int(merged.sum()))
        sh.compute_markers_statistics()
        want = sh.screen_cov(Y, Cov)
    assert sorted(os.listdir(out)) == sorted(["pc_pca_eigenval.txt", "pc_pca_eigenvec.txt", "pc_pca_loadings.bin"] +
                                             ["adj_screen_%s.bin" % k for k in NAMES])
    for k in NAMES:
        got = np.fromfile(out + "adj_screen_%s.bin" % k).reshape(3, M)
        assert np.array_equal(got.view(np.uint64), want[k].view(np.uint64)), k
        assert np.all(np.isfinite(got[:, 23])), k
    # without --cov-file: the three files of the marginal screen and nothing else
    plain = str(tmp_path / "plain") + "/"
    os.makedirs(plain, exist_ok=True)
    stdout = _run(["--run-mode", "screen", "--phen-files", ",".join(files), "--out-name", "t", "--bed-file", bed, "--N", str(N), "--Mt", str(M),
                   "--out-dir", plain])
    assert "screen: 3 phenotypes x %d markers, %d complete cases" % (M, cs["nonas"]) in stdout
    assert sorted(os.listdir(plain)) == ["t_screen_p.bin", "t_screen_r.bin", "t_screen_t.bin"]
    with capi.Shard(N, M) as sh:
        sh.set_layout(False, 2)
        sh.upload_bed(cs["bed"])
        sh.set_mask(cs["m4"], cs["nonas"])
        sh.compute_markers_statistics()
        marg = sh.screen(Y)
    for k, tag in enumerate("rtp"):
        got = np.fromfile(plain + "t_screen_%s.bin" % tag).reshape(3, M)
        ok = ~np.isnan(marg[k])
        assert np.array_equal(np.isnan(got), ~ok), tag
        scale = np.abs(marg[k][ok]) + (0.0 if tag == "p" else 1.0)
        assert np.all(np.abs(got[ok] - marg[k][ok]) <= 1e-12 * scale), tag
