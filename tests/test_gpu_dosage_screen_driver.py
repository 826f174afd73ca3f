"""gvamp_main_real --run-mode screen --geno-format dosage8 --screen-dosage 1, with and without --cov-file and
--dosage-kernels mfma, on 300 individuals x 200 markers: the files <out>_screen_{r,t,p}.bin, or the five of the adjusted screen, equal
capi.Shard.screen / screen_cov on the same inputs bit for bit.  The adjusted screen masks, centres and residualises on the device in
both routes.  The marginal screen prepares its columns on the host, the driver by running sums and the Python layer by numpy's pairwise
ones: the phenotypes here are small integers over 256 complete cases, so every sum of either preparation is exact (the mean is a
multiple of 2^-8, the squares are multiples of 2^-16 below 2^53 of them) and the two prepare the same bits.  Without the flag the
driver's FATAL line is the one it was."""
import os
import subprocess

import numpy as np
import pytest

from gvamp_amd import capi, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
NAMES = ("r", "t", "p", "beta", "se")
N, M = 300, 200


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    for k in ("GV_ATXM_COLS", "GV_ATXM_KS", "GV_ATXM_KERNEL", "GV_ATXM_TILES", "GV_DOSAGE_MFMA_SEG", "GV_DOSAGE_NA_KERNELS"):
        monkeypatch.delenv(k, raising=False)


def _run(args, ok=True):
    res = subprocess.run([EXE] + args, capture_output=True, text=True, timeout=300)
    assert (res.returncode == 0) == ok, res.stdout[-3000:] + res.stderr[-3000:]
    return res.stdout


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("dosage_screen")
    rng = np.random.default_rng(31)
    B = synth.synth_dosage(N, M, 7, 8)
    B[13] = 55                                                       # a constant marker: NaN in every file
    codes = str(d / "toy.codes")
    B.tofile(codes)
    present = np.ones(N, dtype=bool)
    present[rng.choice(N, N - 256, replace=False)] = False           # 256 complete cases
    Y = rng.integers(-40, 41, size=(3, N)).astype(np.float64)
    Y[1] += np.rint(B[5] / 4.0)                                      # an associated marker; still small integers
    Y[:, ~present] = np.nan
    files = []
    for k, y in enumerate(Y):
        path = str(d / ("p%d.phen" % k))
        with open(path, "w") as f:
            for n in range(N):
                f.write("f%d i%d %s\n" % (n, n, "NA" if np.isnan(y[n]) else repr(float(y[n]))))
        files.append(path)
    Cov = np.stack([rng.standard_normal(N), 55.0 + 8.0 * rng.standard_normal(N)])
    cov_file = str(d / "cov.txt")
    with open(cov_file, "w") as f:
        for n in range(N):
            f.write(" ".join(repr(float(c)) for c in Cov[:, n]) + "\n")
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    idx = np.nonzero(present)[0]
    np.bitwise_or.at(m4, idx >> 2, (1 << (idx & 3)).astype(np.uint8))
    return dict(dir=d, B=B, codes=codes, files=files, cov_file=cov_file, Y=Y, Cov=Cov, m4=m4, nonas=256)


def _shard(inp, route):
    sh = capi.Shard(N, M)
    sh.set_dosage_route(route)
    sh.upload_dosage(inp["B"], 1.0 / 127.0)
    sh.set_mask(inp["m4"], inp["nonas"])
    sh.compute_markers_statistics()
    sh.set_screen_dosage(1)
    assert sh.dosage_route() == (route, route)
    return sh


@pytest.mark.parametrize("kernels", ["valu", "mfma"])
def test_the_files_equal_the_python_results_bit_for_bit(inputs, kernels, tmp_path):
    route = 1 if kernels == "mfma" else 0
    out = str(tmp_path / "out") + "/"
    os.makedirs(out, exist_ok=True)
    common = ["--run-mode", "screen", "--geno-format", "dosage8", "--screen-dosage", "1", "--dosage-kernels", kernels, "--bed-file", inputs["codes"],
              "--N", str(N), "--Mt", str(M), "--phen-files", ",".join(inputs["files"]), "--out-dir", out]
    plain = _run(common + ["--out-name", "m"])
    assert ("fixed-point i8 MFMA route" if route else "fp64 VALU kernels") in plain
    stdout = _run(common + ["--out-name", "a", "--cov-file", inputs["cov_file"], "--C", "2", "--screen-cols", "2"])
    assert "adjusted for 2 covariates, 256 complete cases" in stdout
    assert sorted(os.listdir(out)) == sorted(["m_screen_%s.bin" % k for k in "rtp"] + ["a_screen_%s.bin" % k for k in NAMES])
    with _shard(inputs, route) as sh:
        marg = sh.screen(inputs["Y"])
        assert "screen: 3 phenotypes x %d markers, 256 complete cases of %d, %s path" % (M, N, sh.atxm_info()["path"]) in plain
        adj = sh.screen_cov(inputs["Y"], inputs["Cov"])
    for k, tag in enumerate("rtp"):
        got = np.fromfile(out + "m_screen_%s.bin" % tag).reshape(3, M)
        assert np.array_equal(got.view(np.uint64), marg[k].view(np.uint64)), tag
        assert np.all(np.isnan(got[:, 13])) and np.isfinite(got).sum() == 3 * (M - 1), tag
    for name in NAMES:
        got = np.fromfile(out + "a_screen_%s.bin" % name).reshape(3, M)
        assert np.array_equal(got.view(np.uint64), adj[name].view(np.uint64)), name
        assert np.all(np.isnan(got[:, 13])) and np.isfinite(got).sum() == 3 * (M - 1), name
    assert abs(marg[1][1, 5]) > 5.0                                  # (the associated marker shows)


def test_without_the_flag_the_fatal_line_stays_and_bed_data_ignore_it_with_a_warning(inputs, tmp_path):
    out = str(tmp_path / "o") + "/"
    os.makedirs(out, exist_ok=True)
    base = ["--run-mode", "screen", "--bed-file", inputs["codes"], "--N", str(N), "--Mt", str(M), "--phen-files", ",".join(inputs["files"]),
            "--out-dir", out, "--out-name", "x"]
    stdout = _run(base + ["--geno-format", "dosage8"], ok=False)
    assert "FATAL: --run-mode screen works on 2-bit genotypes only, not on --geno-format dosage8\n" in stdout
    assert os.listdir(out) == []
    bed = str(tmp_path / "toy.bed")
    with open(bed, "wb") as f:
        f.write(bytes([0x6C, 0x1B, 0x01]))
        f.write(synth.synth_bed(N, M, seed=3).tobytes())
    stdout = _run(base[:2] + ["--bed-file", bed] + base[4:] + ["--screen-dosage", "1"])
    assert stdout.count("WARNING: --screen-dosage is ignored for --geno-format bed") == 1
    assert sorted(os.listdir(out)) == ["x_screen_p.bin", "x_screen_r.bin", "x_screen_t.bin"]
