"""gvamp_main_real --run-mode pca on the `ragged` shape of tests/pca_restatement.py written to a temporary
.bed / .phen: N = 1003 individuals x Mt = 517 markers, 5 % missing genotypes, 3 % NA phenotypes, a monomorphic and an all-missing marker.

* the three files have the stated shapes, and <out>_pca_eigenvec.txt parses as a covariates file of K columns; a run that misses the
  tolerance writes nothing and exits non-zero unless --pca-allow-unconverged 1;
* the eigenpairs hold the residual promise against the restatement's dense G and the Davis-Kahan / Kato-Temple bounds against its eigh,
  with r_i the residual norm formed outside; and each eigenvector is within (r_i + r'_i) / delta_i + 2 N eps of the restatement's,
  run from the same starting block (data::pca_start restated below), r'_i the restatement's residual: both lie within their own
  Davis-Kahan angle of the same exact eigenvector;
* the loadings file as --score-file of --run-mode score on the same cohort.  The score run knows no phenotype, so this part runs both
  modes on a .phen without NA.  With v_i = c_i (A^T u_i + e1), c_i = sqrt(N / M) / sqrt(theta_i), and std units scaling a column by
  sqrt(N), the score is z_i = sqrt(N) A v_i + e2 = sqrt(M) (sqrt(theta_i) u_i + (G u_i - theta_i u_i) / sqrt(theta_i)) + ..., so
      |z_i / sqrt(M) - sqrt(theta_i) u_i|_max <= tol sqrt(theta_i)                                   (r_i <= tol theta_i: converged)
            + N / (M sqrt(theta_i)) * ||A||_2 * sqrt(M) * N 2^-50 max msig max|u_i| / sqrt(N)       (e1, the ATx bound of gvamp.h, in 2-norm)
            + M 2^-50 max_j |msig_j x_j| / sqrt(N) / sqrt(M)                                         (e2, the Ax bound, x = sqrt(N) v_i)
            + 8 * 2^-53 sqrt(theta_i) max|u_i|                                                       (the roundings of c_i, v_i, x)
  with ||A||_2 = sqrt(theta_1 M / N)."""
import os
import subprocess

import numpy as np
import pytest

import pca_restatement as pr
from gvamp_amd import capi

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
K, L, TOL, SEED = 2, 10, 1e-9, 5


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")


def _mix(z):
    with np.errstate(over="ignore"):
        z = z + np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def pca_start(seed, L_, N):
    """the starting block of data::pca: Box-Muller on two splitmix64 outputs per entry"""
    with np.errstate(over="ignore"):
        base = _mix(np.uint64(seed))
        idx = np.arange(L_ * N, dtype=np.uint64)
        u1 = ((_mix(base + np.uint64(2) * idx) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
        u2 = ((_mix(base + np.uint64(2) * idx + np.uint64(1)) >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    return (np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)).reshape(L_, N)


def _write(d, cs, present):
    bed, phen = str(d / "g.bed"), str(d / ("all.phen" if present.all() else "na.phen"))
    if not os.path.exists(bed):
        with open(bed, "wb") as f:
            f.write(bytes([0x6C, 0x1B, 0x01]))
            f.write(cs["bed"].tobytes())
    y = np.random.default_rng(3).standard_normal(cs["N"])
    with open(phen, "w") as f:
        for n in range(cs["N"]):
            f.write("f%d i%d %s\n" % (n, n, ("%.6f" % y[n]) if present[n] else "NA"))
    return bed, phen


def _pca(d, cs, present, name):
    bed, phen = _write(d, cs, present)
    out = str(d / name) + "/"
    os.makedirs(out, exist_ok=True)
    cmd = [EXE, "--run-mode", "pca", "--bed-file", bed, "--phen-files", phen, "--N", str(cs["N"]), "--Mt", str(cs["M"]), "--out-dir", out,
           "--out-name", "t", "--pca-k", str(K), "--pca-block", str(L), "--pca-tol", str(TOL), "--pca-seed", str(SEED)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    ev = np.loadtxt(out + "t_pca_eigenval.txt", ndmin=1)
    rows = [ln.split() for ln in open(out + "t_pca_eigenvec.txt").read().splitlines()]
    assert len(rows) == cs["N"] and all(len(r) == K for r in rows)                # what read_covariates parses: N lines of K tokens
    U = np.array(rows, dtype=np.float64)
    V = np.fromfile(out + "t_pca_loadings.bin")
    assert ev.shape == (K,) and V.size == K * cs["M"]
    line = [ln for ln in res.stdout.splitlines() if ln.startswith("pca: ")]
    assert len(line) == 1 and "converged" in line[0] and "NOT converged" not in line[0], res.stdout[-2000:]
    return dict(eval=ev, U=U, V=V.reshape(K, cs["M"]), out=out, bed=bed, stdout=res.stdout)


def test_the_three_files_and_the_eigenpairs(tmp_path):
    cs = pr.case("ragged")
    N = cs["N"]
    got = _pca(tmp_path, cs, cs["present"], "na")
    _, G = pr.dense_G(cs)
    lam, E = pr.eigh(cs)
    th, U = got["eval"], got["U"]
    r = np.sqrt((((G @ U) - U * th[None, :]) ** 2).sum(axis=0))
    assert np.all(r <= 1.01 * TOL * th), (r, TOL * th)
    delta = pr.gaps(th, lam)
    ref = pr.iterate(cs, TOL, 100, q0=pca_start(SEED, L, N), k=K)
    for i in range(K):
        e = E[:, i]
        s_exact = np.linalg.norm(U[:, i] - e * (e @ U[:, i]))
        w = ref["U"][:, i]
        s_ref = np.linalg.norm(U[:, i] - w * (w @ U[:, i]))
        print(i, th[i], r[i], s_exact, s_ref, delta[i])
        assert s_exact <= r[i] / delta[i] + N * pr.EPS
        assert s_ref <= (r[i] + ref["resid"][i]) / delta[i] + 2 * N * pr.EPS
        assert float(w @ U[:, i]) > 0                                             # the same sign rule
        assert abs(th[i] - lam[i]) <= r[i] ** 2 / delta[i] + N * pr.EPS * lam[0]
    assert np.all(U[~cs["present"]] == 0) and np.array_equal(pr.sign_rule(U), U) and th[0] >= th[1]
    assert np.max(np.abs(U.T @ U - np.eye(K))) <= N * pr.EPS
    for bad, msg in ((["--pca-k", "0"], "strictly positive"), (["--pca-k", "4", "--pca-block", "3"], "FATAL: --run-mode pca: the block")):
        cmd = [EXE, "--run-mode", "pca", "--bed-file", got["bed"], "--phen-files", str(tmp_path / "na.phen"), "--N", str(N), "--Mt",
               str(cs["M"]), "--out-dir", got["out"], "--out-name", "bad"] + bad
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
        assert res.returncode != 0 and msg in res.stdout + res.stderr, res.stdout[-2000:]
    # a run that misses the tolerance writes nothing and fails, unless it is allowed to
    base = [EXE, "--run-mode", "pca", "--bed-file", got["bed"], "--phen-files", str(tmp_path / "na.phen"), "--N", str(N), "--Mt", str(cs["M"]),
            "--out-dir", got["out"], "--pca-k", str(K), "--pca-block", str(L), "--pca-tol", str(TOL), "--pca-max-iter", "1"]
    res = subprocess.run(base + ["--out-name", "short"], capture_output=True, text=True, timeout=300)
    assert res.returncode != 0 and "FATAL: --run-mode pca: NOT converged after 1 iterations" in res.stdout, res.stdout[-2000:]
    assert not any(f.startswith("short_pca") for f in os.listdir(got["out"]))
    res = subprocess.run(base + ["--out-name", "loose", "--pca-allow-unconverged", "1"], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "WARNING: --run-mode pca: NOT converged after 1 iterations" in res.stdout, res.stdout[-2000:]
    assert all(os.path.exists(got["out"] + "loose_pca_" + f) for f in ("eigenval.txt", "eigenvec.txt", "loadings.bin"))


def test_the_loadings_file_scores_the_cohort_back_to_its_components(tmp_path):
    cs = pr.case("ragged")
    N, M = cs["N"], cs["M"]
    got = _pca(tmp_path, cs, np.ones(N, dtype=bool), "all")
    cmd = [EXE, "--run-mode", "score", "--bed-file-test", got["bed"], "--N-test", str(N), "--Mt-test", str(M), "--out-dir", got["out"],
           "--out-name", "t", "--score-file", got["out"] + "t_pca_loadings.bin", "--score-cols", str(K)]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    Z = np.fromfile(got["out"] + "t_scores.bin").reshape(K, N)
    with capi.Shard(N, M) as sh:
        sh.upload_bed(cs["bed"])
        sh.set_mask(pr.mask4(np.ones(N, dtype=bool)), N)
        sh.compute_markers_statistics()
        _, msig = sh.marker_stats()
    th, U = got["eval"], got["U"]
    normA = np.sqrt(th[0] * (1 + 1e-6) * M / N)
    for i in range(K):
        u, x = U[:, i], np.sqrt(float(N)) * got["V"][i]
        bound = TOL * np.sqrt(th[i]) \
            + N / (M * np.sqrt(th[i])) * normA * np.sqrt(M) * N * 2.0 ** -50 * msig.max() * np.abs(u).max() / np.sqrt(N) \
            + M * 2.0 ** -50 * np.max(np.abs(msig * x)) / np.sqrt(N) / np.sqrt(M) \
            + 8 * 2.0 ** -53 * np.sqrt(th[i]) * np.abs(u).max()
        err = float(np.max(np.abs(Z[i] / np.sqrt(M) - np.sqrt(th[i]) * u)))
        print("component %d: max error %.3e, bound %.3e" % (i, err, bound))
        assert err <= bound, (i, err, bound)
