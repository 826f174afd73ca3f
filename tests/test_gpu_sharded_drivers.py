"""The sharded DRIVER path on one GPU: gvamp_sim / gvamp_main_real started as N processes by scripts/run_sharded.py --comm host
--same-gpu -- every rank its own divide_work shard (utilities.cpp:259-291), its own slab of the .bed (file offset 3 + S*mbytes,
data.cpp:215), its own Hutchinson probe (seed + S, vamp.cpp:875), its own writes into the shared .bin files at byte offset S*8
(utilities.cpp:293-301), text files by rank 0 only -- with the sums of data.cpp:928/:995 and utilities.cpp:203 carried by the
shared-memory host transport (host/shm_comm.cpp) instead of RCCL, which needs one GPU per rank.  The files the ranks wrote are
compared with what the REAL reference wrote under `mpirun -np 2` (tests/golden/survey_probe) and with the oracle's sharded runs.
The second half of the file runs the batch products -- --run-mode screen, pca, screen --cov-file and score -- as two and three
processes against the same command on one rank.

(The GPU boxes of this pool allow six processes on the card at once, the test runner included: five ranks at most here; the
reference's np = 8 outputs are covered by the in-process shards of tests/test_gpu_vamp.py.)"""
import lzma
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import bed_fixed_restatement as bx
import pca_restatement as pr
import sharded_products as sp
from gvamp_amd import capi, synth
from test_gpu_pca_driver import pca_start

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "survey_probe")
SIM = os.path.join(ROOT, "gvamp_amd", "gvamp_sim")
REAL = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
TIGHT = 1e-7


def rel(a, b):
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.0)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def sharded(n, exe, args, timeout=900, no_fatal=False):
    """no_fatal: the first line of the job's stdout that says FATAL fails the test with that line, whatever the exit code"""
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "run_sharded.py"), "-n", str(n), "--comm", "host", "--same-gpu",
           "--master-port", str(_free_port()), "--", exe] + [str(a) for a in args]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    if no_fatal:
        fatal = [ln for ln in r.stdout.splitlines() if "FATAL" in ln]
        assert not fatal, fatal[0]
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _toy_bed(tmp_path):
    p = tmp_path / "toy.bed"
    p.write_bytes(lzma.open(os.path.join(G, "toy.bed.xz")).read())
    return str(p)


SIM_ARGS = ["--N", "2000", "--Mt", "10000", "--out-name", "toy", "--iterations", "3", "--num-mix-comp", "3", "--probs",
            "0.90,0.07,0.03", "--vars", "0,0.001,0.01", "--CV", "500", "--h2", "0.5", "--rho", "0.5", "--CG-max-iter", "20",
            "--model", "linear", "--seed", "7", "--store-pvals", "0"]


@pytest.mark.parametrize("kmode,fuse", [(1, 4), (1, 0), (1, 2), (0, 1)])
def test_gvamp_sim_two_processes_vs_real_reference_np2(tmp_path, kmode, fuse):
    """The reference's own command line under `mpirun -np 2`, here as two processes sharing GPU 0: the .bin files assembled by the
    two ranks (each wrote its M doubles at byte offset S*8) against the reference's, the rank-0 text files likewise."""
    bed = _toy_bed(tmp_path)
    out = str(tmp_path / "out") + "/"
    os.makedirs(out)
    stdout = sharded(2, SIM, ["--bed-file", bed, "--out-dir", out, "--kernel-mode", kmode, "--fuse-solves", fuse] + SIM_ARGS)
    assert "rank    0 has 5000 markers" in stdout.replace("INFO   : ", "")
    assert np.array_equal(np.fromfile(out + "toy_beta_true.bin"), np.fromfile(os.path.join(G, "sim_beta_true.bin")))
    for name in ("it_1_x2_hat", "it_3", "it_3_x2_hat", "r1_it_3"):
        mine = np.fromfile(out + "toy_%s.bin" % name)
        assert mine.size == 10000
        assert rel(mine, np.fromfile(os.path.join(G, "sim_np2_%s.bin" % name))) < TIGHT, name
    assert np.allclose(np.loadtxt(out + "toy_gam1s.csv"), np.loadtxt(os.path.join(G, "sim_np2_gam1s.csv")), rtol=1e-5)
    assert np.allclose(np.loadtxt(out + "toy_gam2s.csv"), np.loadtxt(os.path.join(G, "sim_np2_gam2s.csv")), rtol=1e-5)
    assert np.loadtxt(out + "toy_z1_it_2.csv").size == 2000            # one writer: a second one would interleave lines


@pytest.mark.parametrize("n", [3, 5])
def test_gvamp_sim_uneven_shards_vs_oracle(tmp_path, oracle, n):
    """Mt = 10000 over 3 ranks (3334 / 3333 / 3333: the remainder goes to the low ranks) and over 5: every rank's slab offset,
    probe seed and file offset differ; the assembled iterates against the oracle's run with the same shards."""
    bed = _toy_bed(tmp_path)
    out = str(tmp_path / "out") + "/"
    os.makedirs(out)
    sharded(n, SIM, ["--bed-file", bed, "--out-dir", out] + SIM_ARGS)
    raw = np.frombuffer(lzma.open(os.path.join(G, "toy.bed.xz")).read(), dtype=np.uint8)[3:]
    beta, y = oracle.sim_phen(raw, 2000, 10000, 0.5, 500, 7)
    ref = oracle.infere(raw, 2000, 10000, y, [0.90, 0.07, 0.03], [0, 0.001, 0.01], nshards=n, iterations=3, CG_max_iter=20,
                        rho=0.5, seed=7, gam1=1e-8, gamw=2.0, true_signal=beta)
    assert np.array_equal(np.fromfile(out + "toy_beta_true.bin"), beta)
    for k in (1, 2, 3):
        assert rel(np.fromfile(out + "toy_it_%d.bin" % k), ref.x1[k - 1]) < TIGHT, k
        assert rel(np.fromfile(out + "toy_it_%d_x2_hat.bin" % k), ref.x2[k - 1]) < TIGHT, k


N, NT, M = 600, 301, 901           # 901 markers: uneven over 2 and over 3 ranks
PROBS, VARS = "0.9,0.1", "0,0.01"


def read_phen_scaled(path):
    """data::read_phen (data.cpp:128-192)"""
    raw, na = [], []
    for line in open(path):
        t = line.split()
        na.append(t[2] == "NA")
        raw.append(0.0 if t[2] == "NA" else float(t[2]))
    raw, na = np.array(raw), np.array(na)
    avg = raw[~na].mean()
    sqn = np.sqrt((np.sum(~na) - 1) / np.sum((raw[~na] - avg) ** 2))
    return raw, raw * sqn, na, avg, sqn


@pytest.fixture(scope="module")
def world(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("sharded_modes")
    rng = np.random.default_rng(5)
    bed = synth.synth_bed(N, M, seed=311, miss_ppm=5000)
    bed_t = synth.synth_bed(NT, M, seed=312, miss_ppm=5000)
    synth.write_bed(str(d / "tr.bed"), bed)
    synth.write_bed(str(d / "te.bed"), bed_t)
    beta = rng.standard_normal(M) * (rng.random(M) < 0.05) * 0.15
    for name, b, n in (("tr", bed, N), ("te", bed_t, NT)):
        mave, msig = oracle.marker_stats(b, n, M)
        g = oracle.ax(b, n, M, mave, msig, beta * np.sqrt(n))[:n]
        y = 1.5 + 2.0 * (g + 0.7 * rng.standard_normal(n))
        with open(d / (name + ".phen"), "w") as f:
            for i in range(n):
                f.write("F%d I%d %s\n" % (i, i, "NA" if (name == "tr" and i % 97 == 5) else repr(float(y[i]))))
    out = str(d / "out") + "/"
    os.makedirs(out)
    base = ["--bed-file", d / "tr.bed", "--phen-files", d / "tr.phen", "--N", N, "--Mt", M, "--out-dir", out, "--probs",
            PROBS, "--vars", VARS, "--rho", "0.5", "--CG-max-iter", "20", "--seed", "4"]
    return dict(d=d, out=out, bed=bed, bed_t=bed_t, base=base)


def oracle_test_r2(oracle, w, x_est, intercept=0.0, scale=1.0):
    _, yt, na, _, _ = read_phen_scaled(w["d"] / "te.phen")
    mave, msig = oracle.marker_stats(w["bed_t"], NT, M)
    z = oracle.ax(w["bed_t"], NT, M, mave, msig, x_est * np.sqrt(NT))[:NT]
    err2 = np.sum((yt - (intercept + scale * z)) ** 2)
    sd2 = (np.sum(yt ** 2) - NT * yt.mean() ** 2) / (NT - 1)
    return 1 - err2 / (sd2 * NT), err2


def test_main_real_both_as_two_processes(world, oracle):
    """--run-mode both (main_real.cpp:214-283) sharded: TWO data objects per process -- the training shard, then the test shard --
    on the process's ONE communicator (host/data.cpp: gv_host_world); NA phenotypes, ragged N_test; the iterate the two ranks
    assembled against the oracle's 2-shard run, the printed test R2 against the oracle evaluated on that file."""
    w = world
    out = sharded(2, REAL, ["--run-mode", "both", "--out-name", "b", "--iterations", "3", "--bed-file-test", w["d"] / "te.bed",
                            "--phen-files-test", w["d"] / "te.phen", "--N-test", NT, "--Mt-test", M] + w["base"])
    raw, _, na, avg, sqn = read_phen_scaled(w["d"] / "tr.phen")
    ref = oracle.infere(w["bed"], N, M, raw, [0.9, 0.1], [0, 0.01], CG_max_iter=20, rho=0.5, seed=4, iterations=3,
                        is_na=na.astype(np.uint8), nshards=2, gam1=1e-6, gamw=2.0)
    x = np.fromfile(w["out"] + "b_it_3.bin")
    assert x.size == M and rel(x, ref.x1[2]) < TIGHT
    assert np.isclose(float(re.search(r"intercept = ([-0-9.e+]+)", out).group(1)), avg, rtol=1e-5)
    o_r2, _ = oracle_test_r2(oracle, w, x, intercept=avg, scale=sqn)
    assert np.isclose(float(re.search(r"test R2 = ([-0-9.e+]+)", out).group(1)), o_r2, rtol=1e-5, atol=1e-8)


def test_main_real_test_mode_as_three_processes(world, oracle):
    """--run-mode test (main_real.cpp:129-211) over three ranks: each reads its own slice of the estimate file (offset S*8) and its
    own slab of the test .bed; the predictor is summed over the ranks inside Ax; R2 over an iteration range and for one file."""
    w = world
    if not os.path.exists(w["out"] + "b_it_3.bin"):
        pytest.skip("needs the iterates of test_main_real_both_as_two_processes")
    targs = ["--bed-file-test", w["d"] / "te.bed", "--phen-files-test", w["d"] / "te.phen", "--N-test", NT, "--Mt-test", M]
    out = sharded(3, REAL, ["--run-mode", "test", "--estimate-file", w["out"] + "b_it_3.bin"] + targs)
    o_r2, o_err2 = oracle_test_r2(oracle, w, np.fromfile(w["out"] + "b_it_3.bin"))
    assert np.isclose(float(re.search(r"test R2 = ([-0-9.e+]+)", out).group(1)), o_r2, rtol=1e-5)
    assert np.isclose(float(re.search(r"test l2 pred err\^2 = ([-0-9.e+]+)", out).group(1)), o_err2, rtol=1e-5)
    out = sharded(3, REAL, ["--run-mode", "test", "--estimate-file", w["out"] + "b_it_1.bin", "--test-iter-range", "1,3"] + targs)
    vals = [float(v) for v in re.search(r"\n([-0-9.e+, ]+), \n", out).group(1).split(", ")]
    ref = [oracle_test_r2(oracle, w, np.fromfile(w["out"] + "b_it_%d.bin" % k))[0] for k in (1, 2, 3)]
    assert np.allclose(vals, ref, rtol=1e-4, atol=1e-6)


# ---- the batch products as sharded jobs: --run-mode screen | pca | screen --cov-file | score (DESIGN.md sections 21, 23, 24, 26) ----------
# Two and three ranks on the toy data (N = 2000, Mt = 10000: shards of 5000 + 5000 and of 3334 + 3333 + 3333 markers), each run against the
# same command on ONE rank written to another --out-dir.  Per-marker files (screen, adjusted screen) are byte-identical: every column of
# every rank lands at value offset c * Mt + S.  N-space results (scores, eigenvectors) are sums over the ranks: the scores are held to a
# dense long-double score under the rule of section 15 (16 x the deviation of the float64 form, never less than 1e-12; the deviation of a
# column is max |dz| / max |z|, tests/sharded_products.py), the eigenpairs to the checks of tests/test_gpu_pca_driver.py.
#
# The toy genotypes are independent draws: the spectrum of G is a Marchenko-Pastur bulk (lam_1 = 2.087, lam_4 = 2.066, lam_33 = 1.96),
# the subspace iteration contracts by lam_33 / lam_4 = 0.949 an iteration at the widest block, and the restatement needs 108 iterations for
# 1e-4 (277 with a block of 12).  Hence --pca-block 32 --pca-tol 1e-4 --pca-max-iter 200; every check scales with the tolerance.
_TOY = {}                                              # what the two rank counts share of the restatement: computed once, never changed
TN, TMT = 2000, 10000
PCA_K, PCA_L, PCA_TOL, PCA_MAX, PCA_SEED = 4, 32, 1e-4, 200, 5
PCA_ARGS = ["--pca-k", PCA_K, "--pca-block", PCA_L, "--pca-tol", PCA_TOL, "--pca-max-iter", PCA_MAX, "--pca-seed", PCA_SEED]
SCORE_C = 5


def one_rank(args, timeout=900):
    r = subprocess.run([REAL] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def _dense_scores(code, Wstd, Wall, dtype):
    """(std, allele) scores of the weight columns on M x N PLINK codes, every individual phenotyped, in `dtype`: per marker mu the mean of
    the present genotypes and msig = 1 / sqrt(sum (a - mu)^2 / (N - 1)) (1 without variance); std: sum_j (a - mu) msig w_j over the
    present genotypes; allele: sum_j w_j a with a missing genotype counted as mu"""
    M, N = code.shape
    zs, za = np.zeros((len(Wstd), N), dtype=dtype), np.zeros((len(Wall), N), dtype=dtype)
    for m0 in range(0, M, 500):
        c = code[m0:m0 + 500]
        a = np.select([c == 0, c == 2, c == 3], [2, 1, 0], 0).astype(dtype)
        have = c != 1
        cnt = have.sum(axis=1).astype(dtype)
        mu = np.where(cnt > 0, np.where(have, a, dtype(0)).sum(axis=1) / np.where(cnt > 0, cnt, dtype(1)), dtype(0))
        d = np.where(have, a - mu[:, None], dtype(0))
        ss = (d * d).sum(axis=1)
        sg = np.where(ss != 0, dtype(1) / np.sqrt(np.where(ss != 0, ss, dtype(1)) / dtype(N - 1)), dtype(1))
        zs += Wstd[:, m0:m0 + 500].astype(dtype) @ (d * sg[:, None])
        za += Wall[:, m0:m0 + 500].astype(dtype) @ np.where(have, a, mu[:, None])
    return zs, za


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    """the toy .bed, three phenotype files (the second with NA lines), the score inputs and the one-rank runs: made once, never changed"""
    d = tmp_path_factory.mktemp("sharded_products")
    bed = _toy_bed(d)
    raw = np.frombuffer(lzma.open(os.path.join(G, "toy.bed.xz")).read(), dtype=np.uint8)[3:]
    code = bx.decode(raw, TN, TMT)[:, :TN]
    rng = np.random.default_rng(61)
    a = np.select([code == 0, code == 2, code == 3], [2.0, 1.0, 0.0], 1.0)
    Y = rng.standard_normal((3, TN)) * np.array([[1.0], [25.0], [1e-2]]) + np.array([[0.0], [3.0], [-1.0]])
    Y[0] += 1.0 * a[4999] - 0.8 * a[5000]                            # effects on the two sides of a shard edge
    present = np.ones(TN, dtype=bool)
    present[np.arange(TN) % 97 == 5] = False
    phen = []
    for k in range(3):
        path = str(d / ("p%d.phen" % k))
        with open(path, "w") as f:
            for n in range(TN):
                f.write("F%d I%d %s\n" % (n, n, "NA" if (k == 1 and not present[n]) else repr(float(Y[k, n]))))
        phen.append(path)
    W = rng.standard_normal((SCORE_C, TMT)) * 10.0 ** rng.integers(-3, 3, (SCORE_C, 1))
    W[3] = 0.0
    idx, p, w0, thr = sp.clump_fixture(TMT)
    masked = np.array([np.where(np.isin(np.arange(TMT), sp.used_markers_global(idx, p, t)), w0, 0.0) for t in thr])
    files = {}
    for name, arr in (("w.bin", W), ("w0.bin", w0), ("p.bin", p), ("idx.bin", idx)):
        files[name] = str(d / name)
        np.asarray(arr, dtype=np.float64).tofile(files[name])
    base = ["--bed-file", bed, "--N", TN, "--Mt", TMT]
    sbase = ["--run-mode", "score", "--bed-file-test", bed, "--N-test", TN, "--Mt-test", TMT]
    legs = {"std": ["--score-file", files["w.bin"], "--score-cols", SCORE_C],
            "allele": ["--score-file", files["w.bin"], "--score-cols", SCORE_C, "--score-units", "allele"],
            "ct": ["--score-file", files["w0.bin"], "--score-cols", 1, "--score-clump-index", files["idx.bin"], "--score-p-file",
                   files["p.bin"], "--score-p-thresholds", ",".join(repr(t) for t in thr)]}
    screen = ["--run-mode", "screen", "--phen-files", ",".join(phen), "--screen-cols", 2] + base
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("GV_TUNE_CACHE", "0")
        out1 = str(d / "one") + "/"
        os.makedirs(out1)
        one_rank(screen + ["--out-dir", out1, "--out-name", "s"])
        for leg, args in legs.items():
            one_rank(sbase + args + ["--out-dir", out1, "--out-name", leg])
    ref = _dense_scores(code, np.vstack([W, masked]), W, np.longdouble)
    r64 = _dense_scores(code, np.vstack([W, masked]), W, np.float64)
    refs = {"std": (ref[0][:SCORE_C], r64[0][:SCORE_C]), "allele": (ref[1], r64[1]), "ct": (ref[0][SCORE_C:], r64[0][SCORE_C:])}
    return dict(d=d, bed=bed, raw=raw, code=code, present=present, phen=phen, base=base, sbase=sbase, legs=legs, screen=screen, out1=out1, refs=refs,
                masked=masked, ncols={"std": SCORE_C, "allele": SCORE_C, "ct": len(thr)})


def _outdir(toy, name):
    out = str(toy["d"] / name) + "/"
    os.makedirs(out)
    return out


@pytest.mark.parametrize("n", [2, 3])
def test_screen_as_a_sharded_job_writes_the_one_rank_files(toy, n, monkeypatch):
    """three phenotype files, the second with NA lines (complete cases on every rank), --screen-cols 2: two calls, the second of one
    column; column c of a rank at value offset c * Mt + S"""
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    out = _outdir(toy, "screen%d" % n)
    stdout = sharded(n, REAL, toy["screen"] + ["--out-dir", out, "--out-name", "s"], no_fatal=True)
    assert "screen: 3 phenotypes x %d markers, %d complete cases of %d" % (TMT, int(toy["present"].sum()), TN) in stdout
    assert sorted(os.listdir(out)) == ["s_screen_p.bin", "s_screen_r.bin", "s_screen_t.bin"]
    for tag in "rtp":
        got, want = (open(o + "s_screen_%s.bin" % tag, "rb").read() for o in (out, toy["out1"]))
        assert len(got) == 3 * TMT * 8 == len(want), (tag, len(got), len(want))
        assert got == want, (tag, sp.first_bit_difference(np.frombuffer(got), np.frombuffer(want)))
    r = np.fromfile(out + "s_screen_r.bin").reshape(3, TMT)
    assert np.all(np.isfinite(r)) and np.all(np.abs(r) <= 1) and np.abs(r[0, 4999]) > 0.1 and np.abs(r[0, 5000]) > 0.1


def _toy_pca_case(toy, present, name):
    code = toy["code"]
    a = np.select([code == 0, code == 2, code == 3], [2, 1, 0], -1)
    return dict(name=name, N=TN, M=TMT, k=PCA_K, L=PCA_L, a=a, present=present, nonas=int(present.sum()), q0=pca_start(PCA_SEED, PCA_L, TN))


def _read_pca(out, pre):
    ev = np.loadtxt(out + pre + "_pca_eigenval.txt", ndmin=1)
    rows = [ln.split() for ln in open(out + pre + "_pca_eigenvec.txt").read().splitlines()]
    assert ev.shape == (PCA_K,) and len(rows) == TN and all(len(r) == PCA_K for r in rows)      # one writer: K lines, N lines of K tokens
    V = np.fromfile(out + pre + "_pca_loadings.bin")
    assert V.size == PCA_K * TMT
    return ev, np.array(rows, dtype=np.float64), V.reshape(PCA_K, TMT)


@pytest.mark.parametrize("n", [2, 3])
def test_pca_then_the_adjusted_screen_as_sharded_jobs(toy, n, monkeypatch):
    """--run-mode pca on the phenotype file with NA lines: the eigenpairs under the checks of tests/test_gpu_pca_driver.py, the loadings of
    every rank at i * Mt + S; then --run-mode screen --cov-file on that eigenvector file, sharded and on one rank: five files, byte for
    byte"""
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    out = _outdir(toy, "pca%d" % n)
    stdout = sharded(n, REAL, ["--run-mode", "pca", "--phen-files", toy["phen"][1], "--out-dir", out, "--out-name", "pc"] + PCA_ARGS
                     + toy["base"], no_fatal=True)
    line = [ln for ln in stdout.splitlines() if ln.startswith("pca: ")]
    assert len(line) == 1 and "converged" in line[0] and "NOT converged" not in line[0], stdout[-2000:]
    assert sorted(os.listdir(out)) == ["pc_pca_eigenval.txt", "pc_pca_eigenvec.txt", "pc_pca_loadings.bin"]
    th, U, V = _read_pca(out, "pc")
    cs = _toy_pca_case(toy, toy["present"], "toy-na")
    A, Gm = pr.dense_G(cs)
    lam, E = pr.eigh(cs)
    r = np.sqrt((((Gm @ U) - U * th[None, :]) ** 2).sum(axis=0))
    assert np.all(r <= 1.01 * PCA_TOL * th), (r, PCA_TOL * th)
    delta = pr.gaps(th, lam)
    if "iterate" not in _TOY:
        _TOY["iterate"] = pr.iterate(cs, PCA_TOL, PCA_MAX, k=PCA_K)
    ref = _TOY["iterate"]
    its = int(re.search(r"(\d+) iterations", line[0]).group(1))
    print("pca %d ranks: %d iterations (restatement %d), r / theta %s, delta %s" % (n, its, ref["iterations"], r / th, delta))
    assert ref["converged"] and its <= ref["iterations"] + 2
    for i in range(PCA_K):
        e, w = E[:, i], ref["U"][:, i]
        s_exact = np.linalg.norm(U[:, i] - e * (e @ U[:, i]))
        s_ref = np.linalg.norm(U[:, i] - w * (w @ U[:, i]))
        assert s_exact <= r[i] / delta[i] + TN * pr.EPS
        assert s_ref <= (r[i] + ref["resid"][i]) / delta[i] + 2 * TN * pr.EPS
        assert abs(th[i] - lam[i]) <= r[i] ** 2 / delta[i] + TN * pr.EPS * lam[0]
    assert np.all(U[~cs["present"]] == 0) and np.array_equal(pr.sign_rule(U), U) and np.all(np.diff(th) <= 0)
    assert np.max(np.abs(U.T @ U - np.eye(PCA_K))) <= TN * pr.EPS
    # the loadings file: v_i = c_i A^T u_i, c_i = sqrt(N / Mt) / sqrt(theta_i), at i * Mt + S of every rank, against the float64 dense A of
    # the restatement applied to the eigenvectors of the file (17 digits: the device's bits).  Per entry: the ATx bound of
    # include/gvamp.h, N 2^-50 max msig max |u| / sqrt(N), for the device; gamma_N sum |A_nj u_n| <= N 2^-53 |A_j|_2 |u|_2 for the float64
    # dot product, doubled for the few roundings in the entries of A; all times c_i.  (An entry of v is ~ 1 / sqrt(Mt) = 1e-2.)
    with capi.Shard(TN, TMT) as sh:
        sh.upload_bed(toy["raw"])
        sh.set_mask(pr.mask4(cs["present"]), cs["nonas"])
        sh.compute_markers_statistics()
        _, msig = sh.marker_stats()
    col = float(np.sqrt((A * A).sum(axis=0)).max())
    for i in range(PCA_K):
        u = U[:, i]
        c = np.sqrt(TN / TMT) / np.sqrt(th[i])
        bound = c * (TN * 2.0 ** -50 * msig.max() * np.abs(u).max() / np.sqrt(TN) + 2 * TN * 2.0 ** -53 * col * np.linalg.norm(u))
        err = float(np.max(np.abs(V[i] - c * (A.T @ u))))
        print("loadings %d: max error %.3e, bound %.3e, |v|^2 - 1 = %.3e" % (i, err, bound, float(V[i] @ V[i]) - 1.0))
        assert err <= bound, (i, err, bound)
        assert abs(float(V[i] @ V[i]) - 1.0) < 1e-6                                # a right singular vector (theta_i is u_i's Rayleigh quotient)
    # the adjusted screen on the eigenvectors the sharded job wrote
    cov = ["--run-mode", "screen", "--phen-files", ",".join(toy["phen"]), "--cov-file", out + "pc_pca_eigenvec.txt", "--C", PCA_K,
           "--screen-cols", 2, "--out-name", "adj"] + toy["base"]
    outs, out1 = _outdir(toy, "cov%d" % n), _outdir(toy, "cov%d_one" % n)
    stdout = sharded(n, REAL, cov + ["--out-dir", outs], no_fatal=True)
    assert "adjusted for %d covariates, %d complete cases" % (PCA_K, cs["nonas"]) in stdout
    one_rank(cov + ["--out-dir", out1])
    assert sorted(os.listdir(outs)) == sorted("adj_screen_%s.bin" % k for k in ("r", "t", "p", "beta", "se")) == sorted(os.listdir(out1))
    for k in ("r", "t", "p", "beta", "se"):
        got, want = (open(o + "adj_screen_%s.bin" % k, "rb").read() for o in (outs, out1))
        assert len(got) == 3 * TMT * 8 == len(want), (k, len(got), len(want))
        assert got == want, (k, sp.first_bit_difference(np.frombuffer(got), np.frombuffer(want)))
    beta = np.fromfile(outs + "adj_screen_beta.bin").reshape(3, TMT)
    assert np.all(np.isfinite(beta)) and abs(beta[0, 4999] - 1.0) < 0.25 and abs(beta[0, 5000] + 0.8) < 0.15


@pytest.mark.parametrize("leg", ["std", "allele", "ct"])
@pytest.mark.parametrize("n", [2, 3])
def test_score_as_a_sharded_job_is_within_16x_of_float64(toy, n, leg, monkeypatch):
    """--run-mode score: every rank its slice [S, S + M) of every column of the weight, p-value and clump-index files, the sum over the
    ranks inside Ax.  std: five columns; allele: the constants sum_j mave_j w_j all-reduced over the ranks; ct: three thresholds on the
    clump index of sharded_products.clump_fixture -- members on both sides of every shard edge whose index marker lives in the other shard,
    an index marker opening every shard, all of them a thousand times louder than the rest: the reference is the dense score of the
    columns the GLOBAL rule selects, so a member that contributed or a shard-first index marker that did not is far outside the bound"""
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    out = _outdir(toy, "score_%s%d" % (leg, n))
    stdout = sharded(n, REAL, toy["sbase"] + toy["legs"][leg] + ["--out-dir", out, "--out-name", leg], no_fatal=True)
    C = toy["ncols"][leg]
    line = [ln for ln in stdout.splitlines() if ln.startswith("scores: ")]
    assert len(line) == 1 and "%d columns (%s units) x %d individuals" % (C, "allele" if leg == "allele" else "std", TN) in line[0]
    assert "fallback path" in line[0]                                   # a sharded job goes through gv_ax_dev and its all-reduce
    assert os.listdir(out) == ["%s_scores.bin" % leg] and os.path.getsize(out + "%s_scores.bin" % leg) == C * TN * 8       # one writer
    got = np.fromfile(out + "%s_scores.bin" % leg).reshape(C, TN)
    one = np.fromfile(toy["out1"] + "%s_scores.bin" % leg).reshape(C, TN)
    ref, r64 = toy["refs"][leg]
    dev64, _ = sp.score_deviation(r64, ref)
    devg, perg = sp.score_deviation(got, ref)
    dev1, _ = sp.score_deviation(one, ref)
    devd, _ = sp.score_deviation(got, one)
    bound = sp.score_bound(dev64)
    print("score %s, %d ranks: float64 dev %.3e  sharded dev %.3e  one-rank dev %.3e  sharded against one-rank %.3e  bound %.3e"
          % (leg, n, dev64, devg, dev1, devd, bound))
    assert dev64 > 0.0
    assert devg <= bound, (devg, bound, perg)
    assert dev1 <= bound and devd <= bound, (dev1, devd, bound)
    if leg == "ct":
        # which markers the columns use: leaving the loud markers at the shard edges out, or taking their members in, is not a rounding
        split = sp.divide_work(TMT, n)
        assert all(toy["masked"][0][S] != 0 and abs(toy["masked"][0][S]) >= 1000.0 for S, _ in split[1:])
        assert all(toy["masked"][2][S - 1] == 0 and toy["masked"][2][S + 3] == 0 for S, _ in split[1:])
        assert np.any(got[0] != got[1]) and np.any(got[1] != got[2])
    else:
        assert np.all(got[3] == 0.0) and np.any(got[0] != 0.0)


@pytest.mark.parametrize("n", [2, 3])
def test_sharded_loadings_score_the_cohort_back_to_its_components(toy, n, monkeypatch):
    """the second check of tests/test_gpu_pca_driver.py on sharded jobs: --run-mode pca on a phenotype file without NA, then its loadings
    file as --score-file of a sharded --run-mode score: z_i / sqrt(Mt) = sqrt(theta_i) u_i within the bound derived there"""
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    out = _outdir(toy, "back%d" % n)
    sharded(n, REAL, ["--run-mode", "pca", "--phen-files", toy["phen"][0], "--out-dir", out, "--out-name", "pc"] + PCA_ARGS + toy["base"],
            no_fatal=True)
    th, U, V = _read_pca(out, "pc")
    sharded(n, REAL, toy["sbase"] + ["--score-file", out + "pc_pca_loadings.bin", "--score-cols", PCA_K, "--out-dir", out, "--out-name", "pc"],
            no_fatal=True)
    Z = np.fromfile(out + "pc_scores.bin").reshape(PCA_K, TN)
    with capi.Shard(TN, TMT) as sh:
        sh.upload_bed(toy["raw"])
        sh.set_mask(pr.mask4(np.ones(TN, dtype=bool)), TN)
        sh.compute_markers_statistics()
        _, msig = sh.marker_stats()
    normA = np.sqrt(th[0] * (1 + 1e-6) * TMT / TN)
    for i in range(PCA_K):
        u, x = U[:, i], np.sqrt(float(TN)) * V[i]
        bound = PCA_TOL * np.sqrt(th[i]) \
            + TN / (TMT * np.sqrt(th[i])) * normA * np.sqrt(TMT) * TN * 2.0 ** -50 * msig.max() * np.abs(u).max() / np.sqrt(TN) \
            + TMT * 2.0 ** -50 * np.max(np.abs(msig * x)) / np.sqrt(TN) / np.sqrt(TMT) \
            + 8 * 2.0 ** -53 * np.sqrt(th[i]) * np.abs(u).max()
        err = float(np.max(np.abs(Z[i] / np.sqrt(TMT) - np.sqrt(th[i]) * u)))
        print("component %d, %d ranks: max error %.3e, bound %.3e" % (i, n, err, bound))
        assert err <= bound, (i, err, bound)
