"""tests/grm_he_restatement.py (the numpy restatement of gv_grm_apply / gv_grm_he) held to itself: the estimator
from the six sums against the explicit pair list (np.polyfit and a literal OLS) and against a literal delete-one jackknife; the
literal chains against a plain matrix product; the degenerate cases; the conditioning of the formulas on every input of the GPU tests
(float64 against np.longdouble to 1e-13, and the first-order error bound at eps = (N + M + 32) 2^-53 below 1e-8, which is what gives
the GPU tolerances their teeth); and the driver's option parser.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import grm_he_restatement as hr
import grm_restatement as gr
import king_restatement as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")
HE_CASES = ("ragged", "pedigree", "deep")           # the inputs of the GPU tests of gv_grm_he
SEED = {"ragged": 101, "pedigree": 102, "deep": 103}


def _dense_apply(r, dtype=np.float64):
    Gs = hr.operators(r["A"], r["M_ij"], dtype)
    return lambda W: tuple(G @ np.asarray(W, dtype=dtype) for G in Gs)


@pytest.fixture(scope="module")
def small():
    geno = kr.random_geno(40, 300, 3, miss=0.05)
    r = gr.grm(geno)
    rng = np.random.default_rng(8)
    y = r["Z"] @ rng.standard_normal(300) / np.sqrt(300.0) + rng.standard_normal(40)
    y[rng.random(40) < 0.1] = np.nan
    return r, y


def test_the_six_sums_give_the_regression_of_the_explicit_pair_list(small):
    r, y = small
    assert np.isnan(y).sum() >= 2 and (r["M_ij"] > 0).all()
    got = hr.he_traits(y.reshape(-1, 1), _dense_apply(r))[0]
    want = hr.he_pairs(r["A"], r["M_ij"], y)
    nk = int((~np.isnan(y)).sum())
    assert got["n_ind"] == nk and got["n_pairs"] == want["n_pairs"] == nk * (nk - 1) // 2
    for f in ("sum_a", "sum_aa", "h2", "intercept", "se_ols"):
        assert abs(got[f] - want[f]) <= 1e-11 * max(1.0, abs(want[f])), (f, got[f], want[f])
    assert np.allclose([got["h2"], got["intercept"]], want["polyfit"], rtol=1e-9, atol=1e-12)


def test_the_row_term_jackknife_equals_deleting_each_individual(small):
    r, y = small
    got = hr.he_traits(y.reshape(-1, 1), _dense_apply(r))[0]
    se, hj = hr.he_jack_literal(r["A"], r["M_ij"], y)
    assert len(hj) == got["n_ind"] and np.allclose(got["h2_jack"], hj, rtol=1e-10, atol=1e-12)
    assert abs(got["se_jack"] - se) <= 1e-10 * se and se > 0


def test_absent_pairs_leave_the_regression(small):
    r, y = small
    r2 = dict(r)
    Mc = r["M_ij"].copy()
    Mc[3, :] = Mc[:, 3] = 0                          # an individual nobody shares a marker with
    Mc[5, 9] = Mc[9, 5] = 0
    r2["M_ij"] = Mc
    got = hr.he_traits(y.reshape(-1, 1), _dense_apply(r2))[0]
    want = hr.he_pairs(r["A"], Mc, y)
    assert got["n_pairs"] == want["n_pairs"] < hr.he_pairs(r["A"], r["M_ij"], y)["n_pairs"]
    assert abs(got["h2"] - want["h2"]) <= 1e-11 * max(1.0, abs(want["h2"]))


def test_the_literal_chains_equal_a_matrix_product_and_handle_signed_zeros():
    cs = gr.case("edge")
    W = np.random.default_rng(2).standard_normal((cs["N"], 5))
    W[:, 2] = 0.0
    W[:, 3] = -np.abs(W[:, 3])                       # 0 * negative = -0.0 must not leak: a chain starts at +0.0
    got = hr.apply_chain(cs["A"], cs["M_ij"], W)
    for g, G in zip(got, hr.operators(cs["A"], cs["M_ij"])):
        ref = G @ W
        assert np.all(np.abs(g - ref) <= (cs["N"] + 2) * 2.0 ** -53 * (np.abs(G) @ np.abs(W)))
        assert np.all(g[:, 2].view(np.uint64) == 0)
    e = np.zeros((cs["N"], 1))
    e[100, 0] = 1.0                                  # a unit column returns the operator's column, bit for bit
    g0, g1, g2 = hr.apply_chain(cs["A"], cs["M_ij"], e)
    on, G1, G2 = hr.operators(cs["A"], cs["M_ij"])
    assert kr.same_bits(g1[:, 0], G1[:, 100]) and kr.same_bits(g2[:, 0], G2[:, 100]) and np.array_equal(g0[:, 0], on[:, 100])
    assert g1[100, 0] == 0 and g0[100, 0] == 0


def test_degenerate_traits_give_nan():
    cs = gr.case("tiny")
    N = cs["N"]
    const = np.full(N, 2.5)
    two = np.full(N, np.nan)
    two[:2] = (1.0, 3.0)
    none = np.full(N, np.nan)
    for y, nk in ((const, N), (two, 2), (none, 0)):
        rec = hr.he_traits(y.reshape(-1, 1), _dense_apply(cs))[0]
        assert rec["n_ind"] == nk and all(np.isnan(rec[f]) for f in hr.DERIVED), rec
    A = np.full((4, 4), 0.25)                        # every x equal: D = 0
    rec = hr.he_traits(np.array([[0.1], [0.7], [-1.0], [2.0]]), _dense_apply(dict(A=A, M_ij=np.full((4, 4), 9))))[0]
    assert rec["n_pairs"] == 6 and all(np.isnan(rec[f]) for f in hr.DERIVED)


@pytest.mark.parametrize("name", HE_CASES)
def test_float64_and_long_double_agree_to_1e_13_on_every_gpu_input(name):
    cs = gr.case(name)
    Y = hr.traits(cs, SEED[name])
    lo = hr.he_traits(Y, _dense_apply(cs), np.float64)
    hi = hr.he_traits(Y, _dense_apply(cs, np.longdouble), np.longdouble)
    for c, (a, b) in enumerate(zip(lo, hi)):
        assert a["n_pairs"] == b["n_pairs"] > 3
        for f in FIELDS_F:
            rel = abs(float(a[f]) - float(b[f])) / abs(float(b[f]))
            print(name, c, f, float(b[f]), "rel diff", rel)
            assert rel <= 1e-13, (name, c, f)


FIELDS_F = ("sum_a", "sum_aa", "h2", "intercept", "se_ols", "se_jack")


@pytest.mark.parametrize("name", HE_CASES)
def test_the_error_bound_at_the_gpu_tests_eps_is_below_1e_8(name):
    cs = gr.case(name)
    Y = hr.traits(cs, SEED[name])
    eps = (cs["N"] + cs["M"] + 32) * 2.0 ** -53
    for c in range(Y.shape[1]):
        b = hr.he_bound(cs, Y[:, c], eps)
        print(name, c, {k: float(v) for k, v in b.items()})
        assert all(0 < v < 1e-8 for v in b.values()), (name, c, b)


def _run(args, env=None):
    import __graft_entry__ as g
    g.build()
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    e.update(env or {})
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=e, timeout=60)


def test_the_driver_knows_run_mode_he_and_refuses_dense_data_sharded_jobs_and_missing_files(tmp_path):
    phen = tmp_path / "y.phen"
    phen.write_text("".join("f%d i%d %g\n" % (n, n, 0.5 * n) for n in range(8)))
    base = ["--run-mode", "he", "--bed-file", "x.bed", "--N", "8", "--Mt", "12", "--out-dir", str(tmp_path) + "/", "--out-name", "bad"]
    for fmt in ("dosage8", "dosage16"):
        r = _run(base + ["--phen-files", str(phen), "--geno-format", fmt])
        assert r.returncode == 1 and "unknown --run-mode" not in r.stdout
        assert "FATAL: --run-mode he works on 2-bit genotypes only, not on --geno-format " + fmt in r.stdout, r.stdout[-2000:]
    r = _run(base + ["--phen-files", str(phen)], env={"WORLD_SIZE": "2"})
    assert r.returncode == 1 and "FATAL: --run-mode he runs on one rank" in r.stdout, r.stdout[-2000:]
    r = _run(base + ["--phen-files", str(tmp_path / "nothing.phen")])
    assert r.returncode != 0 and "FATAL" in r.stdout + r.stderr and "nothing.phen not found" in r.stdout + r.stderr
    r = _run(base)
    assert r.returncode != 0 and "no phen file(s) provided" in r.stdout
    short = tmp_path / "five.bin"
    short.write_bytes(bytes(5))
    r = _run(base + ["--phen-files", str(phen), "--grm-marker-file", str(short)])
    assert r.returncode == 1 and "FATAL: --grm-marker-file" in r.stdout and "must hold Mt = 12 bytes" in r.stdout, r.stdout[-2000:]
    assert not any(f.startswith("bad") for f in os.listdir(tmp_path))
