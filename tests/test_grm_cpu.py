"""tests/grm_restatement.py (the numpy restatement of gv_grm_*) held to a brute-force double loop, to hand cases
and to the simulated pedigree; and the driver's option parser: --run-mode grm exists and refuses dense data before any device work.
No GPU."""
import os
import subprocess

import numpy as np
import pytest

import grm_restatement as gr
import king_restatement as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "gvamp_amd", "gvamp_main_real")


def test_the_restatement_equals_a_brute_force_double_loop_over_pairs():
    geno = kr.random_geno(40, 300, 3, miss=0.05)
    use = (np.arange(300) % 7 != 3).astype(np.uint8)
    for u in (None, use):
        r = gr.grm(geno, u)
        A, Mij = gr.brute(geno, u)
        assert np.array_equal(Mij, r["M_ij"])
        assert gr.within(A, r)
        assert kr.same_bits(r["A"], r["A"].T)


def test_hand_cases_duplicate_use_mask_dead_markers_and_an_all_missing_individual():
    geno = kr.random_geno(30, 200, 4, miss=0.05)
    geno[11] = geno[10]                                            # a duplicate equals its own diagonal
    r = gr.grm(geno)
    assert kr.same_bits(r["A"][10, 11], r["A"][10, 10]) and kr.same_bits(r["A"][11, 11], r["A"][10, 10])
    assert r["M_ij"][10, 11] == r["M_ij"][10, 10]
    use = (np.random.default_rng(1).random(200) < 0.6).astype(np.uint8)      # a use mask equals deleting the markers
    a, b = gr.grm(geno, use), gr.grm(geno[:, use != 0])
    assert np.array_equal(a["M_ij"], b["M_ij"]) and gr.within(a["A"], b) and a["counting"].sum() == b["counting"].sum()
    assert np.array_equal(a["mu"][use != 0].view(np.uint64), b["mu"].view(np.uint64))
    assert np.all(a["mu"][use == 0] == 0) and np.all(a["rs"][use == 0] == 0)
    dead = np.concatenate([geno, np.zeros((30, 1), int), np.full((30, 1), 2), np.full((30, 1), -1)], axis=1)
    d = gr.grm(dead)                                               # monomorphic and all-missing markers change nothing
    assert d["dropped"] == r["dropped"] + 3 and np.array_equal(d["M_ij"], r["M_ij"]) and gr.within(d["A"], r)
    assert np.all(d["mu"][-3:] == 0) and np.all(d["rs"][-3:] == 0)
    gone = geno.copy()
    gone[5] = -1                                                   # an all-missing individual: NaN, M_ij = 0
    g = gr.grm(gone)
    assert np.all(np.isnan(g["A"][5])) and np.all(np.isnan(g["A"][:, 5])) and np.all(g["M_ij"][5] == 0)
    assert np.isfinite(np.delete(np.delete(g["A"], 5, 0), 5, 1)).all()


def test_the_hand_placed_features_of_ragged_survive():
    cs = gr.case("ragged")
    g = cs["geno"]
    assert set(np.unique(g[:, gr.MONO0])) == {-1, 0} and set(np.unique(g[:, gr.MONO2])) == {-1, 2} and np.all(g[:, gr.ALLMISS] == -1)
    assert (g[:, gr.SINGLETON] == 1).sum() == 1 and (g[:, gr.SINGLETON] == 2).sum() == 0
    assert np.all(g[gr.MISSING_IND] == -1) and np.array_equal(g[gr.DUP_A], g[gr.DUP_B])
    assert not cs["counting"][[gr.MONO0, gr.MONO2, gr.ALLMISS]].any() and cs["counting"][gr.SINGLETON] and cs["dropped"] == 3
    assert np.argmax(np.abs(cs["Z"]).max(axis=0)) == gr.SINGLETON
    assert np.all(np.isnan(cs["A"][gr.MISSING_IND])) and np.all(cs["M_ij"][gr.MISSING_IND] == 0)
    assert kr.same_bits(cs["A"][gr.DUP_A, gr.DUP_B], cs["A"][gr.DUP_A, gr.DUP_A])


def test_every_pair_of_the_pedigree_lands_in_its_class():
    cs = gr.case("pedigree")
    N, A, truth = cs["N"], cs["A"], cs["truth"]
    i, j = np.triu_indices(N, 1)
    v, t = A[i, j], truth[i, j]
    assert len(v) == 2211
    got = np.where(v >= gr.CUT_DUP, kr.DUP, np.where(v >= gr.CUT_FIRST, kr.FIRST, np.where(v >= gr.CUT_SECOND, kr.SECOND, kr.UNREL)))
    assert np.array_equal(got, t)
    # the ranges of the classes, to the three decimals they were recorded with
    for cls, lo, hi in ((kr.DUP, 0.963, 1.008), (kr.FIRST, 0.404, 0.492), (kr.SECOND, 0.183, 0.235)):
        assert round(v[t == cls].min(), 3) == lo and round(v[t == cls].max(), 3) == hi, (cls, v[t == cls].min(), v[t == cls].max())
    assert round(v[t == kr.UNREL].max(), 3) <= 0.042
    assert round(np.diag(A).mean(), 3) == 0.983
    assert (t != kr.UNREL).sum() == 83


@pytest.mark.parametrize("name", gr.CASES)
def test_no_reference_value_sits_within_its_bound_of_the_cutoffs(name):
    cs = gr.case(name)
    i, j = np.triu_indices(cs["N"], 1)
    for cutoff in (0.1, 0.7):
        assert not gr.near(cs, cutoff)[i, j].any()


def test_two_summation_orders_of_the_restatement_stay_inside_the_bound():
    cs = gr.case("edge")
    Z = cs["Z"].astype(np.longdouble)
    S = np.zeros((cs["N"], cs["N"]), dtype=np.longdouble)
    for m in range(cs["M"] - 1, -1, -1):
        S += np.outer(Z[:, m], Z[:, m])
    with np.errstate(divide="ignore", invalid="ignore"):
        A = np.where(cs["M_ij"] > 0, (S / np.maximum(cs["M_ij"], 1)).astype(np.float64), np.nan)
    assert gr.within(A, cs)


def _run(args, env=None):
    import __graft_entry__ as g
    g.build()
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}
    e.update(env or {})
    return subprocess.run([EXE] + args, capture_output=True, text=True, env=e, timeout=60)


def test_the_driver_knows_run_mode_grm_and_refuses_dense_data_and_sharded_jobs(tmp_path):
    base = ["--run-mode", "grm", "--bed-file", "x.bed", "--N", "8", "--Mt", "12", "--out-dir", str(tmp_path) + "/", "--out-name", "bad"]
    for fmt in ("dosage8", "dosage16"):
        r = _run(base + ["--geno-format", fmt, "--grm-cutoff", "0.05"])
        assert r.returncode == 1 and "unknown --run-mode" not in r.stdout
        assert "FATAL: --run-mode grm works on 2-bit genotypes only, not on --geno-format " + fmt in r.stdout, r.stdout[-2000:]
    r = _run(base, env={"WORLD_SIZE": "2"})
    assert r.returncode == 1 and "FATAL: --run-mode grm runs on one rank" in r.stdout, r.stdout[-2000:]
    short = tmp_path / "five.bin"
    short.write_bytes(bytes(5))
    r = _run(base + ["--grm-marker-file", str(short)])
    assert r.returncode == 1 and "FATAL: --grm-marker-file" in r.stdout and "must hold Mt = 12 bytes" in r.stdout, r.stdout[-2000:]
    r = _run(base + ["--grm-cutoff", "abc"])
    assert r.returncode != 0 and "--grm-cutoff has to be a number" in r.stdout + r.stderr
    assert not any(f.startswith("bad") for f in os.listdir(tmp_path))
