"""Principal components of the resident genotypes without a GPU (gv_pca_dev): the numpy restatement of the block
subspace iteration (tests/pca_restatement.py) is held, on every shape of the GPU tests, to the same properties the library is held to
against numpy.linalg.eigh of the dense relationship matrix -- the residual promise checked outside the iteration, the Davis-Kahan and
Kato-Temple bounds, the structure of the outputs -- and the inputs to what the issue asks of them (theta_1 / theta_k <= 2, under 30
iterations at tol = 1e-9).  The packer is held to the decoder of tests/bed_fixed_restatement.py.  Then the declarations: the header, the
binding, the build list and the driver's option text."""
import os
import re

import numpy as np
import pytest

import bed_fixed_restatement as bx
import pca_restatement as pr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-9


@pytest.mark.parametrize("name", list(pr.SHAPES))
def test_restatement_holds_the_properties_against_eigh(name):
    cs = pr.case(name)
    res = pr.iterate(cs, TOL, 100)
    assert res["converged"] and res["iterations"] < 30, res["iterations"]
    fig = pr.check_pairs(cs, res["theta"], res["U"], res["resid"], TOL)
    lam, _ = pr.eigh(cs)
    assert lam[0] / lam[cs["k"] - 1] <= 2.0
    assert lam[cs["L"] - 1] > 1e-6 * lam[0]                      # rank(G) >= L: the block can be orthonormalised
    print(name, res["iterations"], fig["theta"], fig["resid"], fig["outside"], fig["sin"], fig["orth"])


@pytest.mark.parametrize("name", list(pr.SHAPES))
def test_inputs_are_what_the_shapes_are_for(name):
    cs = pr.case(name)
    N, M = cs["N"], cs["M"]
    code = bx.decode(cs["bed"], N, M)[:, :N]
    a = np.select([code == 0, code == 2, code == 3], [2, 1, 0], -1)
    assert np.array_equal(a, cs["a"])                            # the packer against the decoder of the fixed-point restatement
    assert np.all(cs["a"][M // 2] == 2)                          # the monomorphic marker
    if M >= 8:
        assert np.all(cs["a"][M // 3] == -1)                     # the all-missing marker
        miss = float((cs["a"] == -1).mean())
        assert 0.03 < miss < 0.07 and 0 < N - cs["nonas"] < 0.06 * N
    A, G = pr.dense_G(cs)
    assert np.all(A[~cs["present"], :] == 0) and np.all(A[:, M // 2] == 0)
    assert np.allclose(A.sum(axis=0), 0, atol=1e-12)             # centred over the phenotyped individuals with a genotype
    n = np.arange(N)
    assert np.array_equal(((cs["m4"][n >> 2] >> (n & 3)) & 1).astype(bool), cs["present"])   # bit n & 3 of byte n >> 2


def test_one_iteration_is_not_converged_and_its_residual_is_the_outside_norm():
    cs = pr.case("ragged")
    res = pr.iterate(cs, TOL, 1)
    assert not res["converged"] and res["iterations"] == 1
    pr.check_pairs(cs, res["theta"], res["U"], res["resid"], TOL, converged=False)


def test_a_repeated_column_is_rank_deficient():
    cs = pr.case("second-step")
    q0 = cs["q0"].copy()
    q0[3] = q0[1]
    with pytest.raises(pr.RankDeficient):
        pr.iterate(cs, TOL, 5, q0=q0)


def test_declarations():
    hdr = open(os.path.join(ROOT, "include", "gvamp.h")).read()
    for fn in ("gv_pca_dev", "gv_pca_loadings_dev", "gv_pca_info"):
        assert re.search(r"\bint %s\(" % fn, hdr), fn
    assert re.search(r"#define GV_PCA_MAX_BLOCK 32\b", hdr) and "typedef struct gv_pca_stats" in hdr
    assert re.search(r"#define GV_ABI_VERSION 4\b", hdr)
    from gvamp_amd import capi
    for fn in ("gv_pca_dev", "gv_pca_loadings_dev", "gv_pca_info"):
        assert fn in capi.EXPORTS
    for meth in ("pca_dev", "pca", "pca_info", "pca_loadings_dev"):
        assert callable(getattr(capi.Shard, meth))
    import ctypes
    assert ctypes.sizeof(capi.PcaStats) == 64 and capi.PCA_MAX_BLOCK == 32
    assert "gv_pca.hip" in __import__("gvamp_amd.build", fromlist=["SOURCES"]).SOURCES
    opts = open(os.path.join(ROOT, "gvamp_amd", "csrc", "host", "options.hpp")).read()
    assert "--run-mode pca" in opts
    for flag in ("--pca-k", "--pca-block", "--pca-tol", "--pca-max-iter", "--pca-seed", "--pca-allow-unconverged"):
        assert flag in opts, flag
    main = open(os.path.join(ROOT, "gvamp_amd", "csrc", "host", "main_real.cpp")).read()
    assert '{"pca", run_pca}' in main and "int run_pca(const Job& job)" in main and "_pca_eigenvec.txt" in main and "_pca_loadings.bin" in main
