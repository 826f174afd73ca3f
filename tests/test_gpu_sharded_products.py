"""The batch products in a marker-sharded job (DESIGN.md sections 21, 23, 24, 26): gv_score_dev, gv_atxm_dev / gv_screen_dev,
gv_pca_dev / gv_pca_loadings_dev and gv_screen_cov_set / gv_screen_cov_dev on contexts created as capi.Shard(N, M, Mt=Mt, S=S), one
thread per rank, joined by the in-process communicator -- every rank its own slab of the .bed, the same mask on every rank -- and
held to the ONE context that holds the whole matrix (which the rest of the suite holds to the restatements).

Tile layout, kernel mode 1, GV_TUNE_CACHE=0.  Data: the `ragged` cases of tests/bed_fixed_restatement.py (marker products, score) and
of tests/pca_restatement.py (PCA), N = 1003 x Mt = 517, NA phenotypes, a monomorphic and an all-missing marker.  Splits
(tests/sharded_products.py): even2 = divide_work over two ranks; uneven3 = [0, 1), [1, 65), [65, 517): one marker (a partial tile, fewer
markers than the PCA block), exactly one 64-marker row group, a ragged rest; empty3 = [0, 300), [300, 300), [300, 517): a rank without
markers, which must still enter every collective (a rank that leaves one early leaves its peers waiting: the joins have a time limit
and the test asserts that no thread is alive).

Bars.
* marker statistics, atxm_dev, screen_dev (r, t, p), screen_cov_set + screen_cov_dev (r, t, p, beta, se; K = 3 and K = 17): per-marker
  quantities, no collective.  The shards' outputs written at c * Mt + S equal the one-context output bit for bit (uint64 views: signed
  zeros and NaN payloads included), on 9 columns (a second pass of the batch kernel, a zero column).  No quantity of these was found to
  depend on the shard: the sums over individuals are exact integers, and the ordered fp64 sums beside them (the column's sum P, the
  covariate panels' Grams) run over npad = f(N) alone.
* score_dev: the same bits on every rank; path "fallback", 9 columns; against the long-double dense A W at most 16 x the deviation of the
  float64 dense A W and never less than 1e-12 (section 15; the deviation of a column is max |dz| / max |z|, tests/sharded_products.py);
  NA and pad slots exactly 0.  Both deviations are printed.
* pca_dev (tol 1e-9, at most 100 iterations) + pca_loadings_dev: no rank refuses (the block is bounded by min(nonas, Mt), not by the
  shard's M); eval, resid, U, iterations and converged identical on every rank; pr.check_pairs against the restatement's G of the whole
  matrix; iterations <= the restatement's + 2; the loadings, concatenated, equal c_i A^T u_i of the whole matrix in one context bit for
  bit and have unit norm to 1e-6 (the check of tests/test_gpu_pca.py); cols_atxm == cols_score == L * iterations on every rank.
* afterwards one atx_dev and one ax_dev on every joined context equal their values from before the batch calls, bit for bit."""
import threading
import time

import numpy as np
import pytest

import bed_fixed_restatement as bx
import pca_restatement as pr
import screen_cov_restatement as sc
import sharded_products as sp
from gvamp_amd import capi

pytestmark = pytest.mark.gpu
TOL, MAX_ITER = 1e-9, 100
JOIN_SECONDS = 600
PIN_VARS = ("GV_ATXM_COLS", "GV_ATXM_KS", "GV_ATXM_KERNEL", "GV_SCORE_COLS", "GV_SCORE_KS", "GV_SCORE_KERNEL")
SPLITS = sp.splits()
NAMES5 = sc.NAMES
_CACHE = {}


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    for k in PIN_VARS:
        monkeypatch.delenv(k, raising=False)


def _context(cs, S, M, Mt):
    """a context on the markers [S, S + M) of case cs: its own slab of the .bed, the case's mask"""
    mb = (cs["N"] + 3) // 4
    sh = capi.Shard(cs["N"], M, Mt=Mt, S=S)
    sh.set_layout(False, 2)
    sh.set_kernel_mode(1)
    sh.upload_bed(np.asarray(cs["bed"], dtype=np.uint8)[S * mb:(S + M) * mb])
    sh.set_mask(cs["m4"], cs["nonas"])
    sh.compute_markers_statistics()
    return sh


def _job(cs, split, group, body):
    """body(sh, rank, S, M) on one thread per rank, the contexts joined by comm_init_local(group, ..); the ranks' results"""
    n = len(split)
    results, errors = [None] * n, []

    def work(rank):
        try:
            S, M = split[rank]
            with _context(cs, S, M, cs["M"]) as sh:
                assert sh.get_layout() == 2 and sh.get_kernel_mode() == 1
                sh.comm_init_local(group, n, rank)
                results[rank] = body(sh, rank, S, M)
        except BaseException as e:   # noqa: BLE001
            errors.append((rank, repr(e)))

    th = [threading.Thread(target=work, args=(r,), daemon=True) for r in range(n)]
    for t in th:
        t.start()
    t_end = time.time() + JOIN_SECONDS
    for t in th:
        t.join(timeout=max(0.1, t_end - time.time()))
    assert not errors, errors                      # a rank that failed leaves its peers waiting: report the cause first
    assert not any(t.is_alive() for t in th), "a rank is stuck in a collective"
    return results


def _probe_inputs(cs):
    rng = np.random.default_rng(77)
    x = rng.standard_normal(cs["M"])
    p = np.zeros(cs["npad"])
    p[:cs["N"]] = rng.standard_normal(cs["N"]) * cs["present"]
    return x, p


def _probe(sh, cs, S, M):
    """one atx_dev and one ax_dev (the ax_dev is a collective: every rank calls _probe at the same places)"""
    x, p = _probe_inputs(cs)
    xv, pv, zn, zm = sh.vecM(x[S:S + M]), sh.vecN(p), sh.vecN().fill(7.0), sh.vecM().fill(7.0)
    sh.atx_dev(pv, zm)
    sh.ax_dev(xv, zn)
    out = (zm.download(), zn.download())
    for v in (xv, pv, zn, zm):
        v.free()
    return out


def _context_as_found(results):
    for r, res in enumerate(results):
        for a, b, what in zip(res["before"], res["after"], ("atx_dev", "ax_dev")):
            assert sp.first_bit_difference(a, b) is None, (r, what, sp.first_bit_difference(a, b))
    sp.assert_same_on_every_rank([res["after"][1] for res in results], "ax_dev after the calls")
    assert np.any(results[0]["after"][1] != 0)


def _free(*lists):
    for vs in lists:
        for v in vs:
            v.free()


# ---- the per-marker products ----------------------------------------------------------------------------------------------------------
def _marker_body(cs, cols, covs):
    def body(sh, rank, S, M):
        out = dict(before=_probe(sh, cs, S, M))
        out["mave"], out["msig"] = sh.marker_stats()
        ps = [sh.vecN(c) for c in cols]
        os_ = [sh.vecM().fill(7.0) for _ in cols]
        sh.atxm_dev(ps, os_)
        out["atxm"] = np.stack([o.download() for o in os_])
        out["atxm_info"] = sh.atxm_info()
        res = [[sh.vecM().fill(7.0) for _ in cols] for _ in range(3)]
        sh.screen_dev(ps, *res)
        for k, name in enumerate("rtp"):
            out["screen_" + name] = np.stack([v.download() for v in res[k]])
        out["screen_info"] = sh.atxm_info()
        _free(os_, *res)
        for tag, Cov in covs.items():
            sh.screen_cov_set(Cov)
            res = [[sh.vecM().fill(7.0) for _ in cols] for _ in NAMES5]
            sh.screen_cov_dev(ps, *res)
            for k, name in enumerate(NAMES5):
                out["cov%s_%s" % (tag, name)] = np.stack([v.download() for v in res[k]])
            out["cov%s_info" % tag] = sh.screen_cov_info()
            _free(*res)
        _free(ps)
        out["after"] = _probe(sh, cs, S, M)
        return out
    return body


def _marker_inputs():
    fx = sc.fixture("ragged")
    cs = fx["cs"]
    return cs, sp.phenotype_columns(cs), {"3": fx["Cov"][:3], "17": sc.random_covariates(cs, 17)}


MARKER_KEYS = ["atxm"] + ["screen_" + k for k in "rtp"] + ["cov%s_%s" % (t, k) for t in ("3", "17") for k in NAMES5]


def _whole_marker_products():
    """the one context on the whole matrix: computed once, shared, never changed"""
    if "marker" not in _CACHE:
        cs, cols, covs = _marker_inputs()
        with pytest.MonkeyPatch.context() as mp:
            mp.setenv("GV_ATXM_KERNEL", "1")
            with _context(cs, 0, cs["M"], cs["M"]) as sh:
                _CACHE["marker"] = _marker_body(cs, cols, covs)(sh, 0, 0, cs["M"])
    return _CACHE["marker"]


@pytest.mark.parametrize("split", list(SPLITS))
def test_marker_products_concatenate_to_the_one_context_bits(split, monkeypatch):
    cs, cols, covs = _marker_inputs()
    Mt = cs["M"]
    assert Mt == sp.MT and cols.shape == (9, cs["npad"]) and not cols[3].any()
    whole = _whole_marker_products()
    info = whole["atxm_info"]
    assert info["path"] == "kernel" and info["passes"] == -(-9 // info["cols_per_pass"]) >= 2, info
    # what the one context says about these inputs: the NaN markers of the screens, and outputs that are not trivially equal.  (The
    # marginal screen takes its columns as prepared: only the standard-normal kind is close enough to one to be read as a correlation;
    # the adjusted screen scales every column itself.  The zero columns 3 and 7 are NaN or 0 throughout.)
    for key in MARKER_KEYS[1:]:
        nan = np.isnan(whole[key][[0, 4, 8] if key.startswith("screen_") else [0, 1, 2, 4, 5, 6, 8]])
        assert np.array_equal(np.nonzero(nan.any(axis=0))[0], [bx.MONO, bx.ALLMISS]) and np.all(nan[:, [bx.MONO, bx.ALLMISS]]), key
    assert np.all(whole["atxm"][3] == 0) and np.any(whole["atxm"][0] != 0) and not np.any(whole["atxm"] == 7.0)
    monkeypatch.setenv("GV_ATXM_KERNEL", "1")
    shards = SPLITS[split]
    results = _job(cs, shards, 9100 + list(SPLITS).index(split), _marker_body(cs, cols, covs))
    for (S, M), res in zip(shards, results):
        if M > 0:
            assert res["atxm_info"]["path"] == "kernel" and res["screen_info"]["path"] == "kernel", (S, M, res["atxm_info"])
        assert res["atxm_info"]["columns"] == 9 and res["screen_info"]["columns"] == 9
        assert res["cov3_info"]["K"] == 3 and res["cov17_info"]["K"] == 17 and res["cov17_info"]["nu"] == cs["nonas"] - 2 - 17
        assert res["atxm"].shape == (9, M)
    for key in ("mave", "msig"):
        sp.assert_concatenation_is_the_one_shard_result(shards, Mt, [res[key][None, :] for res in results], whole[key][None, :], key)
    for key in MARKER_KEYS:
        sp.assert_concatenation_is_the_one_shard_result(shards, Mt, [res[key] for res in results], whole[key], key)
    _context_as_found(results)
    # the probes of the joined contexts against the one context: ATx bit for bit; Ax is a sum over the ranks, another rounding
    sp.assert_concatenation_is_the_one_shard_result(shards, Mt, [res["after"][0][None, :] for res in results], whole["after"][0][None, :],
                                                    "atx_dev")


# ---- Z = A W ----------------------------------------------------------------------------------------------------------------------------
def _score_inputs():
    if "score" not in _CACHE:
        cs = bx.case("ragged")
        whole = _whole_marker_products()
        W = sp.score_columns(cs, whole["mave"], whole["msig"])
        ref = sp.dense_score(sp.dense_A(cs["bed"], cs["N"], cs["M"], cs["present"]), W)
        r64 = sp.dense_score(sp.dense_A(cs["bed"], cs["N"], cs["M"], cs["present"], dtype=np.float64), W)
        with _context(cs, 0, cs["M"], cs["M"]) as sh:
            one = sh.score(W)
        _CACHE["score"] = (cs, W, ref, r64, one)
    return _CACHE["score"]


@pytest.mark.parametrize("split", list(SPLITS))
def test_score_is_the_same_on_every_rank_and_within_16x_of_float64(split):
    cs, W, ref, r64, one = _score_inputs()
    N, Mt = cs["N"], cs["M"]
    shards = SPLITS[split]

    def body(sh, rank, S, M):
        out = dict(before=_probe(sh, cs, S, M))
        xs, zs = [sh.vecM(w[S:S + M]) for w in W], [sh.vecN().fill(7.0) for _ in W]
        sh.score_dev(xs, zs)
        out["Z"] = np.stack([z.download() for z in zs])
        out["info"] = sh.score_info()
        _free(xs, zs)
        out["after"] = _probe(sh, cs, S, M)
        return out

    results = _job(cs, shards, 9200 + list(SPLITS).index(split), body)
    for res in results:
        assert res["info"]["path"] == "fallback" and res["info"]["columns"] == 9, res["info"]
    sp.assert_same_on_every_rank([res["Z"] for res in results], "score_dev")
    Z = results[0]["Z"]
    gone = np.ones(Z.shape[1], dtype=bool)
    gone[:N] = ~cs["present"]
    assert np.all(Z[:, gone] == 0.0) and np.any(Z[0] != 0) and np.all(Z[3] == 0)
    dev64, per64 = sp.score_deviation(r64, ref)
    devg, perg = sp.score_deviation(Z[:, :N], ref)
    dev1, _ = sp.score_deviation(one[:, :N], ref)
    bound = sp.score_bound(dev64)
    print("score %s: float64 dev %.3e  sharded GPU dev %.3e  one-context GPU dev %.3e  bound %.3e  (per column, GPU: %s)"
          % (split, dev64, devg, dev1, bound, " ".join("%.1e" % d for d in perg)))
    assert dev64 > 0.0
    assert devg <= bound, (devg, bound, perg)
    _context_as_found(results)


# ---- principal components -------------------------------------------------------------------------------------------------------------
def _pca_reference():
    if "pca" not in _CACHE:
        cs = pr.case("ragged")
        _CACHE["pca"] = (cs, pr.iterate(cs, TOL, MAX_ITER))
    return _CACHE["pca"]


@pytest.mark.parametrize("split", list(SPLITS))
def test_pca_is_the_same_on_every_rank_and_holds_the_bounds(split):
    cs, ref = _pca_reference()
    cs = dict(cs, npad=4 * ((cs["N"] + 3) // 4))
    N, Mt, k, L = cs["N"], cs["M"], cs["k"], cs["L"]
    assert Mt == sp.MT
    shards = SPLITS[split]
    Q0 = np.zeros((L, cs["npad"]))
    Q0[:, :N] = cs["q0"]

    def body(sh, rank, S, M):
        out = dict(before=_probe(sh, cs, S, M))
        q0, us, vs = [sh.vecN(q) for q in Q0], [sh.vecN().fill(7.0) for _ in range(k)], [sh.vecM().fill(7.0) for _ in range(k)]
        out["eval"], out["resid"] = sh.pca_dev(q0, us, TOL, MAX_ITER)
        out["info"] = sh.pca_info()
        out["U"] = np.stack([u.download() for u in us])
        sh.pca_loadings_dev(us, out["eval"], vs)
        out["V"] = np.stack([v.download() for v in vs])
        _free(q0, us, vs)
        out["after"] = _probe(sh, cs, S, M)
        return out

    results = _job(cs, shards, 9300 + list(SPLITS).index(split), body)       # (a refusal of any rank is an error of the job)
    for key in ("eval", "resid", "U"):
        sp.assert_same_on_every_rank([res[key] for res in results], key)
    info = results[0]["info"]
    for res in results:
        assert (res["info"]["iterations"], res["info"]["converged"]) == (info["iterations"], info["converged"])
        assert res["info"]["block"] == L and res["info"]["cols_atxm"] == res["info"]["cols_score"] == L * res["info"]["iterations"]
    res = results[0]
    assert np.all(res["U"][:, N:] == 0)                                       # pad slots
    fig = pr.check_pairs(cs, res["eval"], res["U"][:, :N].T, res["resid"], TOL)
    print("pca %s: %d iterations (restatement %d)" % (split, info["iterations"], ref["iterations"]), fig)
    assert info["converged"] == 1 and info["iterations"] <= ref["iterations"] + 2, (info, ref["iterations"])
    # the loadings: every rank's own markers, concatenated, against c_i A^T u_i of the whole matrix in one context
    with _context(cs, 0, Mt, Mt) as sh:
        uv, wv = sh.vecN(), sh.vecM()
        AtU = []
        for u in res["U"]:
            uv.upload(u)
            sh.atx_dev(uv, wv)
            AtU.append(wv.download())
    V = sp.assemble(shards, Mt, [r_["V"] for r_ in results]).reshape(k, Mt)
    for i in range(k):
        c = np.sqrt(np.float64(N) / np.float64(Mt)) / np.sqrt(np.float64(res["eval"][i]))
        assert sp.first_bit_difference(V[i], c * AtU[i]) is None, (i, sp.first_bit_difference(V[i], c * AtU[i]))
        assert abs(float(V[i] @ V[i]) - 1.0) < 1e-6
    _context_as_found(results)
