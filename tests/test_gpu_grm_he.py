"""gv_grm_apply / gv_grm_he against tests/grm_he_restatement.py, on the cases of tests/grm_restatement.py.

gv_grm_apply is held BIT for bit (uint64 view) to the literal chains of the contract fed the library's own gv_grm_block bits -- in
kernel modes 1 and 2, for C = 1, 3, 8, 32, under a use mask, under forced passes -- and to the numpy reference within derived bounds:

    g0: exact -- a sum of at most N terms w, compared with the bound (N + 2) 2^-53 absT0 of an N-term sum (0 for a 0 / 1 panel)
    g1: sum_j (e_ij + 2^-52 |A_ij|) |w_jc| + (N + 2) 2^-53 absT1
        e_ij is section 28's entry bound: the library's entry differs from the reference's by at most e_ij; 2^-52 |A| |w| covers the
        rounding of the product and of the reference entry; the last term is an N-term fp64 sum in any order
    g2: sum_j (e2_ij + 2^-52 A_ij^2) |w_jc| + (N + 2) 2^-53 absT2,    e2 = 2 |A| e + e^2 + 2^-53 (|A| + e)^2
        (A + d)^2 = A^2 + 2 A d + d^2 with |d| <= e, and fl of the square adds 2^-53 (|A| + e)^2

gv_grm_he is held to the restatement's he() evaluated on the library's own gv_grm_apply output within 1e-10 max(1, |value|) (the same
arithmetic; tests/test_grm_he_cpu.py shows the formulas are that well conditioned here), and to the pure-numpy reference within twice
he_bound at eps = (N + M + 32) 2^-53, the factor covering second-order terms.

The worst measured ratios are recorded in DESIGN.md section 30."""
import numpy as np
import pytest

import grm_he_restatement as hr
import grm_restatement as gr
from gvamp_amd import capi, synth

pytestmark = pytest.mark.gpu
CASES = gr.CASES
HE_CASES = ("ragged", "pedigree", "deep")
SEED = {"ragged": 101, "pedigree": 102, "deep": 103}
COLS = (1, 3, 8, 32)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")
    monkeypatch.delenv("GV_GRM_PART_MB", raising=False)


def _shard(cs, mode=1, layout=2):
    sh = capi.Shard(cs["N"], cs["M"], device=0)
    sh.set_layout(False, layout)
    sh.set_kernel_mode(mode)
    sh.upload_bed(cs["bed"])
    return sh


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same(got, want):
    return all(np.array_equal(_bits(g), _bits(w)) for g, w in zip(got, want))


def _units(N):
    """unit columns: in the first group, in the middle, in the (ragged) last group"""
    return (min(3, N - 1), N // 2, N - 1)


def _panel(name):
    """the shared 32-column panel of a case: 0 standard normal, 1 all zero, 2-4 unit columns, 5 the indicator of the all-missing
    individual (ragged; elsewhere of individual 0), 6 negative, 7 a 0 / 1 indicator, the rest standard normal of mixed scale"""
    cs = gr.case(name)
    N = cs["N"]
    rng = np.random.default_rng(77)
    W = rng.standard_normal((N, 32)) * 10.0 ** rng.integers(-3, 4, 32)[None, :]
    W[:, 1] = 0.0
    for c, j in zip((2, 3, 4), _units(N)):
        W[:, c] = 0.0
        W[j, c] = 1.0
    W[:, 5] = 0.0
    W[gr.MISSING_IND if name == "ragged" else 0, 5] = 1.0
    W[:, 6] = -np.abs(W[:, 6])
    W[:, 7] = rng.random(N) < 0.5
    return W


_SHARED = {}


def _shared(name):
    """computed once per case and left unchanged: the library's whole matrix (a, mc), the panel W and the chains of its 32 columns"""
    if name not in _SHARED:
        cs = gr.case(name)
        with _shard(cs) as sh:
            a, mc = sh.grm_block(0, cs["N"], 0, cs["N"])
        W = _panel(name)
        chain = hr.apply_chain(a, mc, W)
        for v in (a, mc, W) + chain:
            v.setflags(write=False)
        _SHARED[name] = dict(a=a, mc=mc, W=W, chain=chain)
    return _SHARED[name]


def _refs(name):
    """the numpy reference of the panel's product in long double and the three bounds, once per case"""
    sd = _shared(name)
    if "ref" not in sd:
        cs = gr.case(name)
        ref, (t0, _, _) = hr.apply_ref(cs, sd["W"])
        b1, b2 = hr.apply_bound(cs, gr.bound(cs), sd["W"])
        sd["ref"] = (ref, ((cs["N"] + 2) * 2.0 ** -53 * t0.astype(np.float64), b1, b2))
    return sd["ref"]


@pytest.mark.parametrize("mode", (1, 2))
@pytest.mark.parametrize("name", CASES)
def test_apply_is_bit_identical_to_the_chains_and_within_the_derived_bounds_of_the_reference(name, mode):
    cs, sd = gr.case(name), _shared(name)
    N, W = cs["N"], sd["W"]
    (r0, r1, r2), (b0, b1, b2) = _refs(name)
    nG = (N + 63) // 64
    with _shard(cs, mode=mode) as sh:
        for C in COLS:
            got = sh.grm_apply(W[:, :C])
            assert all(g.shape == (N, C) for g in got)
            assert _same(got, [x[:, :C] for x in sd["chain"]]), (name, mode, C)
            worst = []
            for g, ref, bnd in zip(got, (r0, r1, r2), (b0, b1, b2)):
                err = np.abs(g.astype(np.longdouble) - ref[:, :C]).astype(np.float64)
                assert np.all(err <= bnd[:, :C]), (name, mode, C)
                with np.errstate(divide="ignore", invalid="ignore"):
                    worst.append(float(np.nanmax(np.where(bnd[:, :C] > 0, err / bnd[:, :C], 0.0))))
            print(name, mode, C, "largest error / bound of g0, g1, g2:", worst)
            info = sh.grm_info()
            assert info["passes"] == 1 and info["blocks_computed"] == info["block_pairs"] == nG * (nG + 1) // 2
            assert info["pairs"] == N * (N - 1) // 2 and info["useful_macs"] == float(info["counting_markers"]) * info["pairs"]
            assert info["counting_markers"] == int(cs["counting"].sum()) and info["scratch_bytes"] > 0 and info["seconds"] > 0
        again = sh.grm_apply(W)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(again, sh.grm_apply(W)))          # two calls, the same bytes
        only = sh.grm_apply(W[:, :3], want=(False, True, False))                                 # outputs may be left out
        assert only[0] is None and only[2] is None and np.array_equal(_bits(only[1]), _bits(sd["chain"][1][:, :3]))


@pytest.mark.parametrize("name", CASES)
def test_the_columns_that_probe_the_edges(name):
    cs, sd = gr.case(name), _shared(name)
    N, a, mc = cs["N"], sd["a"], sd["mc"]
    with _shard(cs) as sh:
        g0, g1, g2 = sh.grm_apply(sd["W"][:, :8])
    for g in (g0, g1, g2):
        assert np.all(_bits(g[:, 1]) == 0)                       # an all-zero column: exact +0.0
    for c, j in zip((2, 3, 4), _units(N)):                       # a unit column returns column j of the operator
        on = (mc[:, j] > 0) & (np.arange(N) != j)
        col = np.where(on, a[:, j], 0.0)
        assert np.array_equal(_bits(g1[:, c]), _bits(col)), (name, j)
        assert np.array_equal(_bits(g2[:, c]), _bits(col * col)) and np.array_equal(g0[:, c], on.astype(np.float64))
        assert g0[j, c] == 0 and g1[j, c] == 0 and g2[j, c] == 0
    if name == "ragged":
        m = gr.MISSING_IND
        assert np.all(mc[m] == 0)
        for g in (g0, g1, g2):
            assert np.all(_bits(g[:, 5]) == 0)                   # the all-missing individual alone: zeros everywhere
            assert np.all(_bits(g[m, :]) == 0)                   # and nothing reaches it
        for c, j in zip((2, 3, 4), _units(N)):
            assert g0[m, c] == 0 and np.count_nonzero(g0[:, c]) == N - 2


def test_a_column_alone_and_at_position_31_of_a_batch_gives_the_same_bits():
    cs, sd = gr.case("ragged"), _shared("ragged")
    W = sd["W"]
    with _shard(cs) as sh:
        alone = sh.grm_apply(W[:, 9])
        moved = np.concatenate([W[:, 10:], W[:, :9], W[:, 9:10]], axis=1)
        assert moved.shape[1] == 32
        batch = sh.grm_apply(moved)
    assert _same([g[:, 0] for g in alone], [x[:, 9] for x in sd["chain"]])
    assert _same([g[:, 31] for g in batch], [x[:, 9] for x in sd["chain"]])
    assert _same([g[:, 0] for g in batch], [x[:, 10] for x in sd["chain"]])


def test_passes_forced_by_a_small_budget_change_no_bit_and_a_budget_below_one_block_is_refused(monkeypatch):
    cs, sd = gr.case("ragged"), _shared("ragged")
    N, W = cs["N"], sd["W"][:, :8]
    nG = (N + 63) // 64
    unit = 2 * 3 * 64 * 8 * 8                       # both terms of one block, three operators, 8 columns of 8 bytes
    unit9 = unit // 8 * 9                           # ... of the 9 columns of three traits
    assert nG == 16
    for g, tiles in ((5, 4), (4, 4), (1, 16)):      # tile edge in groups -> tiles per side (5: a ragged last tile), for 8 and 9 columns
        monkeypatch.setenv("GV_GRM_PART_MB", "%.6f" % ((g * g * unit9 + 600) / 2.0 ** 20))
        with _shard(cs) as sh:
            monkeypatch.delenv("GV_GRM_PART_MB")
            got = sh.grm_apply(W)
            info = sh.grm_info()
            assert info["passes"] == tiles * (tiles + 1) // 2 >= 3 and info["blocks_computed"] == info["block_pairs"] == nG * (nG + 1) // 2
            assert _same(got, [x[:, :8] for x in sd["chain"]]), g
            one = sh.grm_apply(W[:, :1])            # an eighth of the columns: eight times the blocks a tile
            assert sh.grm_info()["passes"] <= info["passes"] and _same(one, [x[:, :1] for x in sd["chain"]])
            he = sh.grm_he(hr.traits(cs, SEED["ragged"]))
            assert sh.grm_info()["passes"] == info["passes"]
        with _shard(cs) as sh:
            assert he.tobytes() == sh.grm_he(hr.traits(cs, SEED["ragged"])).tobytes()
    monkeypatch.setenv("GV_GRM_PART_MB", "%.6f" % ((unit - 600) / 2.0 ** 20))
    with _shard(cs) as sh:
        monkeypatch.delenv("GV_GRM_PART_MB")
        out = np.full((N, 8), -3.0)
        assert sh.L.gv_grm_apply(sh.h, None, 8, capi._dp(np.ascontiguousarray(W)), capi._dp(out), None, None) != 0
        assert b"GV_GRM_PART_MB" in sh.L.gv_last_error(sh.h) and b"cannot hold" in sh.L.gv_last_error(sh.h) and np.all(out == -3.0)
        assert _same(sh.grm_apply(W[:, :4]), [x[:, :4] for x in sd["chain"]])          # (half the columns fit)
    for bad in ("0", "-3", "lots", "nan"):
        monkeypatch.setenv("GV_GRM_PART_MB", bad)
        with pytest.raises(capi.GvError, match="GV_GRM_PART_MB"):
            capi.Shard(N, cs["M"], device=0)


def test_a_use_mask_with_edges_off_the_4_and_64_marker_boundaries():
    cs, sd = gr.case("ragged"), _shared("ragged")
    N, M, W = cs["N"], cs["M"], sd["W"][:, :8]
    u = np.ones(M, dtype=np.uint8)
    u[61:67] = 0
    u[M - 1] = 0
    u[[2, 255, 256]] = 0
    with _shard(cs) as sh:
        a, mc = sh.grm_block(0, N, 0, N, use=u)
        got = sh.grm_apply(W, use=u)
        assert sh.grm_info()["counting_markers"] == int(gr.grm(cs["geno"], u)["counting"].sum())
    assert _same(got, hr.apply_chain(a, mc, W))
    assert not _same(got, [x[:, :8] for x in sd["chain"]])


def test_a_call_leaves_the_products_the_grm_and_the_kinship_of_the_context_unchanged():
    cs, sd = gr.case("ragged"), _shared("ragged")
    N, M = cs["N"], cs["M"]
    rng = np.random.default_rng(9)
    x = rng.standard_normal(M)
    with capi.Shard(N, M, device=0) as sh:
        sh.set_layout(False, 2)
        sh.upload_bed(cs["bed"])
        sh.compute_markers_statistics()
        p = np.zeros(4 * sh.mbytes)
        p[:N] = rng.standard_normal(N)

        def state():
            return (sh.Ax(x), sh.ATx(p)) + sh.grm_block(5, 100, 300, 50) + sh.grm_pairs(0.1)[:4] + sh.king_block(5, 100, 300, 50)

        before = state()
        sh.grm_apply(sd["W"])
        sh.grm_he(hr.traits(cs, SEED["ragged"]))
        after = state()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))


def test_every_refusal_is_raised_with_its_message_and_writes_nothing():
    cs = gr.case("edge")
    N, M = cs["N"], cs["M"]
    w = np.random.default_rng(1).standard_normal((N, 2))
    calls = (lambda s: s.grm_apply(w), lambda s: s.grm_he(w))
    with capi.Shard(N, M, device=0) as sh:        # methylation data
        sh.synth_meth(3)
        for call in calls:
            with pytest.raises(capi.GvError, match="meth"):
                call(sh)
    for dtype, bits in ((np.uint8, 8), (np.uint16, 16)):       # compact dosage data, by width
        with capi.Shard(N, M, device=0) as sh:
            sh.upload_dosage(synth.synth_dosage(N, M, 2, bits).astype(dtype), 1.0 / 127.0)
            for call in calls:
                with pytest.raises(capi.GvError, match="%d-bit codes" % bits):
                    call(sh)
    with capi.Shard(N, M, device=0) as sh:        # raw rows only
        sh.set_layout(True, 0)
        sh.upload_bed(cs["bed"])
        for call in calls:
            with pytest.raises(capi.GvError, match="raw rows alone"):
                call(sh)
    with _shard(cs, layout=1) as sh:              # two stripe sets: the tile layout is the way out
        for call in calls:
            with pytest.raises(capi.GvError, match="two stripe sets.*tile layout"):
                call(sh)
    with _shard(cs) as sh:
        sh.force_multi(1)                         # a job of more than one rank
        for call in calls:
            with pytest.raises(capi.GvError, match="more than one rank"):
                call(sh)
        sh.force_multi(0)
        for C in (0, 33):
            with pytest.raises(capi.GvError, match="outside 1 .. 32"):
                sh.grm_apply(np.zeros((N, C)))
        with pytest.raises(capi.GvError, match="at least one"):
            sh.grm_he(np.zeros((N, 0)))
        L, dp = sh.L, capi._dp
        out = np.full((N, 2), -3.0)
        res = (capi.HeResult * 2)()
        res[0].n_ind = res[1].n_ind = -7
        assert L.gv_grm_apply(sh.h, None, 2, None, dp(out), None, None) != 0 and b"w is NULL" in L.gv_last_error(sh.h)
        assert L.gv_grm_apply(sh.h, None, 2, dp(w), None, None, None) != 0 and b"all NULL" in L.gv_last_error(sh.h)
        assert L.gv_grm_he(sh.h, None, 2, None, res) != 0 and b"y is NULL" in L.gv_last_error(sh.h)
        assert L.gv_grm_he(sh.h, None, 2, dp(w), None) != 0 and b"res is NULL" in L.gv_last_error(sh.h)
        assert L.gv_grm_apply(None, None, 2, dp(w), dp(out), None, None) != 0 and L.gv_grm_he(None, None, 2, dp(w), res) != 0
        for bad in (np.nan, np.inf, -np.inf):
            wb = w.copy()
            wb[N - 1, 1] = bad
            assert L.gv_grm_apply(sh.h, None, 2, dp(wb), dp(out), dp(out), dp(out)) != 0
            assert b"is not finite" in L.gv_last_error(sh.h) and b"w[%d][1]" % (N - 1) in L.gv_last_error(sh.h)
        for bad in (np.inf, -np.inf):
            yb = w.copy()
            yb[3, 0] = bad
            assert L.gv_grm_he(sh.h, None, 2, dp(yb), res) != 0 and b"y[3][0] is infinite" in L.gv_last_error(sh.h)
        assert np.all(out == -3.0) and res[0].n_ind == -7 and res[1].n_ind == -7                   # nothing written
        assert sh.grm_he(w)["n_ind"].tolist() == [N, N]                                            # and the context still works


def _apply_in_chunks(sh, W):
    parts = [sh.grm_apply(W[:, c:c + 30]) for c in range(0, W.shape[1], 30)]
    return tuple(np.concatenate([p[k] for p in parts], axis=1) for k in range(3))


@pytest.mark.parametrize("name", HE_CASES)
def test_he_equals_the_restatement_on_the_librarys_product_and_the_reference_within_the_bound(name):
    cs = gr.case(name)
    N, M = cs["N"], cs["M"]
    Y = hr.traits(cs, SEED[name])
    assert np.isnan(Y[:, 1]).sum() > 0 and not np.isnan(Y[:, [0, 2]]).any()
    with _shard(cs) as sh:
        got = sh.grm_he(Y)
        info = sh.grm_info()
        same = hr.he_traits(Y, lambda W: _apply_in_chunks(sh, W))
        wide = np.concatenate([Y[:, [2, 1]], np.random.default_rng(4).standard_normal((N, 10)), Y[:, [0]]], axis=1)
        batch = sh.grm_he(wide)                     # 13 traits: two calls of the product
        binfo = sh.grm_info()
        alone = [sh.grm_he(Y[:, c]) for c in range(3)]
    nG = (N + 63) // 64
    assert info["passes"] == 1 and info["blocks_computed"] == nG * (nG + 1) // 2 and info["seconds"] > 0
    assert binfo["passes"] == 2 and binfo["blocks_computed"] == nG * (nG + 1)
    assert got.dtype == capi.HE_DTYPE and len(got) == 3 and len(batch) == 13
    for c, pos in ((0, 12), (1, 1), (2, 0)):        # a trait of a batch of 13 equals the same trait alone
        assert batch[pos:pos + 1].tobytes() == alone[c].tobytes() == got[c:c + 1].tobytes(), (name, c)
    ref = hr.he_traits(Y, lambda W: tuple(x.astype(np.float64) for x in hr.apply_ref(cs, W)[0]))
    eps = (N + M + 32) * 2.0 ** -53
    for c in range(3):
        for f in hr.FIELDS:
            v = float(same[c][f])
            print(name, c, f, got[c][f], "restatement on the library's product", v, "reference", float(ref[c][f]))
            assert abs(got[c][f] - v) <= 1e-10 * max(1.0, abs(v)), (name, c, f)
        assert got[c]["n_ind"] == int((~np.isnan(Y[:, c])).sum()) and got[c]["n_pairs"] == ref[c]["n_pairs"]
        bound = hr.he_bound(cs, Y[:, c], eps)
        for f in hr.DERIVED:
            err = abs(got[c][f] - float(ref[c][f]))
            print(name, c, f, "error / (2 bound)", err / (2 * bound[f]))
            assert err <= 2 * bound[f], (name, c, f)
    assert np.isfinite(got["se_jack"]).all()


def test_he_gives_nan_for_a_constant_trait_and_for_fewer_than_three_individuals():
    cs = gr.case("pedigree")
    N = cs["N"]
    Y = np.random.default_rng(6).standard_normal((N, 5))
    Y[:, 1] = 4.0                                   # constant
    Y[:, 2] = np.nan
    Y[[3, 40], 2] = (1.0, 2.0)                      # two individuals: one pair
    Y[:, 3] = np.nan                                # nobody
    with _shard(cs) as sh:
        got = sh.grm_he(Y)                          # return code 0: no exception
        alone = sh.grm_he(Y[:, 0])
    assert got["n_ind"].tolist() == [N, N, 2, 0, N] and got["n_pairs"].tolist()[2:4] == [1, 0]
    assert got["n_pairs"][1] == got["n_pairs"][0] and got["sum_a"][1] == got["sum_a"][0]          # the matrix's share is still reported
    for c in (1, 2, 3):
        assert all(np.isnan(got[c][f]) for f in hr.DERIVED), (c, got[c])
    for c in (0, 4):
        assert all(np.isfinite(got[c][f]) for f in hr.DERIVED), (c, got[c])
    assert got[0:1].tobytes() == alone.tobytes()
