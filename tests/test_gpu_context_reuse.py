"""A context that is REUSED -- another mask, another alpha_scale, another data set, layout, kernel mode, data kind, option or set of
dimensions on the same gv_ctx -- must answer exactly as a context that was created for the new state and never saw the old one.

A gv_ctx keeps derived state with hand-written validity rules: mave / msig / counts (have_stats), the people statistics
(have_people), the window Grams and inverses of the LD preconditioner, the dosage mu / cnt, the fixed-point scratch of dosage
route 1, the score scratch, the decomposition picks, the run-ahead hints of the device-resident CG, and the caller's own vectors.
A stale piece gives a finite, plausible and wrong answer, so every case here

  1. asks the consumers on the reused context in the OLD state first (every cache is warm),
  2. makes only the calls include/gvamp.h documents for the change (its table beside gv_set_mask),
  3. compares every output array of every consumer with the fresh context's by np.array_equal -- no tolerance anywhere: integer
     sums, fixed fp64 summation orders and no atomics make the bits reproducible, and the products are independent of the tuner's
     decomposition pick (GV_TUNE_CACHE=0 keeps a pick persisted by another run out of it, as in test_gpu_bed_fixed.py),
  4. and first shows that the fresh OLD and fresh NEW answers differ, so that a stale answer could not pass.  Where the contract
     itself lets the two states agree for a consumer -- the statistics and products under a preconditioner kind, the statistics
     under a kernel mode or a dosage route, LD correlations under alpha_scale (r_jk is invariant under a rescaling of the
     columns) -- the (changed input, consumer) pair is listed in MAY_AGREE with its reason; such a leg is still compared.

The reference is always the fresh context: what it computes is held to the oracle and the restatements by the rest of the suite.
A new cached field of gv_ctx belongs into a consumer (or a transition) of this file.

Shapes: N = 1203 is ragged modulo 4, 16, 64 and 256 and spans two 1024-individual steps; M = 650 spans eleven 64-marker row groups
and is ragged; methylation data take M = 130; the second set of dimensions is (515, 257).
"""
import numpy as np
import pytest

from gvamp_amd import capi, synth

pytestmark = pytest.mark.gpu
N0, M0, M_METH = 1203, 650, 130
N1, M1 = 515, 257
TAU, GAM2 = 2.0, 0.5
_CACHE = {}
_COUNT = {"arrays": 0, "cases": 0}


@pytest.fixture(autouse=True)
def _no_tune_cache(monkeypatch):
    monkeypatch.setenv("GV_TUNE_CACHE", "0")


@pytest.fixture(scope="module", autouse=True)
def _report_total():
    yield
    print("\ncontext reuse: %d output arrays of %d (state, consumer) pairs compared bit for bit with a fresh context"
          % (_COUNT["arrays"], _COUNT["cases"]))


# ---- states -----------------------------------------------------------------------------------------------------------------------
DEFAULT = dict(kind="bed", seed=1, masked=False, alpha=1.0, layout=2, mode=1, route=0, missing=False, ld_dosage=0, precond=(0, 128),
               anchor=False, dims=(N0, M0))


def S(**kw):
    st = dict(DEFAULT)
    st.update(kw)
    if st["kind"] == "meth" and "dims" not in kw:
        st["dims"] = (N0, M_METH)
    return st


def _key(st):
    return tuple(sorted(st.items()))


def _memo(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


def na_mask(N, with_na):
    """(mask4 nibbles, nonas): every 7th individual from 3 on has no phenotype (the pattern of test_gpu_meth.py)"""
    na = np.ones(N)
    if with_na:
        na[3::7] = 0.0
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    for n in np.nonzero(na)[0]:
        m4[n >> 2] |= 1 << (n & 3)
    return m4, int(na.sum())


def _data(st):
    (N, M), kind, seed = st["dims"], st["kind"], st["seed"]

    def make():
        if kind == "bed":
            return synth.synth_bed(N, M, seed=seed, miss_ppm=10000)
        if kind == "meth":
            return synth.synth_meth(N, M, seed)
        bits = 8 if kind == "d8" else 16
        if st["missing"]:
            return synth.synth_dosage_na(N, M, seed, bits, 10000)
        return synth.synth_dosage(N, M, seed, bits)
    return _memo(("data", N, M, kind, seed, st["missing"]), make)


def _upload(sh, st):
    d = _data(st)
    if st["kind"] == "bed":
        sh.upload_bed(d)
    elif st["kind"] == "meth":
        sh.upload_meth(d)
    else:
        sh.upload_dosage(d, 1.0 / 127.0 if st["kind"] == "d8" else 1.0 / 16384.0, missing=st["missing"])


def _fresh(st):
    """a context that was only ever given state st"""
    N, M = st["dims"]
    sh = capi.Shard(N, M, anchor=st["anchor"])
    if not st["anchor"]:
        sh.set_layout(False, st["layout"])
    sh.set_kernel_mode(st["mode"])
    sh.set_dosage_route(st["route"])
    sh.set_ld_dosage(st["ld_dosage"])
    _upload(sh, st)
    if st["masked"]:
        sh.set_mask(*na_mask(N, True))
    sh.compute_markers_statistics(st["alpha"])
    sh.set_cg_precond(*st["precond"])
    return sh


def _move(sh, a, b, stats=True):
    """state a -> state b on a live context, by the calls the table of include/gvamp.h names and no others"""
    upload = mask = False
    dims = a["dims"] != b["dims"]
    if not dims and a["kind"] == b["kind"] and b["kind"] in ("d8", "d16") and a["missing"] != b["missing"]:
        dims = True          # gv_set_dosage_missing is refused under resident codes of the other setting: gv_set_dims drops them
    if dims:
        sh.set_dims(*b["dims"])                              # the data set, the mask and the statistics go
        upload, mask = True, b["masked"]
    elif a["masked"] != b["masked"]:
        mask = True
    if a["layout"] != b["layout"]:
        sh.set_layout(False, b["layout"])
        upload = True
    if a["mode"] != b["mode"]:
        sh.set_kernel_mode(b["mode"])
    if a["route"] != b["route"]:
        sh.set_dosage_route(b["route"])
    if a["ld_dosage"] != b["ld_dosage"]:
        sh.set_ld_dosage(b["ld_dosage"])
    if (a["kind"], a["seed"], a["missing"]) != (b["kind"], b["seed"], b["missing"]):
        upload = True
    if upload:
        _upload(sh, b)
    if mask:
        sh.set_mask(*na_mask(b["dims"][0], b["masked"]))
    if stats and (upload or mask or a["alpha"] != b["alpha"]):
        sh.compute_markers_statistics(b["alpha"])
    else:
        stats = False
    if a["precond"] != b["precond"]:
        sh.set_cg_precond(*b["precond"])
    return stats          # new marker statistics were computed


# ---- operands (fixed seeds; uploaded anew on every context and at every ask) ------------------------------------------------------
def _ops(N, M):
    def make():
        rng = np.random.default_rng(20240611)
        n4 = 4 * ((N + 3) // 4)

        def nvec(scale=1.0):
            v = np.zeros(n4)
            v[:N] = scale * rng.standard_normal(N)
            return v
        chrom = np.where(np.arange(M) < M // 2, 1, 2).astype(np.int32)
        pos = 1000.0 * np.concatenate([np.arange(M // 2), np.arange(M - M // 2)])          # 1 kb apart, two chromosomes
        return dict(x=rng.standard_normal(M), x2=1e-3 * rng.standard_normal(M), v=rng.standard_normal(M),
                    u=np.where(rng.random(M) < 0.5, -1.0, 1.0) / np.sqrt(M), p=nvec(), p2=nvec(7.0), y=nvec(), z1=nvec(0.3),
                    x1=0.05 * rng.standard_normal(M), W=rng.standard_normal((5, M)), chrom=chrom, pos=pos,
                    pv=rng.random(M) ** 4, probs=np.array([0.7, 0.2, 0.1]), vars=np.array([0.0, 1e-2, 1.0]) * N)
    return _memo(("ops", N, M), make)


def _cg(sh, o, out, tag=""):
    for den in (1, 0):
        v, mu = sh.vecM(o["v"] if den else o["u"]), sh.vecM()
        st, rr = sh.cg_solve(v, None, TAU, GAM2, den, 30, mu)
        out["%scg%d_mu" % (tag, den)] = mu.download()
        out["%scg%d_iters" % (tag, den)] = np.array([st.iters, st.converged, st.n_relres])
        out["%scg%d_relres" % (tag, den)] = rr
        v.free()
        mu.free()


# ---- consumers: shard -> dict of arrays -----------------------------------------------------------------------------------------------
def c_stats(sh, st):
    mave, msig = sh.marker_stats()
    out = dict(mave=mave, msig=msig)
    if st["kind"] in ("d8", "d16"):
        out["cnt"] = sh.marker_counts()
    return out


def c_products(sh, st):
    o = _ops(sh.N, sh.M)
    out = dict(Ax=sh.Ax(o["x"]), ATx=sh.ATx(o["p"]))
    xa, xb, za, zb = sh.vecM(o["x"]), sh.vecM(o["x2"]), sh.vecN(), sh.vecN()
    sh.ax2_dev(xa, xb, za, zb)
    pa, pb, wa, wb = sh.vecN(o["p"]), sh.vecN(o["p2"]), sh.vecM(), sh.vecM()
    sh.atx2_dev(pa, pb, wa, wb)
    lm = sh.vecM()
    sh.lmmse_mult(xa, TAU, GAM2, lm)
    out.update(ax2_a=za.download(), ax2_b=zb.download(), atx2_a=wa.download(), atx2_b=wb.download(), lmmse=lm.download())
    for v in (xa, xb, za, zb, pa, pb, wa, wb, lm):
        v.free()
    return out


def c_cg(sh, st):
    out = {}
    _cg(sh, _ops(sh.N, sh.M), out)
    return out


def c_precond(sh, st):
    """the state carries gv_set_cg_precond(1, W): the solves use the window Grams and their inverses"""
    assert sh.precond_info()["kind"] == 1
    o, out = _ops(sh.N, sh.M), {}
    _cg(sh, o, out, "pc_")
    r, z = sh.vecM(o["x"]), sh.vecM()
    sh.precond_apply(TAU, GAM2, r, z)
    out["pc_apply"] = z.download()
    sh.precond_apply(0.7, 1.9, r, z)                 # another (tau, gam2): the inverses are factorised again
    out["pc_apply2"] = z.download()
    out["pc_fallback"] = np.array([sh.precond_info()["fallback_windows"]])
    r.free()
    z.free()
    return out


def _aat_solves(sh, out):
    o = _ops(sh.N, sh.M)
    vn, mu = sh.vecN(o["p"]), sh.vecN()
    st, rr = sh.cg_solve_aat(vn, None, TAU, 1.1, 30, mu)
    out.update(aat_mu=mu.download(), aat_iters=np.array([st.iters, st.converged, st.n_relres]), aat_relres=rr)
    du, n2, at2, m2 = sh.vecM(o["u"]), sh.vecN(), sh.vecM(), sh.vecM()
    (sa, ra), (sb, rb) = sh.cg_solve_aat2(vn, None, du, TAU, 1.1, 30, n2, at2, m2)
    out.update(aat2_mu_a=n2.download(), aat2_at_mu_a=at2.download(), aat2_mu_b=m2.download(),
               aat2_iters=np.array([sa.iters, sa.converged, sb.iters, sb.converged]), aat2_relres_a=ra, aat2_relres_b=rb)
    for v in (vn, mu, du, n2, at2, m2):
        v.free()
    return out


def c_aat(sh, st):
    pm, ps, pn = sh.compute_people_statistics()
    return _aat_solves(sh, dict(people_mave=pm, people_msig=ps, people_numb=pn))


def c_assoc(sh, st):
    o, out = _ops(sh.N, sh.M), {}
    z1, y, x1 = sh.vecN(o["z1"]), sh.vecN(o["y"]), sh.vecM(o["x1"])
    if st["kind"] == "bed":
        out["pvals_loo"] = sh.pvals_calc(z1, y, x1)
        out["pvals_loco"] = sh.pvals_calc(z1, y, x1, o["chrom"])
    for name, res in (("loo", sh.assoc_calc(z1, y, x1)), ("loco", sh.assoc_calc(z1, y, x1, o["chrom"]))):
        for k, a in res.items():
            out["assoc_%s_%s" % (name, k)] = a
    for v in (z1, y, x1):
        v.free()
    return out


def c_ld(sh, st):
    o, out = _ops(sh.N, sh.M), {}
    for adj in (False, True):
        l2, npairs = sh.ld_scores(100, adjusted=adj)
        out["ld_l2_adj%d" % adj], out["ld_n_adj%d" % adj] = l2, npairs
    out["ld_band"] = sh.ld_band(100, 10, 50)
    if st["kind"] == "bed":
        l2, npairs = sh.ld_scores_pos(o["pos"], 60000.0, chrom=o["chrom"])
        out["ldpos_l2"], out["ldpos_n"] = l2, npairs
        idx, n_index = sh.ld_clump(o["pos"], 60000.0, o["pv"], 1e-2, 0.5, 1e-3, chrom=o["chrom"])
        assert n_index > 3 and np.any((idx >= 0) & (idx != np.arange(sh.M))), "the clumping inputs must form clumps with members"
        out["clump_index_of"], out["clump_n"] = idx, np.array([n_index])
    return out


def c_score(sh, st):
    out = dict(score=sh.score(_ops(sh.N, sh.M)["W"]))
    if st["kind"] == "bed" and st["mode"] == 1 and st["layout"] == 2 and not st["anchor"]:
        assert sh.score_info()["path"] == "kernel"           # the tile layout in kernel mode 1 takes k_score
    return out


CONSUMERS = dict(stats=c_stats, products=c_products, cg=c_cg, precond=c_precond, aat=c_aat, assoc=c_assoc, ld=c_ld, score=c_score)
GROUPS_OF = dict(bed=("stats", "products", "cg", "precond", "aat", "assoc", "ld", "score"),
                 d8=("stats", "products", "cg", "precond", "assoc", "ld", "score"),
                 d16=("stats", "products", "cg", "assoc", "score"), meth=("stats", "products", "cg", "score"))


def _for_group(st, group):
    """the state as the consumer group needs it: the LD preconditioner set for `precond`, gv_set_ld_dosage on for LD on dosage codes"""
    st = dict(st)
    if group == "precond" and st["precond"][0] == 0:
        st["precond"] = (1, 64)
    if group in ("precond", "ld") and st["kind"] == "d8":
        st["ld_dosage"] = 1
    return st


def _fresh_out(st, group):
    def run():
        with _fresh(st) as sh:
            return CONSUMERS[group](sh, st)
    return _memo(("fresh", _key(st), group), run)


def _differs(a, b):
    return [k for k in a if k not in b or a[k].shape != b[k].shape or not np.array_equal(a[k], b[k], equal_nan=True)]


def _equal_or_fail(what, got, ref):
    assert set(got) == set(ref), (what, sorted(set(got) ^ set(ref)))
    bad = _differs(got, ref)
    _COUNT["arrays"] += len(ref)
    _COUNT["cases"] += 1
    assert not bad, "%s: the reused context differs from a fresh one in %s" % (what, ", ".join(
        "%s (%d of %d entries)" % (k, int(np.sum(got[k] != ref[k])) if got[k].shape == ref[k].shape else -1, ref[k].size) for k in bad))


# (changed input, consumer group) pairs for which the contract lets the old and the new state give the same bits: no input can be
# chosen that makes a stale answer of such a pair visible, so a leg that changes nothing else is compared without that assertion
MAY_AGREE = {
    ("alpha", "ld"): "r_jk is invariant under a rescaling of the columns: alpha_scale cannot reach an LD correlation",
    ("mode", "stats"): "the marker statistics are exact counts finished by one formula in every kernel family",
    ("route", "stats"): "statistics keep their kernels on either dosage route",
    ("ld_dosage", "stats"): "gv_set_ld_dosage changes no statistic",
    ("ld_dosage", "products"): "... no product",
    ("ld_dosage", "cg"): "... and no scalar-preconditioned solve",
    ("precond", "stats"): "the preconditioner enters the M-space CG solves only",
    ("precond", "products"): "the same",
}


def _may_agree(a, b, group):
    return all((f, group) in MAY_AGREE for f in a if a[f] != b[f])


def _walk(name, states, group):
    """the consumers on ONE context walked through `states`; at every state the answer is the fresh context's"""
    states = [_for_group(st, group) for st in states]
    fn = CONSUMERS[group]
    with _fresh(states[0]) as sh:
        got = fn(sh, states[0])                              # state A: every cache warm
        _equal_or_fail("%s/%s state 0" % (name, group), got, _fresh_out(states[0], group))
        for i in range(1, len(states)):
            a, b = states[i - 1], states[i]
            fa, fb = _fresh_out(a, group), _fresh_out(b, group)
            changed = _differs(fa, fb)
            if not _may_agree(a, b, group):
                assert changed, "%s/%s leg %d: the fresh answers of the two states are identical -- a stale answer would pass" % (name, group, i)
            print("%s/%s leg %d: %d of %d output arrays differ between the two fresh states" % (name, group, i, len(changed), len(fb)))
            moved = _move(sh, a, b)
            if group == "aat" and moved:
                _stale_people_refused(sh, fb)
            got = fn(sh, b)
            _equal_or_fail("%s/%s leg %d" % (name, group, i), got, fb)


def _stale_people_refused(sh, fresh):
    """new marker statistics, no new people statistics: the N-space solvers refuse.  (Without the have_people flag they answered
    from the previous state's per-individual sums: the comparison below then shows the stale answer before the refusal is missed.)"""
    try:
        stale = _aat_solves(sh, {})
    except capi.GvError as e:
        assert "gv_people_stats" in str(e), str(e)
        return
    bad = _differs(stale, {k: fresh[k] for k in stale})
    raise AssertionError("the N-space solvers accepted stale people statistics; against a fresh context %d of %d of their outputs differ: %s"
                         % (len(bad), len(stale), ", ".join(bad)))


# ---- T1 - T3: every consumer the kind admits -----------------------------------------------------------------------------------
def _t123(kind):
    return dict(mask=[S(kind=kind), S(kind=kind, masked=True)],                         # T1: set_mask, marker statistics
                alpha=[S(kind=kind), S(kind=kind, alpha=0.3)],                             # T2: marker statistics(0.3)
                data=[S(kind=kind, seed=1), S(kind=kind, seed=2)])                         # T3: upload, marker statistics


T123 = [(t, kind, g) for kind in ("bed", "d8", "d16", "meth") for t in ("mask", "alpha", "data") for g in GROUPS_OF[kind]]


@pytest.mark.parametrize("transition,kind,group", T123)
def test_mask_alpha_and_data_set(transition, kind, group):
    _walk(transition, _t123(kind)[transition], group)


# ---- T4 - T9: the statistics, the products, the solves and whatever the transition is about -------------------------------------
BASE = ("stats", "products", "cg")
CHAINS = {
    # T4: tile layout -> two stripe sets -> tile layout (set_layout, upload, statistics); the upload brings the other data set along
    "layout": (BASE + ("score", "aat", "ld"), [S(layout=2, seed=1), S(layout=1, seed=2), S(layout=2, seed=1)]),
    # T5: kernel mode 1 -> 2 -> 1 by gv_set_kernel_mode alone; and 1 -> 0 -> 1 on a context with the raw rows resident
    "mode": (BASE + ("score",), [S(mode=1), S(mode=2), S(mode=1)]),
    "mode0": (BASE, [S(anchor=True, layout=1, mode=1), S(anchor=True, layout=1, mode=0), S(anchor=True, layout=1, mode=1)]),
    # T6: bed -> 8-bit dosage -> methylation (other dimensions) -> bed
    "kind": (BASE + ("score",), [S(kind="bed"), S(kind="d8"), S(kind="meth"), S(kind="bed", seed=2)]),
    # T7: the options of 8-bit dosage codes
    "route": (BASE, [S(kind="d8"), S(kind="d8", route=1), S(kind="d8", route=0), S(kind="d8", route=1, seed=2)]),
    "missing": (BASE + ("assoc",), [S(kind="d8"), S(kind="d8", missing=True, seed=2), S(kind="d8")]),
    "lddosage": (BASE, [S(kind="d8"), S(kind="d8", ld_dosage=1), S(kind="d8")]),
    # T8: preconditioner kind 0 -> 1 (W = 64) -> 1 (W = 32) -> 0, by gv_set_cg_precond alone
    "precond": (BASE, [S(), S(precond=(1, 64)), S(precond=(1, 32)), S()]),
    "precond_d8": (BASE, [S(kind="d8", ld_dosage=1), S(kind="d8", ld_dosage=1, precond=(1, 64)), S(kind="d8", ld_dosage=1, precond=(1, 32)),
                          S(kind="d8", ld_dosage=1)]),
    # T9: other dimensions and back (gv_set_dims, upload, statistics; every vector allocated anew)
    "dims": (BASE + ("score", "aat", "precond"), [S(), S(dims=(N1, M1), seed=2), S()]),
}
T49 = [(name, g) for name, (groups, _) in CHAINS.items() for g in groups]


@pytest.mark.parametrize("name,group", T49)
def test_layout_mode_kind_options_and_dimensions(name, group):
    _walk(name, CHAINS[name][1], group)


def test_the_windows_of_the_preconditioner_follow_its_kind_and_width():
    """T8 for the consumer it is about: precond_apply and the preconditioned solves at W = 64, W = 32 and W = 64 again on one context"""
    _walk("precond_w", [S(precond=(1, 64)), S(precond=(1, 32)), S(precond=(1, 64), masked=True)], "precond")


def test_ld_of_dosage_codes_switched_off_and_on_again():
    """T7 for the consumers gv_set_ld_dosage is about: LD scores, the band and the Grams behind the preconditioner"""
    st = _for_group(S(kind="d8", precond=(1, 64)), "precond")
    with _fresh(st) as sh:
        c_precond(sh, st), c_ld(sh, st)
        sh.set_ld_dosage(0)
        for fn in (c_ld, c_precond):
            with pytest.raises(capi.GvError, match="compact dosage data"):
                fn(sh, st)
        sh.set_ld_dosage(1)
        _equal_or_fail("ld_dosage off/on, precond", c_precond(sh, st), _fresh_out(st, "precond"))
        _equal_or_fail("ld_dosage off/on, ld", c_ld(sh, st), _fresh_out(st, "ld"))


# ---- refusals instead of stale answers ----------------------------------------------------------------------------------------------
REFUSALS = [(kind, ev, g) for kind in ("bed", "d8", "d16", "meth") for ev in ("mask", "data") for g in GROUPS_OF[kind]
            # LD scores of dosage codes form their own integer statistics from the codes and the mask: they never read mave / msig,
            # so without marker statistics they answer, and correctly (compared below like everything else)
            if not (kind == "d8" and g == "ld")]


@pytest.mark.parametrize("kind,event,group", REFUSALS)
def test_after_a_new_mask_or_upload_every_consumer_waits_for_the_statistics(kind, event, group):
    a, b = [_for_group(st, group) for st in _t123(kind)[event]]
    fn = CONSUMERS[group]
    with _fresh(a) as sh:
        fn(sh, a)
        _move(sh, a, b, stats=False)
        with pytest.raises(capi.GvError, match=r"statistics|gv_marker_stats"):
            fn(sh, b)
        sh.compute_markers_statistics(b["alpha"])          # the missing call: the context is as good as new
        _equal_or_fail("refusal %s/%s/%s" % (kind, event, group), fn(sh, b), _fresh_out(b, group))


def test_ld_scores_of_dosage_codes_need_the_mask_alone():
    a, b = [_for_group(st, "ld") for st in _t123("d8")["mask"]]
    with _fresh(a) as sh:
        c_ld(sh, a)
        _move(sh, a, b, stats=False)
        _equal_or_fail("d8 ld after set_mask", c_ld(sh, b), _fresh_out(b, "ld"))


@pytest.mark.parametrize("event", ["mask", "alpha", "data"])
def test_the_nspace_solvers_wait_for_new_people_statistics(event):
    """gv_cg_solve_aat, gv_cg_solve_aat2 and gv_cg_solve_aat2w after new marker statistics: refused by name until gv_people_stats has
    run again, then equal to a fresh context"""
    a, b = _t123("bed")[event]
    o = _ops(N0, M0)
    with _fresh(a) as sh:
        c_aat(sh, a)
        _move(sh, a, b)
        vn, mu, du, at, mb = sh.vecN(o["p"]), sh.vecN(), sh.vecM(o["u"]), sh.vecM(), sh.vecM()
        sa, sb, ra, rb = capi.CgStats(), capi.CgStats(), np.zeros(30), np.zeros(30)
        byref, dp = capi.C.byref, capi._dp
        calls = (lambda: sh.cg_solve_aat(vn, None, TAU, 1.1, 30, mu), lambda: sh.cg_solve_aat2(vn, None, du, TAU, 1.1, 30, mu, at, mb),
                 lambda: sh._ck(sh.L.gv_cg_solve_aat2(sh.h, vn.h, None, du.h, TAU, 1.1, 30, mu.h, at.h, mb.h, byref(sa), byref(sb), dp(ra),
                                                      dp(rb), None, None)))
        for call in calls:
            with pytest.raises(capi.GvError, match="gv_people_stats"):
                call()
        _equal_or_fail("people statistics after %s" % event, c_aat(sh, b), _fresh_out(b, "aat"))


# ---- vectors belong to their context and to its current dimensions --------------------------------------------------------------
# The foreign / surviving vector is always the OUTPUT argument and always comes from the LARGER dimensions (1203 x 650 against
# 515 x 257): a missing guard would write inside the larger allocation, never past an end.
def _vector_calls(sh, big_n, big_m):
    o = _ops(sh.N, sh.M)
    x, p, v = sh.vecM(o["x"]), sh.vecN(o["p"]), sh.vecM(o["v"])
    return dict(ax_dev=lambda: sh.ax_dev(x, big_n), atx_dev=lambda: sh.atx_dev(p, big_m),
                cg_solve=lambda: sh.cg_solve(v, None, TAU, GAM2, 1, 30, big_m),
                denoise=lambda: sh.denoise(v, 1.3, o["probs"], o["vars"], big_m), copy_m=lambda: sh.copy(big_m, x),
                copy_n=lambda: sh.copy(big_n, p), score_dev=lambda: sh.score_dev([x], [big_n]))


def test_a_vector_of_another_context_is_refused():
    small = S(dims=(N1, M1), seed=2)
    for g in BASE + ("score",):                            # (the references first: at most two contexts are alive at a time)
        _fresh_out(small, g), _fresh_out(S(), g)
    with _fresh(S()) as big, _fresh(small) as sh:
        big_n, big_m = big.vecN(), big.vecM()
        for name, call in _vector_calls(sh, big_n, big_m).items():
            with pytest.raises(capi.GvError, match="another context") as ei:
                call()
            assert ("out" in str(ei.value) or "dst" in str(ei.value)), (name, str(ei.value))      # the argument is named
        assert np.all(big_n.download() == 0) and np.all(big_m.download() == 0)
        for g in BASE + ("score",):                        # both contexts work afterwards with their own vectors
            _equal_or_fail("after a foreign vector, small/" + g, CONSUMERS[g](sh, small), _fresh_out(small, g))
            _equal_or_fail("after a foreign vector, big/" + g, CONSUMERS[g](big, S()), _fresh_out(S(), g))


def test_a_vector_that_survived_set_dims_is_refused():
    small = S(dims=(N1, M1), seed=2)
    with _fresh(S()) as sh:
        old_n, old_m = sh.vecN(), sh.vecM()
        _move(sh, S(), small)
        for name, call in _vector_calls(sh, old_n, old_m).items():
            with pytest.raises(capi.GvError, match="earlier dimensions") as ei:
                call()
            assert ("out" in str(ei.value) or "dst" in str(ei.value)), (name, str(ei.value))
        for v in (old_n, old_m):
            with pytest.raises(capi.GvError, match="earlier dimensions"):
                v.download()
            v.free()
        for g in BASE + ("score",):
            _equal_or_fail("after a surviving vector/" + g, CONSUMERS[g](sh, small), _fresh_out(small, g))
