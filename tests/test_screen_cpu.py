"""The restatement of the marginal screen (tests/screen_restatement.py) without a GPU: held to
scipy.stats.pearsonr on the ragged case of tests/bed_fixed_restatement.py (NA phenotypes, missing genotypes, a monomorphic and an
all-missing marker), with its own float64-against-long-double deviation printed -- the yardstick tests/test_gpu_screen.py multiplies by
16 -- and the host-side preparation of capi.Shard.screen_prepare held to its definition."""
import numpy as np
import pytest
import scipy.stats as scipy_stats

import bed_fixed_restatement as bx
import screen_restatement as sr


@pytest.fixture(scope="module")
def ragged():
    cs = bx.case("ragged")
    Y, near, coll = sr.phenotypes(cs)
    ref = sr.screen(cs["bed"], cs["N"], cs["M"], cs["present"], Y)
    r64 = sr.screen(cs["bed"], cs["N"], cs["M"], cs["present"], Y, dtype=np.float64)
    return cs, Y, near, coll, ref, r64


def test_restatement_against_scipy_pearsonr(ragged):
    cs, Y, near, coll, ref, r64 = ragged
    pres, n = cs["present"], cs["nonas"]
    a, have = sr.genotypes(cs["bed"], cs["N"], cs["M"])
    assert ref["n"] == n and list(np.nonzero(ref["novar"])[0]) == [bx.MONO, bx.ALLMISS]
    worst_r = worst_p = 0.0
    for m in list(range(0, cs["M"], 11)) + [near, coll]:
        if m in (bx.MONO, bx.ALLMISS):
            continue
        h = have[m] & pres
        x = np.where(have[m], a[m], a[m][h].mean())[pres].astype(np.float64)
        for c in range(Y.shape[0]):
            res = scipy_stats.pearsonr(x, Y[c][pres])
            worst_r = max(worst_r, abs(float(ref["r"][c, m]) - res.statistic))
            assert abs(float(ref["r"][c, m]) - res.statistic) <= 1e-12, (m, c)
            if (c, m) == (4, coll):
                continue                                           # r = -1: 1 - r^2 is decided by the last bit on both sides
            t = float(ref["t"][c, m])
            # pearsonr's p is the t test with n - 2 degrees of freedom (its beta form); the relative bar follows the cancellation in 1 - r^2
            pw, pg = res.pvalue, float(ref["p"][c, m])
            if pw > 1e-280:
                rel = abs(pg / pw - 1.0)
                worst_p = max(worst_p, rel)
                assert rel <= 1e-9 * max(1.0, t * t / n), (m, c, pg, pw)
    print("restatement against scipy.stats.pearsonr: max |dr| %.3e, max rel dp %.3e" % (worst_r, worst_p))
    dev = sr.deviation(r64, ref, n, skip=[(4, coll)])
    print("restatement float64 against long double: r %.3e, t %.3e" % (dev["r"], dev["t"]))
    assert dev["r"] < 1e-12 and dev["t"] < 1e-6


def test_rules_of_the_restatement(ragged):
    cs, Y, near, coll, ref, r64 = ragged
    for d in (ref, r64):
        for k in ("r", "t", "p"):
            assert np.all(np.isnan(d[k][:, [bx.MONO, bx.ALLMISS]]))
            keep = np.ones(cs["M"], dtype=bool)
            keep[[bx.MONO, bx.ALLMISS]] = False
            assert not np.any(np.isnan(d[k][:, keep]))
        assert float(d["r"][4, coll]) < -1 + 1e-12 and (np.isinf(d["t"][4, coll]) or float(d["t"][4, coll]) < -1e6)
        assert float(d["p"][4, coll]) == 0.0
        assert float(d["r"][3, near]) > 0.99999 and float(d["t"][3, near]) > 1e3
        assert np.all(np.sign(d["t"][:, keep]) == np.sign(d["r"][:, keep]))
    # the rule itself, on made-up values
    assert sr.ar.t_two_sided(np.array([np.inf]), 5)[0] == 0


def test_screen_prepare_of_the_binding():
    from gvamp_amd import capi
    cs = bx.case("ragged")
    Y, _, _ = sr.phenotypes(cs)
    pres, n, N = cs["present"], cs["nonas"], cs["N"]

    class Stub:                                                     # screen_prepare reads N, mbytes and the remembered mask only
        pass
    st = Stub()
    st.N, st.mbytes, st._present = N, (N + 3) // 4, pres
    U = capi.Shard.screen_prepare(st, Y)
    assert U.shape == (5, 4 * st.mbytes) and np.all(U[:, N:] == 0) and np.all(U[:, :N][:, ~pres] == 0)
    for c in range(5):
        u = U[c, :N][pres].astype(np.longdouble)
        y = Y[c][pres].astype(np.longdouble)
        d = y - y.mean()
        want = d * np.sqrt((n - 1) / (d * d).sum())
        assert float(np.max(np.abs(u - want))) <= 1e-12 * float(np.max(np.abs(want)))
        assert abs(float(u.sum())) <= 1e-9 and abs(float((u * u).sum()) - (n - 1)) <= 1e-9 * n
    # values at individuals the mask leaves out are ignored; a NaN at one it keeps is refused
    Y2 = Y.copy()
    Y2[:, ~pres] = 123.0
    assert np.array_equal(capi.Shard.screen_prepare(st, Y2), U)
    Y2[2, np.nonzero(pres)[0][4]] = np.nan
    with pytest.raises(capi.GvError, match="column 2 is NA"):
        capi.Shard.screen_prepare(st, Y2)
