"""tests/screen_cov_restatement.py held to what it restates, without a GPU.

Brute force: per marker, numpy.linalg.lstsq of y on [1, Cov, g_j] over the phenotyped individuals (g_j the mean-imputed genotype column),
beta its last coefficient, se = sqrt(s^2 (X^T X)^-1_gg) with s^2 = RSS / (n - K - 2), t = beta / se.  60 individuals x 40 markers, K = 3,
5 % missing genotypes.  Both routes are float64 and the variance-inflation factors stay below 50, so they agree to about 1e-13 (5.5e-14
was seen); the bar is 1e-9, taken as the GPU test takes its deviations: |d beta| / (|beta| + se), |d se| / se, |d t| / (|t| + 1).

K = 0 is the marginal screen of tests/screen_restatement.py.  In long double the two ways of writing r differ by roundings of 2^-64 over
sums of n ~ 1000 terms: r is held to 1e-15 in that file's deviation measure; t = r sqrt(nu / (1 - r^2)) carries the relative error of r
magnified by 1 / (1 - r^2) (one phenotype is a marker plus 1e-3 noise: 1 - r^2 ~ 1e-6), so |dt| / (|t| + 1) is held to 1e-15 / (1 - r^2)
entry by entry; and p, whose logarithm moves by about t^2 times the relative error of t (t^2 < 3000 wherever p is above 1e-300 at these
degrees of freedom), to 1e-9 relative.

The fixtures of the GPU test (tests/test_gpu_screen_cov.py): a covariate equal to a marker's imputed column plus 3 % noise puts exactly
that marker above a variance-inflation factor of 50 and none above 1e6, and no marker's factor lies within a relative 1e-9 of either
threshold, so the set of NaN markers is decidable in float64."""
import numpy as np
import pytest

import bed_fixed_restatement as bx
import screen_cov_restatement as sc
import screen_restatement as sr
from gvamp_amd import synth


def test_the_restatement_equals_a_least_squares_fit_per_marker():
    N, M, K = 60, 40, 3
    rng = np.random.default_rng(5)
    bed = synth.synth_bed(N, M, seed=9, miss_ppm=50000)
    present = np.ones(N, dtype=bool)
    present[[7, 31, 58]] = False
    Cov = np.stack([rng.standard_normal(N), 55.0 + 8.0 * rng.standard_normal(N), (rng.random(N) < 0.5).astype(float)])
    Y = rng.standard_normal((2, N)) + np.array([[0.4, 0.05, 1.0], [-1.0, 0.0, 0.3]]) @ Cov
    got = sc.screen_cov(bed, N, M, present, Y, Cov, dtype=np.float64)
    assert got["nu"] == 57 - 2 - K and not got["dropped"].any() and float(np.max(got["vif"][~got["novar"]])) < 50.0
    a, have = sr.genotypes(bed, N, M)
    n = int(present.sum())
    worst = dict(beta=0.0, se=0.0, t=0.0)
    tested = 0
    for m in range(M):
        if got["novar"][m]:
            continue
        h = have[m] & present
        g = np.where(have[m], a[m], a[m][h].mean())[present].astype(np.float64)
        X = np.column_stack([np.ones(n), Cov[:, present].T, g])
        for c in range(2):
            y = Y[c, present]
            coef, _, rank, _ = np.linalg.lstsq(X, y, rcond=None)
            assert rank == K + 2
            res = y - X @ coef
            s2 = float(res @ res) / (n - K - 2)
            se = np.sqrt(s2 * np.linalg.inv(X.T @ X)[-1, -1])
            beta = coef[-1]
            worst["beta"] = max(worst["beta"], abs(got["beta"][c, m] - beta) / (abs(beta) + se))
            worst["se"] = max(worst["se"], abs(got["se"][c, m] - se) / se)
            worst["t"] = max(worst["t"], abs(got["t"][c, m] - beta / se) / (abs(beta / se) + 1.0))
            tested += 1
    print("restatement against lstsq over %d fits: %s" % (tested, worst))
    assert tested >= 60
    for k, w in worst.items():
        assert w <= 1e-9, (k, w)


def test_without_covariates_it_is_the_marginal_screen():
    fx = sc.fixture("ragged")
    cs = fx["cs"]
    Y, near, coll = sr.phenotypes(cs)
    ref = sr.screen(cs["bed"], cs["N"], cs["M"], cs["present"], Y)
    got = sc.screen_cov(cs["bed"], cs["N"], cs["M"], cs["present"], Y, None)
    assert got["nu"] == cs["nonas"] - 2 and np.all(got["vif"] == 1) and not got["dropped"].any()
    for k in ("r", "t", "p"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), k
    dev = sr.deviation(got, ref, cs["nonas"], skip=[(4, coll)])
    print("K = 0 against the marginal screen: %s" % dev)
    assert dev["r"] <= 1e-15, dev
    fin = np.isfinite(ref["t"])
    fin[4, coll] = False
    om = 1 - ref["r"][fin] ** 2
    dt = np.abs(got["t"][fin] - ref["t"][fin]) / (np.abs(ref["t"][fin]) + 1)
    assert np.all(om > 0) and np.all(dt * om <= 1e-15), float(np.max(dt * om))
    ok = np.isfinite(ref["p"]) & (ref["p"] > 1e-300)
    ok[4, coll] = False
    rel = float(np.max(np.abs(got["p"][ok] / ref["p"][ok] - 1)))
    assert rel <= 1e-9, rel


@pytest.mark.parametrize("name", list(bx.SHAPES))
def test_the_fourth_covariate_trips_exactly_its_marker_and_the_nan_set_is_decidable(name):
    fx = sc.fixture(name)
    cs = fx["cs"]
    args = (cs["bed"], cs["N"], cs["M"], cs["present"], fx["Y"][:1])
    sets = [("three", fx["Cov"][:3]), ("four", fx["Cov"]), ("none", None)]
    if name == "ragged":
        sets += [("random %d" % K, sc.random_covariates(cs, K)) for K in (16, 17, 32)]
    for label, Cov in sets:
        got = sc.screen_cov(*args, Cov, vif_max=sc.VIF, dtype=np.float64)
        vif = got["vif"][~got["novar"]]
        want = [sc.TRIP] if label == "four" else []
        assert np.array_equal(np.nonzero(got["dropped"] & ~got["novar"])[0], want), (label, np.nonzero(got["dropped"])[0])
        assert not np.any(vif > sc.VIF_LOOSE), label
        for thr in (sc.VIF, sc.VIF_LOOSE):
            assert not np.any(np.abs(vif / thr - 1.0) <= 1e-9), (label, thr)
        if label == "four":
            assert sc.VIF < got["vif"][sc.TRIP] < sc.VIF_LOOSE
        print("%s %s: largest variance-inflation factor %.4g" % (name, label, float(np.max(vif))))
