"""tests/dosage_screen_restatement.py held to what it restates, without a GPU.

Brute force: per marker, numpy.linalg.lstsq of y on [1, Cov, x_j] over the phenotyped individuals (x_j the mean-imputed value column
scale * code), beta its last coefficient, se = sqrt(s^2 (X^T X)^-1_xx) with s^2 = RSS / (n - K - 2), t = beta / se.  60 individuals x 40
markers, K = 3, 5 % reserved codes.  Both routes are float64 and the variance-inflation factors stay below 50; the bar is the 1e-9 of
tests/test_screen_cov_cpu.py, in its measures: |d beta| / (|beta| + se), |d se| / se, |d t| / (|t| + 1).

The bed restatements: a bed matrix written as codes 64 * {0, 1, 2} with scale 1 / 64 and the reserved code at the missing genotypes is
the same data.  Every step of the two restatements then differs by an exact power of two (64 mu, 64^2 sxx), so they agree to the last
bits of long double; they are held to 1e-15 in the deviation measures of the bed files, t entry by entry to 1e-15 / (1 - r^2), p to
1e-9 relative (the bars of test_screen_cov_cpu.py for two long-double ways of writing the same thing).

The fixtures of the GPU test (tests/test_gpu_dosage_screen.py): the fourth covariate puts exactly marker TRIP above a variance-inflation
factor of 50 and none above 1e6, and no marker's factor lies within a relative 1e-9 of either threshold, so the set of NaN markers is
decidable in float64."""
import numpy as np
import pytest

import bed_fixed_restatement as bx
import dosage_screen_restatement as ds
import screen_cov_restatement as sc
import screen_restatement as sr


def test_the_restatement_equals_a_least_squares_fit_per_marker():
    N, M, K, scale = 60, 40, 3, 1.0 / 127.0
    rng = np.random.default_rng(5)
    g = rng.binomial(2, rng.uniform(0.1, 0.5, M)[:, None], (M, N)) + 0.2 * rng.standard_normal((M, N))
    B = np.clip(np.rint(np.clip(g, 0, 2) * 127), 0, 254).astype(np.uint8)
    B[rng.random((M, N)) < 0.05] = 255
    B[7] = 31                                                       # a constant marker
    present = np.ones(N, dtype=bool)
    present[[7, 31, 58]] = False
    Cov = np.stack([rng.standard_normal(N), 55.0 + 8.0 * rng.standard_normal(N), (rng.random(N) < 0.5).astype(float)])
    Y = rng.standard_normal((2, N)) + np.array([[0.4, 0.05, 1.0], [-1.0, 0.0, 0.3]]) @ Cov
    got = ds.screen_cov(B, 8, scale, True, present, Y, Cov, dtype=np.float64)
    assert got["nu"] == 57 - 2 - K and not got["dropped"].any() and float(np.max(got["vif"][~got["novar"]])) < 50.0
    assert np.array_equal(np.nonzero(got["novar"])[0], [7])
    n = int(present.sum())
    worst = dict(beta=0.0, se=0.0, t=0.0)
    tested = 0
    for m in range(M):
        if got["novar"][m]:
            assert all(np.all(np.isnan(got[k][:, m])) for k in ds.NAMES)
            continue
        have = B[m] != 255
        x = scale * np.where(have, B[m].astype(np.float64), B[m][have & present].astype(np.float64).mean())[present]
        X = np.column_stack([np.ones(n), Cov[:, present].T, x])
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


def _bed_as_codes(cs):
    a, have = sr.genotypes(cs["bed"], cs["N"], cs["M"])
    return np.where(have, 64 * a, 255).astype(np.uint8)


def test_a_bed_matrix_written_as_codes_gives_the_bed_restatements():
    fx = sc.fixture("ragged")
    cs, coll = fx["cs"], fx["coll"]
    B = _bed_as_codes(cs)
    n = cs["nonas"]
    # the marginal screen
    Y, _, _ = sr.phenotypes(cs)
    ref = sr.screen(cs["bed"], cs["N"], cs["M"], cs["present"], Y)
    got = ds.screen(B, 8, 1.0 / 64.0, True, cs["present"], Y)
    assert np.array_equal(got["novar"], ref["novar"]) and sorted(np.nonzero(ref["novar"])[0]) == sorted([bx.MONO, bx.ALLMISS])
    _hold_pair("marginal", got, ref, n - 2, coll, sr.deviation(got, ref, n, skip=[(4, coll)]))
    # the adjusted one, K = 3
    ref = sc.screen_cov(cs["bed"], cs["N"], cs["M"], cs["present"], fx["Y"], fx["Cov"][:3])
    got = ds.screen_cov(B, 8, 1.0 / 64.0, True, cs["present"], fx["Y"], fx["Cov"][:3])
    assert got["nu"] == ref["nu"] == n - 5 and np.array_equal(got["novar"], ref["novar"]) and np.array_equal(got["dropped"], ref["dropped"])
    _hold_pair("adjusted", got, ref, n - 5, coll, sc.deviation(got, ref, n - 5, skip=[(4, coll)]))


def _hold_pair(label, got, ref, nu, coll, dev):
    names = [k for k in ds.NAMES if k in ref]
    for k in names:
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), (label, k)
    print("%s against the bed restatement: %s" % (label, dev))
    for k in ("r", "beta", "se"):
        assert dev.get(k, 0.0) <= 1e-15, (label, k, dev)
    fin = np.isfinite(ref["t"])
    fin[4, coll] = False
    om = 1 - ref["r"][fin] ** 2
    dt = np.abs(got["t"][fin] - ref["t"][fin]) / (np.abs(ref["t"][fin]) + 1)
    assert np.all(om > 0) and np.all(dt * om <= 1e-15), (label, float(np.max(dt * om)))
    ok = np.isfinite(ref["p"]) & (ref["p"] > 1e-300)
    ok[4, coll] = False
    rel = float(np.max(np.abs(got["p"][ok] / ref["p"][ok] - 1)))
    assert rel <= 1e-9, (label, rel)


@pytest.mark.parametrize("bits,missing", [(8, False), (8, True), (16, False), (16, True)])
def test_the_fixtures_of_the_gpu_test_have_a_decidable_nan_set(bits, missing):
    fx = ds.fixture(bits, missing)
    args = (fx["B"], bits, fx["scale"], missing, fx["present"], fx["Y"][:1])
    sets = [("three", fx["Cov"][:3]), ("four", fx["Cov"]), ("none", None), ("random 17", ds.random_covariates(fx, 17))]
    for label, Cov in sets:
        got = ds.screen_cov(*args, Cov, vif_max=ds.VIF, dtype=np.float64)
        assert np.array_equal(np.nonzero(got["novar"])[0], fx["novar"]), (label, np.nonzero(got["novar"])[0])
        assert np.all(got["q"][got["novar"]] == 0) and np.all(got["q"][~got["novar"]] > 0)
        vif = got["vif"][~got["novar"]]
        want = [ds.TRIP] if label == "four" else []
        assert np.array_equal(np.nonzero(got["dropped"] & ~got["novar"])[0], want), (label, np.nonzero(got["dropped"])[0])
        assert not np.any(vif > ds.VIF_LOOSE), label
        for thr in (ds.VIF, ds.VIF_LOOSE):
            assert not np.any(np.abs(vif / thr - 1.0) <= 1e-9), (label, thr)
        if label == "four":
            assert ds.VIF < got["vif"][ds.TRIP] < ds.VIF_LOOSE
        print("%d bits%s %s: largest variance-inflation factor %.4g" % (bits, " missing" if missing else "", label, float(np.max(vif))))
