"""--model robust (vamp_Huber.cpp) on the CPU: the closed-form delta_H objective against quadrature, the reference's Monte-Carlo
rule and why it is replaced, the new C ABI names, and the dense restatement of the corrected model."""
import os
import re
import subprocess

import numpy as np
import pytest
from scipy import integrate

from gvamp_amd import capi, synth

import robust_restatement as rr
from test_independent_restatement import Dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_NAMES = ("gv_huber_denoise", "gv_huber_delta")


def quad_expect(mu, s, d):
    """E[rho_d(mu + s t)], t ~ N(0, 1), by quadrature over the three pieces of the Huber loss, truncated at |t| = 40"""
    a, b = (-d - mu) / s, (d - mu) / s
    phi = lambda t: np.exp(-0.5 * t * t) / np.sqrt(2 * np.pi)             # noqa: E731
    pieces = ((-40.0, a, lambda t: d * (-(mu + s * t) - d / 2) * phi(t)),
              (a, b, lambda t: 0.5 * (mu + s * t) ** 2 * phi(t)),
              (b, 40.0, lambda t: d * ((mu + s * t) - d / 2) * phi(t)))
    tot = 0.0
    for lo, hi, f in pieces:
        lo, hi = max(lo, -40.0), min(hi, 40.0)
        if hi > lo:
            tot += integrate.quad(f, lo, hi, epsabs=0, epsrel=1e-13, limit=200)[0]
    return tot


@pytest.mark.parametrize("d", rr.GRID)
def test_closed_form_expected_loss_matches_quadrature(d):
    worst = 0.0
    for mu in (-50.0, -7.5, -1.0, -1e-3, 0.0, 2e-6, 0.3, 1.0, 2.9, 12.0, 50.0):
        for s in (1e-5, 1e-3, 0.1, 0.7, 1.0, 3.0, 10.0):
            want = quad_expect(mu, s, d)
            got = float(rr.huber_expect(mu, s, d))
            worst = max(worst, abs(got - want) / abs(want))
            assert np.isclose(got, want, rtol=1e-10, atol=0), (mu, s, d, got, want)
    assert worst < 1e-10


def test_log_normaliser_matches_quadrature():
    for d in rr.GRID:
        centre = integrate.quad(lambda w: np.exp(-0.5 * w * w), 0.0, d, epsabs=0, epsrel=1e-13)[0]
        # tail int_d^inf exp(-d w + d^2/2) dw with u = d w
        tail = integrate.quad(lambda u: np.exp(-u), d * d, np.inf, epsabs=0, epsrel=1e-13)[0] * np.exp(0.5 * d * d) / d
        assert np.isclose(rr.log_norm(d), np.log(2 * (centre + tail)), rtol=1e-12, atol=0), d


def _noises(N, seed):
    rng = np.random.default_rng(seed)
    return {"gaussian": rng.standard_normal(N), "t2": rng.standard_t(2, N),
            "contaminated": np.where(rng.random(N) < 0.1, 10.0, 1.0) * rng.standard_normal(N)}


def test_reference_monte_carlo_rule_never_leaves_the_bottom_of_its_grid():
    """vamp_Huber.cpp:522-586 as written: the Huber loss is non-decreasing in d for every residual, so without log Z the
    expected-loss minimiser is grid[0] = 1e-6 whatever the noise -- the reason for correction (b)"""
    N = 20000
    for name, e in _noises(N, 5).items():
        for tau1 in (100.0, 1.0):
            got = rr.reference_mc_delta(np.zeros(N), e, tau1, np.random.default_rng(7))
            assert got == rr.GRID[0], (name, tau1, got)


def test_corrected_rule_picks_a_larger_delta_for_gaussian_than_for_contaminated_noise():
    N = 20000
    noise = _noises(N, 5)
    p1 = np.zeros(N)
    for tau1 in (100.0, 1.0):
        pick = {k: rr.first_min(rr.delta_objective(p1, e, tau1)) for k, e in noise.items()}
        assert pick["gaussian"] > pick["contaminated"], (tau1, pick)
        assert pick["gaussian"] > pick["t2"], (tau1, pick)
        assert min(pick.values()) > rr.GRID[0], (tau1, pick)


def test_first_minimum_with_strict_less_than():
    assert rr.first_min([3.0, 1.0, 1.0, 2.0], [1, 2, 3, 4]) == 2
    assert rr.first_min([np.nan, 5.0], [1, 2]) == 2


def test_new_abi_names_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "gvamp.h")) as f:
        hdr = f.read()
    for name in NEW_NAMES:
        assert re.search(r"\bint\s+%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS
    assert re.search(r"#define\s+GV_ABI_VERSION\s+4\b", hdr)
    lib = os.path.join(ROOT, "gvamp_amd", "libgvamp.so")
    if os.path.exists(lib):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout
        for name in NEW_NAMES:
            assert re.search(r"\bT %s$" % name, syms, re.M), name


def test_huber_denoiser_restatement_and_its_derivative():
    """g1_Huber's three branches (|w| == thr exactly on the inside one) and the corrected derivative by finite differences"""
    tau1, d = 0.8, 0.5
    var = 1 / tau1
    thr = (1 + var) * d
    y = np.array([0.0, 3.0, -3.0, thr, -thr, 0.2])
    p1 = np.zeros_like(y)
    z1, der = rr.g1_huber(p1, tau1, d, y)
    assert np.allclose(z1[:3], [0.0, 3.0 - (3.0 - var * d), -3.0 - (-3.0 + var * d)])
    assert z1[3] == y[3] - thr / (1 + var) and z1[4] == y[4] + thr / (1 + var)
    assert np.allclose(der, [1 / (1 + var), 1, 1, 1 / (1 + var), 1 / (1 + var), 1 / (1 + var)])
    h = 1e-7
    for i in (0, 1, 2, 5):
        zp, _ = rr.g1_huber(p1[i:i + 1] + h, tau1, d, y[i:i + 1])
        zm, _ = rr.g1_huber(p1[i:i + 1] - h, tau1, d, y[i:i + 1])
        assert np.isclose((zp - zm)[0] / (2 * h), der[i], rtol=1e-6), i


def _restated_case(N, M, seed, bed_seed):
    rng = np.random.default_rng(seed)
    D = Dense(synth.synth_bed(N, M, seed=bed_seed, miss_ppm=10000), N, M)
    beta = rng.standard_normal(M) * (rng.random(M) < 0.3) * 0.3
    y = D.Ax(beta * np.sqrt(N)) + np.sqrt(0.5) * rng.standard_normal(N)
    return D, beta, y


def test_small_n_breakdown_when_no_residual_falls_inside_the_threshold():
    """A finite-N failure of the loop as stated, not a property of the corrected model: iteration 1 picks
    delta_H under the starting cavity tau1 = gam1 = 1e-8 (s = 1e4), where the objective ~ d s E|t| - log d has its minimiser near 1/s.
    Iteration 2 applies that delta with a fitted tau1, so thr = (1 + 1/tau1) delta ~ 1e-4; beta1 == 1 exactly when none of the N
    residuals |y - p1| falls inside, with probability ~ exp(-2 N thr f(0)), f the density of y - p1 at 0.  At N = 300 none does:
    tau2 = tau1 (1 - beta1) / beta1 clips to gamma_min and p2 = (z1 - beta1 p1) / (1 - beta1) is infinite."""
    D, _beta, y = _restated_case(300, 60, 8, 9)
    with np.errstate(all="ignore"):
        out = rr.robust_run(D, y, [0.7, 0.3], [0.0, 0.09], iterations=3, gam1=1e-8, rho=0.5, CG_max_iter=30, seed=4)
    first, second = out[0], out[1]
    assert first["deltaH"] <= 1e-3                                    # chosen with tau1 = 1e-8: s = 1e4
    assert np.isfinite(first["tau1_next"]) and first["tau1_next"] > 1e-3
    assert second["beta1"] == 1.0                                      # every |y - p1| > (1 + 1/tau1) deltaH
    assert not np.isfinite(second["tau2"])


def test_restatement_converges_once_n_is_large():
    """The companion of the test above: the same loop, gam1 = 1e-8 start included, at N = 20 000.  Some residuals fall inside
    iteration 2's threshold, beta1 stays below 1, the delta step leaves the bottom of the grid (0.4 to 3 on this Gaussian noise) and
    x1 recovers the simulated effects."""
    D, beta, y = _restated_case(20000, 500, 8, 9)
    out = rr.robust_run(D, y, [0.7, 0.3], [0.0, 0.09], iterations=6, gam1=1e-8, rho=0.5, CG_max_iter=30, seed=4,
                        stop_criteria_thr=1e-12)
    assert len(out) == 6
    assert out[0]["deltaH"] <= 1e-3
    for t in out:
        assert t["beta1"] < 1.0 and np.isfinite(t["tau2"]) and np.isfinite(t["tau1_next"]), t["beta1"]
    assert all(t["deltaH"] >= 0.1 for t in out[1:]), [t["deltaH"] for t in out]
    assert np.corrcoef(out[-1]["x1"], beta)[0, 1] > 0.99
