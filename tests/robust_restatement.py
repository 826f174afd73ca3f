"""Dense-numpy restatement of --model robust (vamp::infere_robust, vamp_Huber.cpp:24-441) with the two corrections of DESIGN.md
section 12, written from the reference source (file:line cited at every statement) in the style of test_independent_restatement.py,
whose design matrix, signal-side denoiser, prior EM, CG solver and Onsager probe it reuses.  Imported by test_robust_cpu.py and
test_gpu_robust.py; not a test module itself.

  * g1_Huber               vamp_Huber.cpp:443-461, in its operation order
  * the derivative         d z1 / d p1 of g1_Huber -- NOT g1d_Huber_der (:485-503), correction (a)
  * the delta_H step       mean_i E[rho_d(W_i)] + log Z(d) in closed form -- NOT the Monte-Carlo expected loss of :522-573,
                           correction (b); the reference's own rule is restated as well (reference_mc_delta) to show why
"""
import numpy as np
from scipy import special

from test_independent_restatement import bern_probe, clip, g1_g1d, precond_cg, update_prior

GRID = [1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 0.2, 0.4, 0.6, 0.8, 1, 1.5, 2, 3]      # vamp_Huber.cpp:259
R2 = np.sqrt(0.5)


def huber_loss(w, d):
    """vamp_Huber.cpp:505-519 (as a function of the residual w = y - z)"""
    aw = np.abs(w)
    return np.where(aw <= d, w * w / 2, d * (aw - d / 2))


# 20-point Gauss-Legendre on [-1, 1]: the positive nodes and their weights (the kernel holds the same digits)
GL_X = np.array([0.076526521133497338, 0.2277858511416451, 0.37370608871541955, 0.51086700195082713, 0.63605368072651502,
                 0.7463319064601508, 0.83911697182221878, 0.91223442825132584, 0.96397192727791381, 0.99312859918509488])
GL_W = np.array([0.15275338713072578, 0.14917298647260366, 0.14209610931838187, 0.13168863844917653, 0.11819453196151825,
                 0.10193011981724026, 0.083276741576704671, 0.062672048334109443, 0.040601429800386217, 0.017614007139153273])
NARROW = 0.5          # d / s at or below which the quadratic piece is integrated by Gauss-Legendre


def huber_expect(mu, s, d):
    """E[rho_d(W)], W ~ N(mu, s^2), in closed form; Phi(b) - Phi(a) on the tail side (erfc) or across 0 (erf).  The quadratic
    piece over |w| <= d is O(d^3) while its three closed-form terms are O(d) each: for d / s <= 1/2 it is integrated instead by
    20-point Gauss-Legendre in w, exact to rounding there (the integrand is a polynomial times a Gaussian over at most one s)."""
    mu, s = np.broadcast_arrays(np.asarray(mu, dtype=np.float64), np.asarray(s, dtype=np.float64))
    a, b = (-d - mu) / s, (d - mu) / s
    dphi = np.where(a >= 0, 0.5 * (special.erfc(a * R2) - special.erfc(b * R2)),
                    np.where(b <= 0, 0.5 * (special.erfc(-b * R2) - special.erfc(-a * R2)),
                             0.5 * (special.erf(b * R2) + special.erf(-a * R2))))
    phi_mb, phi_a = 0.5 * special.erfc(b * R2), 0.5 * special.erfc(-a * R2)
    pa, pb = np.exp(-0.5 * a * a) / np.sqrt(2 * np.pi), np.exp(-0.5 * b * b) / np.sqrt(2 * np.pi)
    centre = 0.5 * ((mu * mu + s * s) * dphi + 2 * mu * s * (pa - pb) + s * s * (a * pa - b * pb))
    gl = np.zeros_like(mu)
    for x, wt in zip(GL_X, GL_W):
        w = d * x
        tp, tm = (w - mu) / s, (-w - mu) / s
        gl = gl + wt * (w * w) * (np.exp(-0.5 * tp * tp) + np.exp(-0.5 * tm * tm)) / np.sqrt(2 * np.pi)
    gl = gl * (0.5 * d / s)
    centre = np.where(d <= NARROW * s, gl, centre)
    return centre + d * ((mu - d / 2) * phi_mb + s * pb) + d * ((-mu - d / 2) * phi_a + s * pa)


def log_norm(d):
    """log Z(d), Z(d) = int exp(-rho_d(w)) dw = sqrt(2 pi)(2 Phi(d) - 1) + (2/d) exp(-d^2/2)"""
    return np.log(np.sqrt(2 * np.pi) * special.erf(d * R2) + 2.0 / d * np.exp(-0.5 * d * d))


def g1_huber(p1, tau1, d, y):
    """vamp_Huber.cpp:443-461 -> (z1, d z1 / d p1).  The derivative is 1/(1+var) inside the threshold and 1 outside (Bradic & Chen,
    Ex. 2, which the reference cites); g1d_Huber_der (:485-503) tests |p1| instead of |w| and returns -1 below -thr."""
    var = 1.0 / tau1
    thr = (1 + var) * d
    w = y - p1
    inside = np.abs(w) <= thr
    est = np.where(inside, w / (1 + var), np.where(w > thr, w - var * d, w + var * d))
    return y - est, np.where(inside, 1.0 / (1 + var), 1.0)


def delta_objective(p1, y, tau1, grid=GRID):
    """corrected M_deltaH_update objective per grid value: mean_i E[rho_d(y_i - z)], z ~ N(p1_i, 1/tau1), + log Z(d)"""
    s = np.sqrt(1.0 / tau1)
    return np.array([huber_expect(y - p1, s, d).mean() + log_norm(d) for d in grid])


def first_min(obj, grid=GRID):
    """M_deltaH_update's selection (vamp_Huber.cpp:558-571): the first minimum, strict <"""
    k, best = 0, np.finfo(np.float64).max
    for i, v in enumerate(obj):
        if v < best:
            k, best = i, v
    return grid[k]


def reference_mc_delta(p1, y, tau1, rng, deltaH=1e-3, grid=GRID, num_MC_steps=100, num_EM_steps=100):
    """the reference's rule as written: EM_deltaH (:576-586) over M_deltaH_update (:554-573) over the Monte-Carlo
    E_MC_eval (:543-551) / E_MC_eval_ind (:522-540), z ~ N(p1, 1/tau1), Huber_loss(z, d, y) -- no log Z"""
    s = np.sqrt(1.0 / tau1)
    for _ in range(num_EM_steps):
        prev = deltaH
        draws = p1[:, None] + s * rng.standard_normal((p1.size, num_MC_steps))      # fresh draws on every evaluation
        obj = [huber_loss(y[:, None] - draws, d).mean(1).mean() for d in grid]
        deltaH = first_min(obj, grid)
        if abs(prev - deltaH) / deltaH < 1e-3:
            break
    return deltaH


def robust_run(D, y, probs, vars_, *, iterations, gam1, rho, CG_max_iter, seed, stop_criteria_thr=1e-5):
    """vamp::infere_robust, vamp_Huber.cpp:24-441, corrected; y is the filtered phenotype (NA -> 0, :217)"""
    N, M, Mt = D.N, D.M, D.M
    vars_ = [v * N for v in vars_]                      # vamp.cpp:154-155
    probs = list(probs)
    tau1 = gam1                                         # :36
    r1, r2, x1 = np.zeros(M), np.zeros(M), np.zeros(M)  # :47-49
    p1 = np.zeros(N)                                    # :48
    alpha1, gam2 = 0.0, 0.0                             # :50
    deltaH = 1e-3                                       # :57
    u = bern_probe(seed, 0, M, Mt)
    out = []
    for it in range(1, iterations + 1):
        x1_prev, alpha1_prev = x1.copy(), alpha1        # :88-89
        for it_revar in range(1, 51):                   # :92-131
            x1, dd = g1_g1d(r1, gam1, probs, vars_)
            alpha1 = dd.sum() / Mt                      # :112-114
            eta1 = gam1 / alpha1
            if it <= 1:
                break
            g_prev = gam1
            gam1 = clip(1.0 / (1.0 / eta1 + ((x1 - r1) ** 2).sum() / Mt))      # :121
            probs, vars_ = update_prior(r1, gam1, probs, vars_, Mt)           # :126
            if abs(gam1 - g_prev) < 1e-3:
                break
        if it > 1:                                      # :133-138
            x1 = rho * x1 + (1 - rho) * x1_prev
            alpha1 = rho * alpha1 + (1 - rho) * alpha1_prev
        r1_start = r1.copy()                            # stored at :154-158
        gam2 = clip(eta1 - gam1)                        # :183
        r2 = (eta1 * x1 - gam1 * r1) / gam2             # :191-192
        z1, der = g1_huber(p1, tau1, deltaH, y)         # :224-227
        beta1 = der.sum() / N                           # :242-249 (corrected derivative)
        zeta1 = tau1 / beta1                            # :254
        if it >= 2:
            tau1 = clip(1.0 / (1.0 / zeta1 + ((z1 - p1) ** 2).sum() / N))    # :256-257
        deltaH = first_min(delta_objective(p1, y, tau1))                     # :259-260 (corrected, one evaluation)
        p2 = (z1 - beta1 * p1) / (1 - beta1)            # :277-278
        tau2 = clip(tau1 * (1 - beta1) / beta1)         # :287
        v = tau2 * D.ATx(p2) + gam2 * r2                # :306-309
        x2, cg_steps = precond_cg(D, v, np.zeros(M), tau2, gam2, 1, CG_max_iter)   # :312, from zero
        invq, ons_steps = precond_cg(D, u, np.zeros(M), tau2, gam2, 0, CG_max_iter)
        alpha2 = gam2 * (u @ invq)                      # :321 (g2d_onsager, vamp.cpp:871-889)
        eta2 = gam2 / alpha2                            # :325
        gam2_used = gam2
        if it > 1:                                      # :332-333
            gam2 = clip(1.0 / (1.0 / eta2 + ((x2 - r2) ** 2).sum() / Mt))
        r1 = (x2 - alpha2 * r2) / (1 - alpha2)          # :338-339
        gam1 = gam2 * (1 - alpha2) / alpha2             # :355
        z2 = D.Ax(x2)                                   # :369
        beta2 = Mt / N * (1 - alpha2)                   # :372
        zeta2 = tau2 / beta2                            # :382
        tau2_used = tau2
        if it > 1:
            tau2 = 1.0 / (1.0 / zeta2 + ((z2 - p2) ** 2).sum() / N)           # :384-385, not clipped
        p1_used = p1
        p1 = (z2 - beta2 * p2) / (1 - beta2)            # :391-392
        tau1 = clip(tau2 * (1 - beta2) / beta2)         # :408
        out.append(dict(x1=x1.copy(), x2=x2.copy(), r1=r1_start, alpha1=alpha1, eta1=eta1, gam2=gam2_used, alpha2=alpha2,
                        beta1=beta1, tau2=tau2, tau2_solve=tau2_used, tau1_next=tau1, gam1_next=gam1, deltaH=deltaH,
                        cg=cg_steps, ons=ons_steps, L=len(probs), p1_in=p1_used, z1=z1))
        rel_err = np.sqrt(((x1_prev - x1) ** 2).sum() / (x1_prev ** 2).sum()) if it > 1 else np.inf   # :415-420
        if it > 1 and rel_err < stop_criteria_thr:      # :431-435
            break
    return out
