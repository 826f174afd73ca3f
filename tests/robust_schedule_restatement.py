"""Dense-numpy restatement of --model robust as the product runs it (vamp::infere_robust): the loop of
tests/robust_restatement.py::robust_run with its two corrections, plus the delta_H schedule and the guard.

  * schedule "deferred" (the default): iteration 1 skips the delta_H step of vamp_Huber.cpp:259; iteration 2 picks delta_H on the
    p1 and tau1 it is about to denoise, before g1_Huber; from iteration 2 on the step at :259 runs as the reference has it
  * schedule "reference": the reference's order, statement for statement robust_run's
  * the guard: a run whose 1 - beta1 is not strictly positive, or whose p2 or tau2 is not finite, stops in that iteration; the
    iteration is not recorded, and `stopped` holds (iteration, the deltaH and the tau1 g1_Huber was given, beta1)

Imported by test_robust_schedule_cpu.py and test_gpu_robust_loop.py; not a test module itself."""
import numpy as np

from gvamp_amd import synth

from robust_restatement import delta_objective, first_min, g1_huber
from test_independent_restatement import Dense, bern_probe, clip, g1_g1d, precond_cg, update_prior


class Run(list):
    """the per-iteration records; `stopped` = (iteration, deltaH, tau1, beta1) when the guard ended the run, else None"""
    stopped = None


def robust_run(D, y, probs, vars_, *, iterations, gam1, rho, CG_max_iter, seed, stop_criteria_thr=1e-5,
               schedule="deferred", shards=1):
    """vamp_Huber.cpp:24-441 with corrections (a), (b), the schedule and the guard; y is the filtered phenotype.  Per iteration,
    `deltaH` is what the :259 step left (robust_run's field), `deltaH_applied` the value g1_Huber denoised with.  shards: the
    Onsager probe of a run over that many marker shards (divide_work, each slice drawn from seed + S, vamp.cpp:875)."""
    if schedule not in ("deferred", "reference"):
        raise ValueError(schedule)
    deferred = schedule == "deferred"
    N, M, Mt = D.N, D.M, D.M
    vars_ = [v * N for v in vars_]                      # vamp.cpp:154-155
    probs = list(probs)
    tau1 = gam1                                         # :36
    r1, r2, x1 = np.zeros(M), np.zeros(M), np.zeros(M)  # :47-49
    p1 = np.zeros(N)                                    # :48
    alpha1, gam2 = 0.0, 0.0                             # :50
    deltaH = 1e-3                                       # :57
    size, extra = divmod(M, shards)
    sizes = [size + 1 if r < extra else size for r in range(shards)]
    u = np.concatenate([bern_probe(seed, sum(sizes[:r]), sizes[r], Mt) for r in range(shards)])
    out = Run()
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
        if deferred and it == 2:                        # the deferred first step: on the cavity iteration 2 denoises
            deltaH = first_min(delta_objective(p1, y, tau1))
        delta_applied, tau1_applied = deltaH, tau1
        z1, der = g1_huber(p1, tau1, deltaH, y)         # :224-227
        beta1 = der.sum() / N                           # :242-249 (corrected derivative)
        zeta1 = tau1 / beta1                            # :254
        if it >= 2:
            tau1 = clip(1.0 / (1.0 / zeta1 + ((z1 - p1) ** 2).sum() / N))    # :256-257
        if not (deferred and it == 1):
            deltaH = first_min(delta_objective(p1, y, tau1))                 # :259-260 (corrected, one evaluation)
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            p2 = (z1 - beta1 * p1) / (1 - beta1)        # :277-278
        tau2 = clip(tau1 * (1 - beta1) / beta1)         # :287
        if not (1 - beta1 > 0) or not np.all(np.isfinite(p2)) or not np.isfinite(tau2):   # the guard
            out.stopped = (it, delta_applied, tau1_applied, beta1)
            break
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
                        deltaH_applied=delta_applied, cg=cg_steps, ons=ons_steps, L=len(probs), p1_in=p1_used, z1=z1))
        rel_err = np.sqrt(((x1_prev - x1) ** 2).sum() / (x1_prev ** 2).sum()) if it > 1 else np.inf   # :415-420
        if it > 1 and rel_err < stop_criteria_thr:      # :431-435
            break
    return out


def case(N, M, seed, bed_seed, noise="gaussian", frac=0.3, sd=0.3):
    """(bed, Dense, beta, y): test_robust_cpu.py::_restated_case, and with noise = "contaminated" 10 % of its noise scaled by 10"""
    rng = np.random.default_rng(seed)
    bed = synth.synth_bed(N, M, seed=bed_seed, miss_ppm=10000)
    D = Dense(bed, N, M)
    beta = rng.standard_normal(M) * (rng.random(M) < frac) * sd
    e = rng.standard_normal(N)
    if noise == "contaminated":
        e = e * np.where(rng.random(N) < 0.1, 10.0, 1.0)
    elif noise != "gaussian":
        raise ValueError(noise)
    return bed, D, beta, D.Ax(beta * np.sqrt(N)) + np.sqrt(0.5) * e
