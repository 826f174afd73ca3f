"""Restatement of the covariate-adjusted association screen (gv_screen_cov_set / gv_screen_cov_dev), written from
its definition and kept apart from the library's code: decode the 2-bit genotypes and impute a missing genotype with the marker's mean
(as tests/screen_restatement.py), centre the covariates over the n phenotyped individuals and orthonormalise them by modified
Gram-Schmidt (applied twice), residualise the centred phenotype on that basis, and per (marker, phenotype column)

    rho  = xh_j . u / sqrt(v_j)        xh_j the unit-norm centred imputed column, u the unit-norm residual, v_j = 1 - |Q^T xh_j|^2
    t    = rho sqrt(nu / (1 - rho^2))  nu = n - 2 - K,  p the two-sided tail of Student's t with nu degrees of freedom
    beta = rho sqrt(S / (sxx_j v_j))   S the residual's sum of squares, sxx_j the centred imputed column's
    se   = sqrt(S (1 - rho^2) / (nu sxx_j v_j))

numpy long double by default; dtype=np.float64 gives the same formulas in plain float64, whose deviation from long double is the yardstick
of the GPU test (the rule of section 15).

Rules: 1 - rho^2 <= 0 gives t = +-inf, p = 0 and se = 0; a marker without variance among the phenotyped present genotypes, and a marker
whose variance-inflation factor 1 / v_j is above vif_max, give NaN in all five; a phenotype whose residual is zero gives NaN in all five."""
import numpy as np

import assoc_restatement as ar
import bed_fixed_restatement as bx
import screen_restatement as sr

LD = np.longdouble
NAMES = ("r", "t", "p", "beta", "se")


def imputed_columns(bed, N, M, present, dtype=LD):
    """(xc, sxx, novar, mu): the centred mean-imputed columns over the phenotyped (M x n), their sums of squares, the markers without
    variance among the phenotyped present genotypes, the means"""
    a, have = sr.genotypes(bed, N, M)
    a, have = a[:, present].astype(dtype), have[:, present]
    cnt = have.sum(axis=1).astype(dtype)
    mu = np.where(cnt > 0, (a * have).sum(axis=1) / np.where(cnt > 0, cnt, dtype(1)), dtype(0))
    xc = np.where(have, a - mu[:, None], dtype(0))
    return xc, (xc * xc).sum(axis=1), ~sr._differs(a, have), mu


def basis(Cov, present, dtype=LD):
    """the orthonormal basis (K x n) of the covariates centred over the phenotyped: each column scaled to unit norm, then modified
    Gram-Schmidt applied twice.  A column that loses all but 1e-10 of its norm is collinear: ValueError"""
    n = int(present.sum())
    if Cov is None or len(Cov) == 0:
        return np.zeros((0, n), dtype=dtype)
    A = np.atleast_2d(np.asarray(Cov, dtype=np.float64))[:, present].astype(dtype)
    A = A - (A.sum(axis=1) / dtype(n))[:, None]
    Q = []
    for k, q in enumerate(A):
        nrm = np.sqrt((q * q).sum())
        if not nrm > 0:
            raise ValueError("covariate %d is constant over the phenotyped" % k)
        q = q / nrm
        for _ in range(2):
            for b in Q:
                q = q - (b * q).sum() * b
        left = np.sqrt((q * q).sum())
        if not left > 1e-10:
            raise ValueError("covariate %d is collinear with the ones before it" % k)
        Q.append(q / left)
    return np.stack(Q)


def screen_cov(bed, N, M, present, Y, Cov, vif_max=50.0, dtype=LD):
    """Y: C x N raw phenotype columns, Cov: K x N raw covariate columns or None (entries at individuals outside `present` are ignored).
    Returns dict r, t, p, beta, se (C x M), vif (M; inf where v <= 0), dropped (M: vif > vif_max), novar (M), n, nu"""
    present = np.ones(N, dtype=bool) if present is None else np.asarray(present, dtype=bool)
    n = int(present.sum())
    xc, sxx, novar, _ = imputed_columns(bed, N, M, present, dtype)
    sx1 = np.where(novar, dtype(1), sxx)
    xh = xc / np.sqrt(sx1)[:, None]
    Q = basis(Cov, present, dtype)
    K = Q.shape[0]
    nu = n - 2 - K
    Z = xh @ Q.T                                                   # M x K
    v = dtype(1) - (Z * Z).sum(axis=1)
    with np.errstate(divide="ignore"):
        vif = np.where(v > 0, dtype(1) / np.where(v > 0, v, dtype(1)), dtype(np.inf))
    dropped = vif > dtype(vif_max)
    v1 = np.where(dropped | novar, dtype(1), v)
    Yc = np.atleast_2d(np.asarray(Y, dtype=np.float64))[:, present].astype(dtype)
    Yc = Yc - (Yc.sum(axis=1) / dtype(n))[:, None]
    for _ in range(2):
        for b in Q:
            Yc = Yc - (Yc @ b)[:, None] * b[None, :]
    S = (Yc * Yc).sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        U = Yc / np.sqrt(S)[:, None]
        rho = (U @ xh.T) / np.sqrt(v1)[None, :]                    # C x M
        om = dtype(1) - rho * rho
        flat = om <= 0
        om1 = np.where(flat, dtype(1), om)
        t = np.where(flat, np.copysign(dtype(np.inf), rho), rho * np.sqrt(dtype(nu) / om1))
        d = (sx1 * v1)[None, :]
        beta = rho * np.sqrt(S[:, None] / d)
        se = np.where(flat, dtype(0), np.sqrt(S[:, None] * om1 / (dtype(nu) * d)))
    p = ar.t_two_sided(t.astype(LD), nu).astype(dtype)
    p[np.isinf(t)] = 0
    out = dict(r=rho, t=t, p=p, beta=beta, se=se)
    for k in NAMES:
        out[k][:, novar | dropped] = np.nan
        out[k][~(S > 0), :] = np.nan
    out.update(vif=vif, dropped=dropped, novar=novar, n=n, nu=nu, S=S)
    return out


def deviation(got, ref, nu, skip=()):
    """max deviation from the reference: r and t as tests/screen_restatement.py takes them (with nu in place of n - 2), beta as
    |d| / (|beta| + se) and se as |d| / se; entries where the reference is not finite or its se is zero and the (column, marker) entries
    of `skip` are left out"""
    g = {k: np.asarray(got[k], dtype=LD) for k in ("r", "t", "beta", "se")}
    f = {k: np.asarray(ref[k], dtype=LD) for k in ("r", "t", "beta", "se")}
    ok = np.isfinite(f["t"]) & np.isfinite(f["r"]) & np.isfinite(f["beta"]) & (f["se"] > 0)
    for c, m in skip:
        ok[c, m] = False
    with np.errstate(invalid="ignore", divide="ignore"):
        noise = np.sqrt(np.maximum(LD(1) - f["r"] * f["r"], LD(0)) / LD(nu))
        dev = dict(r=np.abs(g["r"] - f["r"]) / (np.abs(f["r"]) + noise), t=np.abs(g["t"] - f["t"]) / (np.abs(f["t"]) + 1),
                   beta=np.abs(g["beta"] - f["beta"]) / (np.abs(f["beta"]) + f["se"]), se=np.abs(g["se"] - f["se"]) / f["se"])
    return {k: float(np.max(d[ok])) for k, d in dev.items()}


# ---- the inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------------------
TRIP = 200                                   # the marker the fourth covariate is built on
VIF, VIF_LOOSE = 50.0, 1e6


def _imputed(a, have, pres, m):
    return np.where(have[m], a[m], a[m][have[m] & pres].mean())


def covariates(cs, seed=11):
    """(Cov, anc): four raw covariate columns of case cs (tests/bed_fixed_restatement.py) -- an ancestry-like one (a weighted sum of 20
    markers' imputed columns plus noise), an age-like one (mean 55, sd 8), a 0 / 1 one, and a fourth equal to marker TRIP's imputed column
    plus 3 % noise, which puts that marker's variance-inflation factor between VIF and VIF_LOOSE.  The tests use the first three, or all
    four.  NaN at the individuals without a phenotype.  anc: the 20 markers"""
    N, M, pres = cs["N"], cs["M"], np.asarray(cs["present"], dtype=bool)
    rng = np.random.default_rng(seed + M)
    a, have = sr.genotypes(cs["bed"], N, M)
    free = np.setdiff1d(np.arange(M), [17, 40, bx.MONO, bx.ALLMISS, TRIP])
    anc = np.sort(rng.choice(free, 20, replace=False))
    w = rng.standard_normal(20)
    Cov = np.empty((4, N))
    Cov[0] = sum(wi * _imputed(a, have, pres, m) for wi, m in zip(w, anc)) + 2.0 * rng.standard_normal(N)
    Cov[1] = 55.0 + 8.0 * rng.standard_normal(N)
    Cov[2] = (rng.random(N) < 0.45).astype(np.float64)
    g = _imputed(a, have, pres, TRIP)
    Cov[3] = g + 0.03 * g[pres].std() * rng.standard_normal(N)
    Cov[:, ~pres] = np.nan
    return Cov, anc


def random_covariates(cs, K, seed=23):
    """K columns of standard normals (the K = 16, 17 and 32 cases of the GPU test), NaN at the individuals without a phenotype"""
    Cov = np.random.default_rng(seed + K).standard_normal((K, cs["N"]))
    Cov[:, ~np.asarray(cs["present"], dtype=bool)] = np.nan
    return Cov


_FIX = {}


def fixture(name):
    """the case, its four covariates and five phenotypes: computed once, shared by the tests, never changed"""
    if name not in _FIX:
        cs = bx.case(name)
        Cov, anc = covariates(cs)
        Y, near, coll = phenotypes(cs, Cov)
        _FIX[name] = dict(cs=cs, Cov=Cov, anc=anc, Y=Y, near=near, coll=coll)
    return _FIX[name]


def phenotypes(cs, Cov):
    """the five phenotypes of tests/screen_restatement.py plus covariate effects (the first three covariates).  Column 4 stays exactly
    collinear with marker `coll` once the covariates are taken out.  Returns (Y, near, coll)"""
    Y, near, coll = sr.phenotypes(cs)
    pres = np.asarray(cs["present"], dtype=bool)
    eff = np.array([[0.3, 0.02, -0.5], [1e-4, 1e-5, 2e-4], [4.0, -0.9, 10.0], [0.1, 0.01, 0.2], [-0.2, 0.03, 0.4]])
    C3 = np.where(pres[None, :], Cov[:3], 0.0)
    Y = Y + eff @ C3
    Y[:, ~pres] = np.nan
    return Y, near, coll
