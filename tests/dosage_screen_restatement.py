"""Restatement of the association screens on dosage data (gv_set_screen_dosage; gv_screen_dev, gv_screen_cov_set / gv_screen_cov_dev on
8- / 16-bit codes), written from the definition and kept apart from the library's code: decode the codes
(value = scale * code; with `missing` the all-ones code is a missing entry), impute a missing entry with the marker's mean over the
phenotyped individuals with a present entry, and per (marker, phenotype column)

    marginal:   r the Pearson correlation of the imputed column with the phenotype over the n phenotyped individuals,
                t = r sqrt((n - 2) / (1 - r^2)), p the two-sided tail of Student's t with n - 2 degrees of freedom
    adjusted:   the partial regression of tests/screen_cov_restatement.py (centre the K covariates, modified Gram-Schmidt applied twice,
                residualise the phenotype): rho, t and p with nu = n - 2 - K, beta = rho sqrt(S / (sxx_j v_j)) per unit of the value
                scale * code, se = sqrt(S (1 - rho^2) / (nu sxx_j v_j))

numpy long double by default; dtype=np.float64 gives the same formulas in plain float64, whose deviation from long double is the yardstick
of the GPU test (the rule of section 15).

Rules: 1 - r^2 <= 0 gives t = +-inf, p = 0 (and se = 0); a marker whose present entries among the phenotyped take one value, or that has
none (constant, all missing: q == 0, decided on the integer codes), gives NaN in every output; so does a marker whose variance-inflation
factor 1 / v_j is above vif_max, and a phenotype whose residual is zero."""
import numpy as np

import assoc_restatement as ar
import screen_cov_restatement as sc

LD = np.longdouble
NAMES = sc.NAMES


def reserved(bits):
    return (1 << bits) - 1


def decode(B, bits, missing):
    """(code, have): M x N integer codes and whether the entry is present"""
    code = np.asarray(B).astype(np.int64)
    have = code != reserved(bits) if missing else np.ones(code.shape, dtype=bool)
    return code, have


def imputed_columns(B, bits, scale, missing, present, dtype=LD):
    """(xc, sxx, novar, q): the centred mean-imputed value columns over the phenotyped (M x n), their sums of squares, the markers without
    variance among the phenotyped present entries, and q = sxx / scale^2 in code units"""
    code, have = decode(B, bits, missing)
    code, have = code[:, present], have[:, present]
    cnt = have.sum(axis=1)
    tot = (code * have).sum(axis=1)                                 # exact integers
    mu = np.where(cnt > 0, tot.astype(dtype) / np.where(cnt > 0, cnt, 1).astype(dtype), dtype(0))
    dc = np.where(have, code.astype(dtype) - mu[:, None], dtype(0))
    q = (dc * dc).sum(axis=1)
    big = np.where(have, code, -1).max(axis=1)
    small = np.where(have, code, 1 << 62).min(axis=1)
    novar = ~(big > small)                                          # one value, or no present entry at all
    xc = dtype(scale) * dc
    return xc, (xc * xc).sum(axis=1), novar, q


def screen_cov(B, bits, scale, missing, present, Y, Cov, vif_max=50.0, dtype=LD):
    """B: M x N codes; Y: C x N raw phenotype columns, Cov: K x N raw covariate columns or None (entries at individuals outside `present`
    are ignored).  Returns dict r, t, p, beta, se (C x M), vif, dropped, novar (M), q (M), n, nu"""
    B = np.asarray(B)
    N = B.shape[1]
    present = np.ones(N, dtype=bool) if present is None else np.asarray(present, dtype=bool)
    n = int(present.sum())
    xc, sxx, novar, q = imputed_columns(B, bits, scale, missing, present, dtype)
    sx1 = np.where(novar, dtype(1), sxx)
    xh = xc / np.sqrt(sx1)[:, None]
    Q = sc.basis(Cov, present, dtype)
    K = Q.shape[0]
    nu = n - 2 - K
    Z = xh @ Q.T
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
        rho = (U @ xh.T) / np.sqrt(v1)[None, :]
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
    out.update(vif=vif, dropped=dropped, novar=novar, q=q, sxx=sxx, n=n, nu=nu, S=S)
    return out


def screen(B, bits, scale, missing, present, Y, dtype=LD):
    """the marginal screen: the adjusted one without covariates (v_j = 1, nu = n - 2); dict r, t, p (C x M), novar, n"""
    full = screen_cov(B, bits, scale, missing, present, Y, None, dtype=dtype)
    return dict(r=full["r"], t=full["t"], p=full["p"], novar=full["novar"], q=full["q"], n=full["n"])


def from_r(r, nu):
    """t and p restated from a given r (the device's own): t = r sqrt(nu / (1 - r^2)) in long double, the rules at 1 - r^2 <= 0"""
    r = np.asarray(r, dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        om = LD(1) - r * r
        flat = om <= 0
        t = np.where(flat, np.copysign(LD(np.inf), r), r * np.sqrt(LD(nu) / np.where(flat, LD(1), om)))
    t = np.where(np.isnan(r), LD(np.nan), t)
    return t


def beta_se_from_r(r, nu, S, sxx, v):
    """beta and se restated from a given rho (the device's own) in long double: S per column (C), sxx and v per marker (M)"""
    r = np.asarray(r, dtype=LD)
    S = np.asarray(S, dtype=LD)[:, None]
    d = (np.asarray(sxx, dtype=LD) * np.asarray(v, dtype=LD))[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        om = LD(1) - r * r
        flat = om <= 0
        beta = r * np.sqrt(S / d)
        se = np.where(flat, LD(0), np.sqrt(S * np.where(flat, LD(1), om) / (LD(nu) * d)))
    return beta, np.where(np.isnan(r), LD(np.nan), se)


# ---- the inputs shared by the CPU and the GPU tests ---------------------------------------------------------------------------------
N_FIX, M_FIX = 515, 300                      # row pitch 576 = 9 x 64, five K-steps of 128 individuals; three 128-row blocks, the last partial
ALLMISS, ONE, CONST, TRIP, NEAR, COLL = 11, 29, 47, 200, 17, 40
VIF, VIF_LOOSE = 50.0, 1e6
_FIX = {}


def present_mask(N):
    """every 7th individual from 3 on has no phenotype: (mask4 nibbles, present[N], nonas)"""
    pres = np.ones(N, dtype=bool)
    pres[3::7] = False
    idx = np.nonzero(pres)[0]
    m4 = np.zeros((N + 3) // 4, dtype=np.uint8)
    np.bitwise_or.at(m4, idx >> 2, (1 << (idx & 3)).astype(np.uint8))
    return m4, pres, int(pres.sum())


def fixture(bits, missing):
    """codes of N_FIX x M_FIX, the mask, five phenotypes and four covariates: computed once, shared by the tests, never changed.
    With `missing`: 5 % reserved codes and three hand-placed rows -- ALLMISS all missing, ONE with one present entry among the
    phenotyped, CONST constant where present.  Without: CONST alone.  The covariates: an ancestry-like one (a weighted sum of 20 markers'
    imputed columns plus noise), an age-like one, a 0 / 1 one and a fourth equal to marker TRIP's imputed column plus 3 % noise (its
    variance-inflation factor between VIF and VIF_LOOSE).  Phenotype 3 is marker NEAR plus 1e-3 noise, phenotype 4 exactly collinear
    with marker COLL once the first three covariates are taken out.  Y0: the same five before the covariate effects are added (the
    marginal screen's: phenotype 4 exactly collinear with COLL as it stands)."""
    key = (bits, missing)
    if key in _FIX:
        return _FIX[key]
    N, M = N_FIX, M_FIX
    rng = np.random.default_rng(1000 + bits + (1 if missing else 0))
    top = reserved(bits)
    # dosage-like codes: allele frequency per marker, genotype 0 / 1 / 2 copies plus imputation noise, on the grid of the default scale
    unit = 127 if bits == 8 else 16384
    f = rng.uniform(0.05, 0.5, M)
    g = rng.binomial(2, f[:, None], (M, N)).astype(np.float64) + 0.15 * rng.standard_normal((M, N))
    B = np.clip(np.rint(np.clip(g, 0.0, 2.0) * unit), 0, top - 1).astype(np.int64)
    B[CONST] = 77
    m4, pres, nonas = present_mask(N)
    if missing:
        B[rng.random((M, N)) < 0.05] = top
        B[ALLMISS] = top
        B[ONE] = top
        B[ONE, np.nonzero(pres)[0][9]] = 100
        B[ONE, np.nonzero(~pres)[0][2]] = 50          # (a present entry outside the mask does not count)
        B[CONST, ::5] = top
        for m in (TRIP, NEAR, COLL):
            assert np.sum(B[m][pres] != top) > 400
    B = B.astype(np.uint8 if bits == 8 else np.uint16)
    scale = 1.0 / unit
    code, have = decode(B, bits, missing)

    def imputed(m):
        h = have[m] & pres
        return scale * np.where(have[m], code[m], code[m][h].mean())

    free = np.setdiff1d(np.arange(M), [ALLMISS, ONE, CONST, TRIP, NEAR, COLL])
    anc = np.sort(rng.choice(free, 20, replace=False))
    w = rng.standard_normal(20)
    Cov = np.empty((4, N))
    Cov[0] = sum(wi * imputed(m) for wi, m in zip(w, anc)) + 2.0 * rng.standard_normal(N)
    Cov[1] = 55.0 + 8.0 * rng.standard_normal(N)
    Cov[2] = (rng.random(N) < 0.45).astype(np.float64)
    gt = imputed(TRIP)
    Cov[3] = gt + 0.03 * gt[pres].std() * rng.standard_normal(N)
    Y = rng.standard_normal((5, N)) * np.array([1.0, 1e-3, 50.0, 1.0, 1.0])[:, None] + np.array([0.0, 4.0, -30.0, 0.0, 0.0])[:, None]
    Y[3] = imputed(NEAR) + 1e-3 * rng.standard_normal(N)
    Y[4] = 3.0 - 2.0 * imputed(COLL)
    Y0 = Y.copy()
    Y0[:, ~pres] = np.nan
    eff = np.array([[0.3, 0.02, -0.5], [1e-4, 1e-5, 2e-4], [4.0, -0.9, 10.0], [0.1, 0.01, 0.2], [-0.2, 0.03, 0.4]])
    Y = Y + eff @ Cov[:3]
    Y[:, ~pres] = np.nan
    Cov[:, ~pres] = np.nan
    novar = [CONST] + ([ALLMISS, ONE] if missing else [])
    for a in (B, m4, pres, Y, Y0, Cov):
        a.setflags(write=False)
    _FIX[key] = dict(bits=bits, missing=missing, N=N, M=M, B=B, scale=scale, m4=m4, present=pres, nonas=nonas, Y=Y, Y0=Y0, Cov=Cov, anc=anc,
                     novar=sorted(novar))
    return _FIX[key]


def random_covariates(fx, K, seed=23):
    Cov = np.random.default_rng(seed + K).standard_normal((K, fx["N"]))
    Cov[:, ~fx["present"]] = np.nan
    return Cov
