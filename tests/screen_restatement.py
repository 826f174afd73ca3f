"""Restatement of the marginal association screen (gv_screen_dev), written from its definition and kept apart
from the library's code: decode the 2-bit genotypes, impute a missing genotype with the marker's mean over the phenotyped individuals
with a present genotype, and per (marker, phenotype column) take the Pearson correlation r over the n phenotyped individuals,
t = r sqrt((n - 2) / (1 - r^2)) and the two-sided tail p of Student's t with n - 2 degrees of freedom.  numpy long double by default;
dtype=np.float64 gives the same formulas in plain float64, whose deviation from long double is the yardstick of the GPU test (the rule
of section 15).

Rules: 1 - r^2 <= 0 gives t = +-inf and p = 0; a marker without variance among the phenotyped present genotypes (monomorphic or all
missing) gives NaN in all three."""
import numpy as np

import assoc_restatement as ar
import bed_fixed_restatement as bx

LD = np.longdouble


def genotypes(bed, N, M):
    """(a, have): M x N genotypes 0 / 1 / 2 and whether they are present (PLINK codes 00 / 10 / 11 = 2 / 1 / 0, 01 = missing)"""
    code = bx.decode(bed, N, M)[:, :N]
    a = np.select([code == 0, code == 2, code == 3], [2, 1, 0], 0)
    return a, code != 1


def screen(bed, N, M, present, Y, dtype=LD):
    """Y: C x N raw phenotype columns (entries at individuals outside `present` are ignored).  Returns dict r, t, p, each C x M"""
    present = np.ones(N, dtype=bool) if present is None else np.asarray(present, dtype=bool)
    a, have = genotypes(bed, N, M)
    a, have = a[:, present].astype(dtype), have[:, present]
    n = int(present.sum())
    cnt = have.sum(axis=1).astype(dtype)
    mu = np.where(cnt > 0, (a * have).sum(axis=1) / np.where(cnt > 0, cnt, dtype(1)), dtype(0))
    xc = np.where(have, a - mu[:, None], dtype(0))               # the mean-imputed column, centred: its mean is mu itself
    sxx = (xc * xc).sum(axis=1)
    novar = ~_differs(a, have)
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))[:, present].astype(dtype)
    yc = Y - (Y.sum(axis=1) / dtype(n))[:, None]
    syy = (yc * yc).sum(axis=1)
    sxy = yc @ xc.T                                              # C x M
    with np.errstate(invalid="ignore", divide="ignore"):
        r = sxy / np.sqrt(syy[:, None] * np.where(novar, dtype(1), sxx)[None, :])
        om = dtype(1) - r * r
        t = np.where(om <= 0, np.copysign(dtype(np.inf), r), r * np.sqrt(dtype(n - 2) / np.where(om <= 0, dtype(1), om)))
    p = ar.t_two_sided(t.astype(LD), n - 2).astype(dtype)
    p[np.isinf(t)] = 0
    r[:, novar], t[:, novar], p[:, novar] = np.nan, np.nan, np.nan
    return dict(r=r, t=t, p=p, novar=novar, n=n)


def _differs(a, have):
    """True for a marker whose present genotypes take more than one value (decided on the integers, no rounding involved)"""
    big = np.where(have, a, -np.inf).max(axis=1)
    small = np.where(have, a, np.inf).min(axis=1)
    return big > small


def deviation(got, ref, n, skip=()):
    """max deviation of r and t from the reference, each against its own magnitude plus the scale of its sampling noise (section 15):
    |dr| / (|r| + sqrt((1 - r^2) / (n - 2))), |dt| / (|t| + 1); entries where the reference is not finite and the (column, marker)
    entries of `skip` are left out"""
    g = {k: np.asarray(got[k], dtype=LD) for k in ("r", "t")}
    f = {k: np.asarray(ref[k], dtype=LD) for k in ("r", "t")}
    ok = np.isfinite(f["t"]) & np.isfinite(f["r"])
    for c, m in skip:
        ok[c, m] = False
    with np.errstate(invalid="ignore"):
        se = np.sqrt(np.maximum(LD(1) - f["r"] * f["r"], LD(0)) / LD(n - 2))
        dr = np.abs(g["r"] - f["r"]) / (np.abs(f["r"]) + se)
        dt = np.abs(g["t"] - f["t"]) / (np.abs(f["t"]) + 1)
    return dict(r=float(np.max(dr[ok])), t=float(np.max(dt[ok])))


def phenotypes(cs, seed=7):
    """the five raw columns of the tests on case cs (tests/bed_fixed_restatement.py): three normal ones, one equal to a marker's
    mean-imputed column plus 1e-3 noise (large |t|), one exactly collinear with a marker (the 1 - r^2 <= 0 rule).  Returns (Y, near,
    coll): Y is 5 x N with NaN at the individuals without a phenotype; near / coll are the two markers"""
    N, M, pres = cs["N"], cs["M"], np.asarray(cs["present"], dtype=bool)
    rng = np.random.default_rng(seed + M)
    a, have = genotypes(cs["bed"], N, M)
    near, coll = 17, 40
    assert near not in (bx.MONO, bx.ALLMISS) and coll not in (bx.MONO, bx.ALLMISS)

    def imputed(m):
        h = have[m] & pres
        return np.where(have[m], a[m], a[m][h].mean())

    Y = rng.standard_normal((5, N)) * np.array([1.0, 1e-3, 50.0, 1.0, 1.0])[:, None] + np.array([0.0, 4.0, -30.0, 0.0, 0.0])[:, None]
    Y[3] = imputed(near) + 1e-3 * rng.standard_normal(N)
    Y[4] = 3.0 - 2.0 * imputed(coll)                              # r = -1 exactly, up to the rounding of the sums
    Y[:, ~pres] = np.nan
    return Y, near, coll
