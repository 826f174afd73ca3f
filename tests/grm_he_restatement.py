"""Numpy restatement of the GRM-times-panel product and of Haseman-Elston regression (gv_grm_apply / gv_grm_he),
written from the contract in include/gvamp.h and not from the kernel:

  operators     G0, G1, G2 of a dense (A, M_ij): zero diagonal, zero where M_ij = 0, G2 = fl(A A)
  apply_chain   the literal summation chains of the contract in float64 -- numpy has no FMA, which is why the contract has none
  apply_ref     G w in np.longdouble from the reference A, and absT = |G| |w|
  apply_bound   the derived bounds of the GPU test for g1 and g2
  columns       K, the standardisation and the three columns k, yt, yt^2 of a trait
  he            the estimator from the six sums and its delete-one jackknife from the row terms, in any dtype
  he_pairs      the same regression from the explicit pair list: np.polyfit and a literal OLS
  he_jack_literal   delete each individual, rebuild the pair list, refit
  he_bound      first-order propagation through he's formulas of a relative error eps on each sum's absolute-value companion
Test infrastructure only."""
import numpy as np

FIELDS = ("n_ind", "n_pairs", "sum_a", "sum_aa", "h2", "intercept", "se_ols", "se_jack")
DERIVED = FIELDS[4:]
BATCH = 10          # traits per gv_grm_apply call of gv_grm_he: three columns each


def operators(A, Mc, dtype=np.float64):
    """(G0, G1, G2) as dense N x N arrays of dtype"""
    A = np.asarray(A)
    N = A.shape[0]
    on = (np.asarray(Mc) > 0) & ~np.eye(N, dtype=bool)
    G1 = np.where(on, np.where(on, A, 0.0), 0.0).astype(np.float64)
    G2 = G1 * G1                                    # rounded to fp64 before anything is multiplied into it
    return on.astype(dtype), G1.astype(dtype), G2.astype(dtype)


def apply_chain(A, Mc, W):
    """(g0, g1, g2), N x C float64: per 64-individual source group the chain over j ascending, from +0.0, of acc = acc + Gp_ij * w_jc
    (two roundings), then the chain over the groups ascending, from +0.0, of acc = acc + b_S"""
    W = np.ascontiguousarray(W, dtype=np.float64)
    N, C = W.shape
    out = []
    for G in operators(A, Mc):
        acc = np.zeros((N, C))
        for s0 in range(0, N, 64):
            b = np.zeros((N, C))
            for j in range(s0, min(N, s0 + 64)):
                b = b + G[:, j:j + 1] * W[j:j + 1, :]
            acc = acc + b
        out.append(acc)
    return tuple(out)


def apply_ref(r, W):
    """((g0, g1, g2), (abs0, abs1, abs2)) in np.longdouble from the reference r (a dict of grm_restatement.grm): Gp w and |Gp| |w|"""
    Wl = np.asarray(W, dtype=np.longdouble)
    Gs = operators(r["A"], r["M_ij"], np.longdouble)
    Gs = (Gs[0], Gs[1], Gs[1] * Gs[1])              # the reference squares exactly (to long double)
    return tuple(G @ Wl for G in Gs), tuple(np.abs(G) @ np.abs(Wl) for G in Gs)


def apply_bound(r, e, W):
    """(bound of g1, bound of g2), N x C, of a library output against apply_ref, with e the entry bound of A (grm_restatement.bound):
        g1: sum_j (e_ij + 2^-52 |A_ij|) |w_jc| + (N + 2) 2^-53 absT1
            -- the entry's own error; the rounding of the product and of the reference entry; an N-term sum in any order
        g2: sum_j (e2_ij + 2^-52 A_ij^2) |w_jc| + (N + 2) 2^-53 absT2,   e2 = 2 |A| e + e^2 + 2^-53 (|A| + e)^2
            -- (A + d)^2 = A^2 + 2 A d + d^2 with |d| <= e, and the rounding of the square"""
    u = 2.0 ** -53
    N = r["A"].shape[0]
    on, G1, G2 = operators(r["A"], r["M_ij"])
    aw = np.abs(np.asarray(W, dtype=np.float64))
    e = np.where(on > 0, e, 0.0)
    a1 = np.abs(G1)
    e2 = 2.0 * a1 * e + e * e + u * (a1 + e) ** 2
    b1 = (e + 2.0 * u * a1) @ aw + (N + 2) * u * (a1 @ aw)
    b2 = (e2 + 2.0 * u * G2) @ aw + (N + 2) * u * (G2 @ aw)
    return b1, b2


def columns(y, dtype=np.float64):
    """(k, yt, yt2, usable) of one trait (NaN = missing): m = sum y / n_K, v = sum (y - m)^2 / (n_K - 1), yt = (y - m) / sqrt(v) on K"""
    y = np.asarray(y, dtype=np.float64)
    K = ~np.isnan(y)
    nk = int(K.sum())
    k = K.astype(dtype)
    yt = np.zeros(len(y), dtype=dtype)
    usable = False
    if nk > 1:
        yk = y[K].astype(dtype)
        m = yk.sum() / dtype(nk)
        v = ((yk - m) ** 2).sum() / dtype(nk - 1)
        usable = bool(v > 0 and np.isfinite(v))
        if usable:
            yt[K] = (yk - m) / np.sqrt(v)
    return k, yt, yt * yt, usable


def panel(Y):
    """the N x 3 C panel of the traits Y (N x C): columns k, yt, yt^2 of each, and the usable flags"""
    Y = np.asarray(Y, dtype=np.float64).reshape(len(Y), -1)
    cols, usable = [], []
    for c in range(Y.shape[1]):
        k, yt, y2, ok = columns(Y[:, c])
        cols += [k, yt, y2]
        usable.append(ok)
    return np.stack(cols, axis=1), usable


def _h2(n, sx, sxx, sz, sxz):
    with np.errstate(divide="ignore", invalid="ignore"):
        D = n * sxx - sx * sx
        return np.where((n >= 3) & (D > 0), (n * sxz - sx * sz) / np.where(D > 0, D, 1), np.nan)


def he(w3, g0, g1, g2, usable=True, dtype=np.float64):
    """the record of one trait from its three columns w3 = (k, yt, yt^2) (N x 3) and the matching columns of G0 w, G1 w, G2 w"""
    w3, g0, g1, g2 = (np.asarray(x).astype(dtype) for x in (w3, g0, g1, g2))
    k, yt, y2 = w3[:, 0], w3[:, 1], w3[:, 2]
    rows = dict(n=k * g0[:, 0], sx=k * g1[:, 0], sxx=k * g2[:, 0], sz=yt * g0[:, 1], szz=y2 * g0[:, 2], sxz=yt * g1[:, 1])
    s = {key: v.sum() / dtype(2) for key, v in rows.items()}
    nan = dtype(np.nan)
    out = dict(n_ind=int(round(float(k.sum()))), n_pairs=int(round(float(s["n"]))), sum_a=s["sx"], sum_aa=s["sxx"])
    h2 = dtype(_h2(s["n"], s["sx"], s["sxx"], s["sz"], s["sxz"])) if usable else nan
    if np.isnan(h2):
        out.update(h2=nan, intercept=nan, se_ols=nan, se_jack=nan)
        return out
    D = s["n"] * s["sxx"] - s["sx"] * s["sx"]
    c0 = (s["sz"] - h2 * s["sx"]) / s["n"]
    rss = s["szz"] - c0 * s["sz"] - h2 * s["sxz"]
    with np.errstate(invalid="ignore"):
        se = np.sqrt(rss / (s["n"] - 2) * s["n"] / D)
    K = k != 0
    hj = _h2(*[(s[key] - rows[key][K]) for key in ("n", "sx", "sxx", "sz", "sxz")]).astype(dtype)
    nk = dtype(K.sum())
    se_jack = np.sqrt((nk - 1) / nk * ((hj - hj.sum() / nk) ** 2).sum())
    out.update(h2=h2, intercept=c0, se_ols=se, se_jack=se_jack, h2_jack=hj)
    return out


def he_traits(Y, apply_fn, dtype=np.float64):
    """he of every column of Y through apply_fn(W) -> (g0, g1, g2): a list of records"""
    W, usable = panel(Y)
    g = apply_fn(W)
    return [he(W[:, 3 * c:3 * c + 3], g[0][:, 3 * c:3 * c + 3], g[1][:, 3 * c:3 * c + 3], g[2][:, 3 * c:3 * c + 3], usable[c], dtype)
            for c in range(len(usable))]


def pair_list(A, Mc, y):
    """(i, j, x, z, yt) of the regression: i < j in K with M_ij > 0, x = A_ij, z = yt_i yt_j"""
    k, yt, _, usable = columns(y)
    i, j = np.triu_indices(len(yt), 1)
    keep = (k[i] != 0) & (k[j] != 0) & (np.asarray(Mc)[i, j] > 0)
    i, j = i[keep], j[keep]
    return i, j, np.asarray(A)[i, j], yt[i] * yt[j], yt


def _ols(x, z):
    """(slope, intercept, se of the slope) by the textbook formulas on centred data"""
    n = len(x)
    xm, zm = x.mean(), z.mean()
    sxx = ((x - xm) ** 2).sum()
    b = ((x - xm) * (z - zm)).sum() / sxx
    a = zm - b * xm
    rss = ((z - a - b * x) ** 2).sum()
    return b, a, np.sqrt(rss / (n - 2) / sxx)


def he_pairs(A, Mc, y):
    """dict n_pairs, sum_a, sum_aa, h2, intercept, se_ols of the explicit pair list, and the np.polyfit pair (slope, intercept)"""
    i, j, x, z, _ = pair_list(A, Mc, y)
    b, a, se = _ols(x, z)
    return dict(n_pairs=len(x), sum_a=x.sum(), sum_aa=(x * x).sum(), h2=b, intercept=a, se_ols=se, polyfit=tuple(np.polyfit(x, z, 1)))


def he_jack_literal(A, Mc, y):
    """(se_jack, h2_(-i) for i in K): every individual of K deleted in turn, the standardisation of the full K kept"""
    i, j, x, z, _ = pair_list(A, Mc, y)
    K = np.flatnonzero(~np.isnan(np.asarray(y, dtype=np.float64)))
    hj = np.array([_ols(x[(i != d) & (j != d)], z[(i != d) & (j != d)])[0] for d in K])
    nk = len(K)
    return np.sqrt((nk - 1) / nk * ((hj - hj.mean()) ** 2).sum()), hj


def he_bound(r, y, eps):
    """dict h2, intercept, se_ols, se_jack: the first-order bound of the error of he's results when every sum S = u' G v / 2 carries an
    error of at most eps * |u|' Gbar |v| / 2, its absolute-value companion.  Gbar is G0 for the sums in G0 (n itself is an exact
    integer: no error), Abar = absS / M_ij >= |A| for those in G1 and Abar^2 for Sxx -- an entry's error is relative to Abar, not to
    |A| (grm_restatement.bound).  For the jackknife, h_i = f(S - q_i) with q_i the row terms: the error of the full sums S is common
    to every h_i and reaches h_i - mean(h) only through the difference of the gradients, |f'(S - q_i) - mean f'| dS; the rows' own errors
    dq_i enter in full, |f'_i| dq_i + mean_l |f'_l| dq_l."""
    on, G1, G2 = operators(r["A"], r["M_ij"])
    with np.errstate(divide="ignore", invalid="ignore"):
        Abar = np.where(on > 0, r["absS"] / np.maximum(r["M_ij"], 1), 0.0)
    k, yt, y2, usable = columns(y)
    ay = np.abs(yt)
    rows = dict(n=k * (on @ k), sx=k * (G1 @ k), sxx=k * (G2 @ k), sz=yt * (on @ yt), szz=y2 * (on @ y2), sxz=yt * (G1 @ yt))
    arow = dict(n=0.0 * k, sx=eps * k * (Abar @ k), sxx=eps * k * ((Abar * Abar) @ k), sz=eps * ay * (on @ ay), szz=eps * y2 * (on @ y2),
                sxz=eps * ay * (Abar @ ay))
    s = {key: v.sum() / 2 for key, v in rows.items()}
    d = {key: v.sum() / 2 for key, v in arow.items()}

    def h2_and_gradient(s):
        D = s["n"] * s["sxx"] - s["sx"] ** 2
        h2 = (s["n"] * s["sxz"] - s["sx"] * s["sz"]) / D
        return h2, dict(sxz=s["n"] / D, sx=(2 * h2 * s["sx"] - s["sz"]) / D, sz=-s["sx"] / D, sxx=-h2 * s["n"] / D), D

    h2, grad, D = h2_and_gradient(s)
    bh = sum(abs(grad[key]) * d[key] for key in grad)
    c0 = (s["sz"] - h2 * s["sx"]) / s["n"]
    bc = (d["sz"] + abs(h2) * d["sx"] + abs(s["sx"]) * bh) / s["n"]
    rss = s["szz"] - c0 * s["sz"] - h2 * s["sxz"]
    brss = d["szz"] + abs(c0) * d["sz"] + abs(s["sz"]) * bc + abs(h2) * d["sxz"] + abs(s["sxz"]) * bh
    bD = s["n"] * d["sxx"] + 2 * abs(s["sx"]) * d["sx"]
    se = np.sqrt(rss / (s["n"] - 2) * s["n"] / D)
    bse = 0.5 * se * (brss / abs(rss) + bD / abs(D))
    K = k != 0
    hj, gj, _ = h2_and_gradient({key: s[key] - rows[key][K] for key in s})
    own = sum(np.abs(gj[key]) * arow[key][K] for key in gj)
    bdev = sum(np.abs(gj[key] - gj[key].mean()) * d[key] for key in gj) + own + own.mean()
    nk = K.sum()
    f = (nk - 1) / nk
    dev = hj - hj.mean()
    sej = np.sqrt(f * (dev ** 2).sum())
    bsej = f * (2 * np.abs(dev) * bdev).sum() / (2 * sej)
    return dict(h2=bh, intercept=bc, se_ols=bse, se_jack=bsej)


def traits(r, seed, n=3):
    """the traits of the tests on case r, N x n: column 0 a standardised genetic value Z beta plus noise (h2 about 0.5), column 1
    standard normal with 10 % missing, the rest standard normal"""
    rng = np.random.default_rng(seed)
    N, M = r["Z"].shape
    Y = rng.standard_normal((N, n))
    gval = r["Z"] @ rng.standard_normal(M)
    sd = gval.std()
    Y[:, 0] = (gval / sd if sd > 0 else 0.0) + rng.standard_normal(N)
    if n > 1:
        Y[rng.random(N) < 0.1, 1] = np.nan
    return Y
