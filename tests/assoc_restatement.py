"""Restatement of the per-marker association test of include/gvamp.h (gv_assoc_*), in numpy, kept apart from the library's code.

Written from the lines the definition cites: the sums of data::pvals_calc / pvals_calc_LOCO (data.cpp:1145-1176, :1262-1284) and the
regression of linear_reg1d_pvals (utilities.cpp:321-334), whose commented-out effect size is restored as beta = sxy / s2x.  Everything
works on a decoded matrix -- the standardised columns V[k, n] = (x_kn - mave_k) msig_k b_kn, before the phenotype mask -- in the dtype
the caller names: numpy long double is the yardstick, plain float64 the measure of what a float64 evaluation in another summation
order may deviate from it.  The Student-t tail is evaluated here as well (incomplete beta function by its continued fraction, DLMF
8.17.22), so the module needs numpy alone."""
import math

import numpy as np

LD = np.longdouble
_lgamma = np.vectorize(math.lgamma, otypes=[np.float64])


def _beta_cf(a, b, x):
    """Lentz evaluation of the continued fraction of I_x(a, b) (DLMF 8.17.22), arrays in long double"""
    tiny = LD(1e-300)
    one = LD(1)

    def guard(v):
        return np.where(np.abs(v) < tiny, tiny, v)

    c = np.ones_like(x)
    d = one / guard(one - (a + b) * x / (a + one))
    h = d.copy()
    live = np.ones(x.shape, dtype=bool)
    for m in range(1, 100000):
        m2 = LD(2 * m)
        num = LD(m) * (b - LD(m)) * x / ((a - one + m2) * (a + m2))
        d = one / guard(one + num * d)
        c = guard(one + num / c)
        h = np.where(live, h * d * c, h)
        num = -(a + LD(m)) * (a + b + LD(m)) * x / ((a + m2) * (a + one + m2))
        d = one / guard(one + num * d)
        c = guard(one + num / c)
        delta = d * c
        h = np.where(live, h * delta, h)
        live &= np.abs(delta - one) >= LD(1e-19)
        if not live.any():
            break
    return h


def t_two_sided(t, nu):
    """P(|T_nu| > |t|) = I_x(nu / 2, 1 / 2), x = nu / (nu + t^2); NaN where t is NaN or nu <= 0"""
    t = np.abs(np.asarray(t, dtype=LD))
    nu = np.broadcast_to(np.asarray(nu, dtype=LD), t.shape)
    out = np.full(t.shape, LD("nan"))
    ok = np.isfinite(t) & (nu > 0)
    out[ok & (t == 0)] = LD(1)
    out[np.isinf(t) & (nu > 0)] = LD(0)
    ok &= t != 0
    if ok.any():
        tt, a, b = t[ok], nu[ok] / LD(2), LD(0.5)
        w = tt * tt / nu[ok]
        x = LD(1) / (LD(1) + w)
        a64 = a.astype(np.float64)
        lnB = (_lgamma(a64 + 0.5) - _lgamma(a64) - math.lgamma(0.5)).astype(LD)       # -ln B(a, 1/2)
        front = np.exp(lnB - a * np.log1p(w) + b * (np.log(w) - np.log1p(w)))
        direct = x < (a + LD(1)) / (a + b + LD(2))
        res = np.empty(tt.shape, dtype=LD)
        if direct.any():
            res[direct] = front[direct] * _beta_cf(a[direct], np.full(int(direct.sum()), b), x[direct]) / a[direct]
        if (~direct).any():
            o = ~direct
            res[o] = LD(1) - front[o] * _beta_cf(np.full(int(o.sum()), b), a[o], LD(1) - x[o]) / b
        out[ok] = res
    return out


def reg1d(sumx, sumsqx, sumxy, sumy, sumsqy, n, with_p=True):
    """utilities.cpp:321-334 with the effect restored; se = beta / t written without the quotient (t == 0 gives no 0/0).  n < 3 -- no
    degree of freedom left for the test -- gives NaN in every output (include/gvamp.h)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        s2y = (sumsqy - sumy * sumy / n) / (n - 1)
        s2x = (sumsqx - sumx * sumx / n) / (n - 1)
        sxy = (sumxy - sumx * sumy / n) / (n - 1)
        rxy = sxy / np.sqrt(s2x * s2y)
        t = rxy * np.sqrt((n - 2) / (1 - rxy * rxy))
        beta = sxy / s2x
        se = np.sqrt((n - 1) / (n - 2) * s2y * (1 - rxy * rxy) / ((n - 1) * s2x))
    out = dict(beta=beta, se=se, t=t)
    for k in out:
        out[k] = np.where(np.asarray(n) < 3, np.asarray(beta).dtype.type("nan"), out[k])
    if with_p:
        out["p"] = t_two_sided(t, n - 2)
    return out


def bed_columns(G, have, mave, msig, dtype=LD):
    """bed data: V = (a - mave) msig b with a the hard call and b = 1 where the genotype is present (dotp_lut_a / dotp_lut_b)"""
    b = np.asarray(have, dtype=dtype)
    V = (np.asarray(G, dtype=dtype) - np.asarray(mave, dtype=dtype)[:, None]) * np.asarray(msig, dtype=dtype)[:, None] * b
    return V, b


def dosage_columns(codes, scale, na, alpha=1.0, dtype=LD):
    """compact dosage data, in code units as the header defines them: mu' = (sum_present code) / nonas with the integer sum exact,
    q = sum_present (code - mu')^2, msig = 1 if q == 0 else (scale sqrt(q / (nonas - 1)))^-alpha; V = (code - mu') (msig scale), b == 1
    (returned as None).  Also returns msig."""
    nai = np.asarray(na).astype(np.int64)
    nonas = int(nai.sum())
    mu = (codes.astype(np.int64) * nai[None, :]).sum(axis=1).astype(dtype) / dtype(nonas)
    D = codes.astype(dtype) - mu[:, None]
    q = ((D * D) * np.asarray(na, dtype=dtype)[None, :]).sum(axis=1)
    sd = dtype(scale) * np.sqrt(np.where(q != 0, q, dtype(1)) / dtype(max(nonas - 1, 1)))
    msig = np.where(q != 0, sd ** dtype(-alpha), dtype(1))
    D *= (msig * dtype(scale))[:, None]
    return D, None, msig


def assoc(V, b, na, y, z1, x1, chrom=None, dtype=LD, with_p=True, chunk=4096):
    """The four outputs of gv_assoc_loo (chrom None) / gv_assoc_loco for the standardised columns V (M x N, unmasked), b (M x N
    genotype-present flags or None for all ones), the 0/1 phenotype mask na, and y, z1 (first N entries used), x1 (M).
    value = V na;  LOO: y_mark = y - z1 + value x1[k] / sqrt(N);  LOCO: y_mark = y - z1 + sum_{m on k's chromosome} value_m x1[m] / sqrt(N);
    sumx = sum value, sumsqx = sum value^2, sumxy = sum value y_mark, sumy = sum y_mark b na, sumsqy = sum y_mark^2 b na, n = sum b na.
    The reference leaves y - z1 unmasked and multiplies every use by na; it is masked once here instead (a caller's y may hold
    anything at the NA slots).  LOCO: markers with a chromosome outside 1..23 get 0 in every output."""
    M, N = V.shape
    na = np.asarray(na, dtype=dtype)
    sqrtN = np.sqrt(dtype(N))
    x1 = np.asarray(x1, dtype=dtype)
    ymod = np.where(na != 0, np.asarray(y[:N], dtype=dtype) - np.asarray(z1[:N], dtype=dtype), dtype(0))
    S = {k: np.zeros(M, dtype=dtype) for k in ("sumx", "sumsqx", "sumxy", "sumy", "sumsqy", "n")}

    def column_sums(rows, Vn, bn):
        S["sumx"][rows] = Vn.sum(axis=1)
        S["sumsqx"][rows] = np.einsum("ij,ij->i", Vn, Vn)
        S["n"][rows] = na.sum() if bn is None else bn.sum(axis=1)

    if chrom is None:
        for m0 in range(0, M, chunk):
            sl = slice(m0, min(M, m0 + chunk))
            Vn = V[sl] * na[None, :]
            bn = None if b is None else b[sl] * na[None, :]
            ymark = Vn * (x1[sl] / sqrtN)[:, None]
            ymark += ymod[None, :]
            column_sums(sl, Vn, bn)
            S["sumxy"][sl] = np.einsum("ij,ij->i", Vn, ymark)
            if bn is None:                                   # b == 1: the factor b na is na
                S["sumy"][sl] = ymark @ na
                ymark *= ymark
                S["sumsqy"][sl] = ymark @ na
            else:
                S["sumy"][sl] = np.einsum("ij,ij->i", ymark, bn)
                S["sumsqy"][sl] = np.einsum("ij,ij,ij->i", ymark, ymark, bn)
        return reg1d(S["sumx"], S["sumsqx"], S["sumxy"], S["sumy"], S["sumsqy"], S["n"], with_p)
    chrom = np.asarray(chrom)
    tested = np.zeros(M, dtype=bool)
    for ch in range(1, 24):
        rows = np.nonzero(chrom == ch)[0]
        if rows.size == 0:
            continue
        tested[rows] = True
        Vn = V[rows] * na[None, :]
        bn = None if b is None else b[rows] * na[None, :]
        ymark = ymod + (x1[rows] / sqrtN) @ Vn              # one residual for the whole chromosome
        column_sums(rows, Vn, bn)
        S["sumxy"][rows] = Vn @ ymark
        S["sumy"][rows] = na @ ymark if bn is None else bn @ ymark
        S["sumsqy"][rows] = na @ (ymark * ymark) if bn is None else bn @ (ymark * ymark)
    S["n"][~tested] = dtype(3)        # (any n > 2 with zero sums: these rows are overwritten below)
    out = reg1d(S["sumx"], S["sumsqx"], S["sumxy"], S["sumy"], S["sumsqy"], S["n"], with_p)
    for v in out.values():
        v[~tested] = dtype(0)
    return out


def decode_bed(bed, N, M):
    """PLINK 2-bit rows -> (hard calls 0 / 1 / 2 with 0 at a missing genotype, genotype-present flags)"""
    mb = (N + 3) // 4
    b = np.asarray(bed, dtype=np.uint8).reshape(M, mb)
    codes = np.stack([(b >> (2 * k)) & 3 for k in range(4)], axis=2).reshape(M, 4 * mb)[:, :N]
    return np.choose(codes, [2, 0, 1, 0]).astype(np.int64), codes != 1
