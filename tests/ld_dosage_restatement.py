"""Restatement of the LD of 8-bit dosage codes (gv_set_ld_dosage, include/gvamp.h) in Python integers: the
integer sums of the planes, the centred product X_jk formed without any rounding (object arrays of Python ints), float(int) -- which
rounds correctly -- and r = fl(X_jk) / sqrt(fl(X_jj) fl(X_kk)).  Band and scores are those of ld_restatement.  Test infrastructure
only."""
import numpy as np

import ld_restatement as ldr

scores, band, in_band = ldr.scores, ldr.band, ldr.in_band
_tofloat = np.frompyfunc(float, 1, 1)


def planes(codes, na=None, missing=False):
    """P = b na and V = (code - 128) P as int64 (M x N); b = 0 at the reserved code 255 when `missing`, 1 otherwise"""
    codes = np.asarray(codes)
    M, N = codes.shape
    na = np.ones(N) if na is None else np.asarray(na)
    b = codes != 255 if missing else np.ones((M, N), dtype=bool)
    P = (b & (na != 0)[None, :]).astype(np.int64)
    return P, (codes.astype(np.int64) - 128) * P


def sums(codes, na=None, missing=False):
    """the exact integer sums over the individuals: dict of VV, VP (VP[j][k] = sum V_j P_k), PP (M x M) and c, T (M), int64"""
    P, V = planes(codes, na, missing)
    return dict(VV=V @ V.T, VP=V @ P.T, PP=P @ P.T, c=P.sum(1), T=V.sum(1))


def centred(s):
    """X_jk = c_j c_k VV_jk - c_j T_k VP_jk - c_k T_j VP_kj + T_j T_k PP_jk as an M x M object array of Python integers"""
    o = lambda a: np.asarray(a).astype(object)
    c, T = o(s["c"]), o(s["T"])
    return (c[:, None] * c[None, :] * o(s["VV"]) - c[:, None] * T[None, :] * o(s["VP"]) - T[:, None] * c[None, :] * o(s["VP"].T)
            + T[:, None] * T[None, :] * o(s["PP"]))


def corr(X):
    """(r, poly) from the integers: r_jk = float(X_jk) / sqrt(float(X_jj) float(X_kk)), evaluated for j < k and mirrored; monomorphic
    iff X_jj == 0; r_jj = 1 for a polymorphic marker, r_jk = 0 if either marker is monomorphic"""
    M = X.shape[0]
    poly = np.array([X[j, j] != 0 for j in range(M)], dtype=bool)
    Xf = _tofloat(X).astype(np.float64)
    d = np.diag(Xf).copy()
    den = np.sqrt(d[:, None] * d[None, :])
    U = np.triu(np.where(poly[:, None] & poly[None, :], Xf / np.where(den != 0, den, 1.0), 0.0), 1)
    r = U + U.T
    r[np.diag_indices(M)] = poly.astype(np.float64)
    return r, poly


def ld(codes, na=None, missing=False):
    """dict of r (M x M, unbanded), poly and the integers X"""
    X = centred(sums(codes, na, missing))
    r, poly = corr(X)
    return {"r": r, "poly": poly, "X": X}


def abs_terms(r, poly, B, chrom=None, adjusted=False, nonas=None):
    """sum over the marker's band of |f(r_jk^2)|: what the bar of l_j scales with"""
    M = r.shape[0]
    terms = in_band(M, B, chrom) & poly[None, :] & ~np.eye(M, dtype=bool)
    x = r * r
    f = x - (1.0 - x) / (nonas - 2.0) if adjusted else x
    return np.where(terms, np.abs(f), 0.0).sum(1)


def rare_rows(N=1003, M=200, seed=5):
    """rare-variant rows: code 253 with 1 % of 254"""
    rng = np.random.default_rng(seed)
    return np.where(rng.random((M, N)) < 0.01, 254, 253).astype(np.uint8)


def bound_case(N=140000, M=70, seed=9):
    """row 0 alternates 0 / 255, row 1 is 255 - row 0 (the missing option off: 255 is a value): |VV_00| and |VV_01| exceed 2^31"""
    codes = np.random.default_rng(seed).integers(0, 256, size=(M, N), dtype=np.uint8)
    codes[0] = np.where(np.arange(N) % 2 == 0, 0, 255)
    codes[1] = 255 - codes[0]
    return codes
