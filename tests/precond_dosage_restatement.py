"""Restatement of the LD-block preconditioner's window Grams of 8-bit dosage codes (include/gvamp.h), written from
the definition: the integers X_jk, c_j, T_j of tests/ld_dosage_restatement.py, the statistics of tests/assoc_restatement.py
(dosage_columns) / tests/dosage_na_restatement.py, and the ONE fp64 evaluation order of the header, symmetric in j and k:

    G_jk = ((s_j * s_k) * (1 / N)) * (fl(X_jk) / (fl(c_j) * fl(c_k))),    s_j = msig_j * scale

with exact zeros for a row with c_j = 0.  Windows, the two grids, the factorisation and the apply are those of
tests/precond_restatement.py.  Test infrastructure only."""
import numpy as np

import assoc_restatement as ar
import dosage_na_restatement as dnr
import ld_dosage_restatement as ldd

LD = np.longdouble
SCALE = 1.0 / 127.0


def msig(codes, na=None, missing=False, scale=SCALE, dtype=LD):
    """msig of the contract in code units (long double by default); missing: the reserved code 255 is a missing entry"""
    codes = np.asarray(codes)
    na = np.ones(codes.shape[1]) if na is None else np.asarray(na)
    if missing:
        return dnr.stats(codes, 8, na, scale, missing=True, dtype=dtype)["msig"]
    return ar.dosage_columns(codes, scale, na, dtype=dtype)[2]


def matrix(codes, na=None, missing=False, scale=SCALE, dtype=LD):
    """A, N x M: A_nj = (code_nj - mu'_j) s_j b_nj na_n / sqrt(N), s_j = msig_j * scale -- the matrix whose Gram the windows hold"""
    codes = np.asarray(codes)
    N = codes.shape[1]
    na = np.ones(N) if na is None else np.asarray(na)
    st = dnr.stats(codes, 8, na, scale, missing=missing, dtype=dtype)
    return (st["D"] * st["w"][:, None] * na.astype(dtype)[None, :]).T / np.sqrt(dtype(N))


def gram(codes, na=None, missing=False, scale=SCALE, ms=None):
    """the M x M integer Gram of all the rows of codes in the header's fp64 order; ms: msig as float64 (default: the restatement's)"""
    codes = np.asarray(codes)
    M, N = codes.shape
    s = ldd.sums(codes, na, missing)
    Xf = ldd._tofloat(ldd.centred(s)).astype(np.float64)
    c = s["c"].astype(np.float64)
    ms = np.asarray(msig(codes, na, missing, scale), dtype=np.float64) if ms is None else np.asarray(ms, dtype=np.float64)
    sj = ms * np.float64(scale)
    ok = (c[:, None] != 0) & (c[None, :] != 0)
    den = np.where(ok, c[:, None] * c[None, :], 1.0)
    inv_n = 1.0 / np.float64(N)
    return np.where(ok, ((sj[:, None] * sj[None, :]) * inv_n) * (Xf / den), 0.0)


def window_gram(codes, S, lo, hi, na=None, missing=False, scale=SCALE, ms=None):
    """G of the window [lo, hi) (global marker indices) of a shard that starts at S"""
    sl = slice(lo - S, hi - S)
    return gram(np.asarray(codes)[sl], na, missing, scale, None if ms is None else np.asarray(ms)[sl])
