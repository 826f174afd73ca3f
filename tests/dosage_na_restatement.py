"""Restatement of compact dosage data with missing entries (include/gvamp.h, gv_set_dosage_missing), in numpy, kept apart from the
library's code and written from the definitions of the header, not from the kernels.

With the option on b_kn = 0 where the code of marker k, individual n is the reserved (all-ones) one, 1 otherwise; na_n is the
phenotype mask:
    cnt_k  = sum_n b na                                  (an exact integer)
    mu'_k  = (sum_n code b na) / cnt_k                   (the integer sum exact; 0 when cnt_k == 0)
    q_k    = sum_n ((code - mu'_k) b na)^2
    msig_k = 1 if q_k == 0 else (scale sqrt(q_k / (nonas - 1)))^-alpha;     mave_k = scale mu'_k
    A_nk   = (code - mu'_k) (msig_k scale) b_kn / sqrt(N)      -- no phenotype mask in the operator (the dense rule)
With the option off b == 1 and the definition is the one tests/test_gpu_dosage.py restates.  numpy long double is the yardstick;
`dtype=np.float64` gives the same expressions in plain float64 (the measure of what another summation order may deviate)."""
import numpy as np

import assoc_restatement as ar

LD = np.longdouble


def reserved(bits):
    return (1 << bits) - 1


def stats(B, bits, na, scale, alpha=1.0, missing=True, dtype=LD):
    """B: M x N codes; na: N zeros / ones.  Returns a dict: b (M x N, dtype), cnt (int64), mu, q, mave, msig, D = (B - mu') b,
    w = msig scale, scale, N, nonas"""
    B = np.asarray(B)
    M, N = B.shape
    nai = np.asarray(na).astype(np.int64)
    nonas = int(nai.sum())
    bi = (B != reserved(bits)).astype(np.int64) if missing else np.ones(B.shape, dtype=np.int64)
    P = bi * nai[None, :]
    cnt = P.sum(axis=1)
    s = (B.astype(np.int64) * P).sum(axis=1)
    mu = np.where(cnt != 0, s.astype(dtype) / np.where(cnt != 0, cnt, 1).astype(dtype), dtype(0))
    b = bi.astype(dtype)
    D = (B.astype(dtype) - mu[:, None]) * b
    Dn = D * nai.astype(dtype)[None, :]
    q = (Dn * Dn).sum(axis=1)
    sd = dtype(scale) * np.sqrt(np.where(q != 0, q, dtype(1)) / dtype(max(nonas - 1, 1)))
    msig = np.where(q != 0, sd ** dtype(-alpha), dtype(1))
    return dict(b=b, cnt=cnt, mu=mu, q=q, mave=dtype(scale) * mu, msig=msig, D=D, w=msig * dtype(scale), scale=scale, N=N,
                nonas=nonas, dtype=dtype)


def matrix(st):
    """the operator, N x M: A_nk = (code - mu'_k) (msig_k scale) b_kn / sqrt(N)"""
    dt = st["dtype"]
    return (st["D"] * st["w"][:, None]).T / np.sqrt(dt(st["N"]))


def ax(st, x, npad):
    """gv_ax: A x at the N individuals, exact zeros at the pad slots"""
    dt = st["dtype"]
    out = np.zeros(npad, dtype=dt)
    out[:st["N"]] = (st["D"].T @ (st["w"] * np.asarray(x, dtype=dt))) / np.sqrt(dt(st["N"]))
    return out


def atx(st, p):
    """gv_atx: A^T p, p as given (first N entries)"""
    dt = st["dtype"]
    return st["w"] * (st["D"] @ np.asarray(p[:st["N"]], dtype=dt)) / np.sqrt(dt(st["N"]))


def lmmse_mult(st, x, tau, gam2):
    """gv_lmmse_mult: tau A^T A x + gam2 x"""
    dt = st["dtype"]
    return dt(tau) * atx(st, ax(st, x, st["N"])) + dt(gam2) * np.asarray(x, dtype=dt)


def assoc(st, na, y, z1, x1, chrom=None, with_p=True):
    """gv_assoc_loo (chrom None) / gv_assoc_loco: value_n = (code - mu') (msig scale) b na, the sample size of marker k is cnt_k;
    sumy and sumsqy run over b na (data.cpp:1164-1176, as tests/assoc_restatement.py restates them for bed data).  A marker with
    cnt_k < 3 or q_k == 0 gives NaN in all four outputs (LOCO: where its chromosome is tested at all)."""
    dt = st["dtype"]
    V = st["D"] * st["w"][:, None]
    out = ar.assoc(V, st["b"], na, y, z1, x1, chrom=chrom, dtype=dt, with_p=with_p)
    dead = (st["cnt"] < 3) | (st["q"] == 0)
    if chrom is not None:
        c = np.asarray(chrom)
        dead &= (c >= 1) & (c <= 23)
    for v in out.values():
        v[dead] = dt("nan")
    return out
