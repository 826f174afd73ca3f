"""Restatement of the principal components of the resident genotypes (gv_pca_dev) in plain numpy float64, written
from the definition and kept apart from the library's code:

  * a packer from a genotype array to PLINK .bed bytes and the Balding-Nichols inputs of the tests;
  * A and the dense G = (N / M) A A^T: decode, mask, mean-impute, centre, scale by msig, divide by sqrt(N);
  * numpy.linalg.eigh of G;
  * the block subspace iteration of the section (CholeskyQR applied twice, Rayleigh-Ritz, residuals from the Y of the iteration).

Inputs: Balding-Nichols genotypes with F_ST = 0.1 over k + 1 populations, 5 % missing genotypes, 3 % individuals without a phenotype,
one monomorphic and one all-missing marker.  `wide` and `many` take the block and k above 16.  The 5 x 3 shape keeps the monomorphic marker only and no NA phenotype: with both planted
markers one informative marker would be left and rank(G) < 2 = L."""
import numpy as np

EPS = 2.0 ** -52
FST = 0.1
# name -> N, M, k, L, seed
SHAPES = {
    "ragged": dict(N=1003, M=517, k=2, L=10, seed=101),
    "even": dict(N=2100, M=1100, k=2, L=10, seed=103),
    "four": dict(N=1003, M=517, k=4, L=12, seed=105),
    "second-step": dict(N=257, M=65, k=2, L=8, seed=110),
    "tile": dict(N=5, M=3, k=1, L=2, seed=109),
    "wide": dict(N=1003, M=517, k=2, L=20, seed=111),             # a block above 16: the 32-wide instantiations of the panel kernels
    "many": dict(N=1200, M=900, k=17, L=24, seed=113),            # k above 16 as well: 18 populations, a 32-wide residual Gram
}
PIVOT_EPS = 32.0 * EPS
_CACHE = {}


def pack_bed(a):
    """M x N genotypes (0 / 1 / 2 copies, -1 missing) -> PLINK .bed bytes without the header, marker-major, ceil(N / 4) bytes a marker:
    individual n at bits 2 (n & 3) of byte n >> 2, codes 00 / 10 / 11 = 2 / 1 / 0 copies, 01 = missing"""
    a = np.asarray(a)
    M, N = a.shape
    mb = (N + 3) // 4
    code = np.zeros((M, 4 * mb), dtype=np.uint8)
    code[:, :N] = np.select([a == 2, a == 1, a == 0], [0, 2, 3], 1)
    code = code.reshape(M, mb, 4)
    return (code[:, :, 0] | (code[:, :, 1] << 2) | (code[:, :, 2] << 4) | (code[:, :, 3] << 6)).astype(np.uint8).reshape(-1)


def mask4(present):
    present = np.asarray(present, dtype=bool)
    m4 = np.zeros((len(present) + 3) // 4, dtype=np.uint8)
    idx = np.nonzero(present)[0]
    np.bitwise_or.at(m4, idx >> 2, (1 << (idx & 3)).astype(np.uint8))
    return m4


def balding_nichols(N, M, npop, rng, fst=FST):
    """M x N genotypes: ancestral frequencies U(0.1, 0.9), population frequencies Beta(p (1 - F) / F, (1 - p) (1 - F) / F), individuals
    dealt to the populations in turn"""
    p = rng.uniform(0.1, 0.9, M)
    f = rng.beta(p[:, None] * (1 - fst) / fst, (1 - p[:, None]) * (1 - fst) / fst, (M, npop))
    pop = np.arange(N) % npop
    return rng.binomial(2, f[:, pop]).astype(np.int64)


def case(name):
    """dict N, M, k, L, a (M x N, -1 missing), bed, present, m4, nonas, q0 (L x N standard normals) of one shape"""
    if name in _CACHE:
        return _CACHE[name]
    sp = SHAPES[name]
    N, M, k, L = sp["N"], sp["M"], sp["k"], sp["L"]
    rng = np.random.default_rng(sp["seed"])
    a = balding_nichols(N, M, k + 1, rng)
    tiny = M < 8
    if not tiny:
        a[rng.random((M, N)) < 0.05] = -1
        a[M // 3] = -1                                         # all missing
    a[M // 2] = 2                                              # monomorphic
    present = np.ones(N, dtype=bool) if tiny else rng.random(N) >= 0.03
    q0 = rng.standard_normal((L, N))
    cs = dict(name=name, N=N, M=M, k=k, L=L, a=a, bed=pack_bed(a), present=present, m4=mask4(present), nonas=int(present.sum()), q0=q0)
    _CACHE[name] = cs
    return cs


def dense_A(a, present):
    """N x M: the matrix gv_ax_dev / gv_atx_dev apply.  Per marker over the phenotyped individuals with a present genotype: mu their
    mean, msig = 1 / sqrt(sum (a - mu)^2 / (nonas - 1)) (1 for a marker without variance); entry (a - mu) msig / sqrt(N) there, 0 at
    missing genotypes and at individuals without a phenotype"""
    a = np.asarray(a)
    M, N = a.shape
    present = np.asarray(present, dtype=bool)
    have = (a >= 0) & present[None, :]
    cnt = have.sum(axis=1)
    mu = np.where(cnt > 0, np.where(have, a, 0).sum(axis=1) / np.maximum(cnt, 1), 0.0)
    d = np.where(have, a - mu[:, None], 0.0)
    ss = (d * d).sum(axis=1)
    nonas = int(present.sum())
    sg = np.where(ss != 0, 1.0 / np.sqrt(np.where(ss != 0, ss, 1.0) / (nonas - 1.0)), 1.0)
    return (d * sg[:, None]).T / np.sqrt(float(N))


def dense_G(cs):
    """(A, G) of a case, G = (N / M) A A^T"""
    key = ("G", cs["name"])
    if key not in _CACHE:
        A = dense_A(cs["a"], cs["present"])
        _CACHE[key] = (A, (cs["N"] / cs["M"]) * (A @ A.T))
    return _CACHE[key]


def eigh(cs):
    """(lam descending, E columns) of G"""
    key = ("eigh", cs["name"])
    if key not in _CACHE:
        lam, E = np.linalg.eigh(dense_G(cs)[1])
        _CACHE[key] = (lam[::-1].copy(), E[:, ::-1].copy())
    return _CACHE[key]


class RankDeficient(Exception):
    pass


def chol_qr(Y):
    """one CholeskyQR step: S = Y^T Y = R^T R, Y R^-1; a pivot not above PIVOT_EPS times its diagonal entry raises"""
    S = Y.T @ Y
    S = 0.5 * (S + S.T)
    d0 = np.diag(S).copy()
    L = S.shape[0]
    R = np.zeros_like(S)
    W = S.copy()
    for j in range(L):
        d = W[j, j]
        if not (d > PIVOT_EPS * d0[j] and d > 0 and np.isfinite(d)):
            raise RankDeficient(j)
        R[j, j:] = W[j, j:] / np.sqrt(d)
        W[j + 1:, j + 1:] -= np.outer(R[j, j + 1:], R[j, j + 1:])
    return np.linalg.solve(R.T, Y.T).T


def orth(Y):
    return chol_qr(chol_qr(Y))


def sign_rule(U):
    """every column's entry of largest magnitude made positive (the lowest index on ties)"""
    U = np.array(U, dtype=np.float64)
    for j in range(U.shape[1]):
        i = int(np.argmax(np.abs(U[:, j])))
        if U[i, j] < 0:
            U[:, j] = -U[:, j]
    return U


def iterate(cs, tol, max_iter, q0=None, k=None):
    """the iteration of the section on the dense A of a case: dict theta (k), U (N x k, sign rule applied), resid (k), iterations,
    converged"""
    A, _ = dense_G(cs)
    N, M = cs["N"], cs["M"]
    k = cs["k"] if k is None else k
    Q0 = np.asarray(cs["q0"] if q0 is None else q0, dtype=np.float64).T
    Q = orth(Q0 * cs["present"][:, None])
    it = 0
    while True:
        it += 1
        Y = (N / M) * (A @ (A.T @ Q))
        T = Q.T @ Y
        th, V = np.linalg.eigh(0.5 * (T + T.T))
        th, V = th[::-1], V[:, ::-1]
        U = Q @ V
        R = Y @ V - U * th[None, :]
        r = np.sqrt((R * R).sum(axis=0))
        conv = bool(np.all(r[:k] <= tol * th[:k]))
        if conv or it >= max_iter:
            break
        Q = orth(Y)
    return dict(theta=th[:k].copy(), U=sign_rule(U[:, :k]), resid=r[:k].copy(), iterations=it, converged=conv)


def gaps(theta, lam):
    """delta_i = min over j != i of |theta_i - lam_j|"""
    out = np.empty(len(theta))
    for i, t in enumerate(theta):
        d = np.abs(t - lam)
        d[i] = np.inf
        out[i] = d.min()
    return out


def check_pairs(cs, theta, U, resid, tol, converged=True):
    """properties 1 to 3 of the section's tests for Ritz pairs (theta (k), U (N x k), resid (k)) against the dense G and its eigh;
    returns the figures it checked.  converged=False keeps only what holds for any iterate: the reported residual agrees with the
    outside norm, and the structure of the outputs"""
    _, G = dense_G(cs)
    lam, E = eigh(cs)
    N, k = cs["N"], len(theta)
    theta, U, resid = np.asarray(theta), np.asarray(U), np.asarray(resid)
    fig = dict(theta=theta, resid=resid)
    # 1. the residual promise, outside the library
    out = np.sqrt((((G @ U) - U * theta[None, :]) ** 2).sum(axis=0))
    fig["outside"] = out
    if converged:
        assert np.all(out <= 1.01 * tol * theta), (out, tol * theta)
    # 1 % agreement.  `out` is itself an N-term fp64 sum against lam_1-sized entries, rounded to N eps lam_1 at worst: where the
    # residual is at that level (out <= 100 N eps lam_1: the block spans the whole range of G, as on the 5 x 3 shape) both numbers are
    # rounding noise, 1 % of them cannot hold, and they are held to that rounding instead.  Everywhere else: the bare 1 %
    noise = out <= 100 * N * EPS * lam[0]
    assert np.all(np.abs(resid - out) <= np.where(noise, N * EPS * lam[0], 0.01 * out)), (resid, out)
    # 3. structure
    fig["orth"] = float(np.max(np.abs(U.T @ U - np.eye(k))))
    assert fig["orth"] <= N * EPS, fig["orth"]
    assert np.all(U[~cs["present"], :] == 0)
    assert np.all(np.diff(theta) <= 0)
    assert np.array_equal(sign_rule(U), U)
    if not converged:
        return fig
    # 2. against the exact eigenpairs: Davis-Kahan and Kato-Temple
    delta = gaps(theta, lam)
    sines = np.empty(k)
    for i in range(k):
        e = E[:, i]
        sines[i] = np.linalg.norm(U[:, i] - e * (e @ U[:, i]))
    fig["sin"], fig["delta"] = sines, delta
    assert np.all(sines <= resid / delta + N * EPS), (sines, resid / delta)
    assert np.all(np.abs(theta - lam[:k]) <= resid ** 2 / delta + N * EPS * lam[0]), (theta - lam[:k], resid ** 2 / delta)
    return fig
