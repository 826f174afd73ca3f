"""Dense numpy restatement of the LD-block preconditioner, written from its definitions: the PLINK decode,
the standardised matrix A that Ax / ATx apply, the window Grams (dense and by the integer-plane formula), the two-grid apply and
the reference's preconditioned CG with its two stop rules.  Test infrastructure only."""
import numpy as np

# PLINK 2-bit code -> genotype a (0 at missing) and "present" b: 00 -> 2, 10 -> 1, 11 -> 0, 01 -> missing
_A = np.array([2.0, 0.0, 1.0, 0.0])
_B = np.array([1.0, 0.0, 1.0, 1.0])


def decode(bed, N, M):
    """(a, b): N x M genotype values and presence, from M * ceil(N/4) marker-major bytes"""
    mb = (N + 3) // 4
    raw = np.frombuffer(bytes(bed), dtype=np.uint8)[:M * mb].reshape(M, mb)
    codes = np.stack([(raw >> (2 * q)) & 3 for q in range(4)], axis=2).reshape(M, 4 * mb)[:, :N].T
    return _A[codes], _B[codes]


def marker_stats(a, b, na):
    """mave, msig of compute_markers_statistics over the individuals with a phenotype (na)"""
    P = b * na[:, None]
    nonas = float(na.sum())
    sb = P.sum(0)
    mave = np.where(sb != 0, (a * P).sum(0) / np.where(sb != 0, sb, 1), 0.0)
    ss = (((a - mave) * P) ** 2).sum(0)
    msig = np.where(ss != 0, 1.0 / np.sqrt(np.where(ss != 0, ss, 1) / (nonas - 1.0)), 1.0)
    return mave, msig


def matrix(a, b, na, mave, msig):
    """A_ni = (a_ni - mave_i) msig_i b_ni na_n / sqrt(N)"""
    N = a.shape[0]
    return (a - mave) * msig * b * na[:, None] / np.sqrt(N)


def windows(S, M, W):
    """the windows of both grids that overlap the shard [S, S+M): (grid, k, lo, hi) with global, clipped [lo, hi)"""
    h = W // 2
    out = []
    for u in range(S // h, (S + M - 1) // h + 2 if M > 0 else S // h):
        lo, hi = max((u - 1) * h, S, 0), min((u + 1) * h, S + M)
        out.append((0, (u - 1) // 2, lo, hi) if u % 2 else (1, u // 2, lo, hi))
    return out


def gram_dense(A, S, lo, hi):
    Aw = A[:, lo - S:hi - S]
    return Aw.T @ Aw


def gram_planes(a, b, na, mave, msig, S, lo, hi):
    """G_ij = msig_i msig_j / N (VV_ij - mave_j VP_ij - mave_i VP_ji + mave_i mave_j PP_ij), integer VV, VP, PP"""
    N = a.shape[0]
    sl = slice(lo - S, hi - S)
    P = (b[:, sl] * na[:, None]).astype(np.int64)
    V = a[:, sl].astype(np.int64) * P
    VV, VP, PP = V.T @ V, V.T @ P, P.T @ P
    m, s = mave[sl], msig[sl]
    inner = VV - m[None, :] * VP - m[:, None] * VP.T + np.outer(m, m) * PP
    return np.outer(s, s) / N * inner


class TwoGrid:
    """z = 1/2 sum over both grids of blockdiag((tau G + gam2 I)^-1) r; a window whose Cholesky pivot is <= 1e-12 x its largest
    diagonal (or not finite) takes the scalar rule r / diag on its markers"""

    def __init__(self, A, S, W, tau, gam2):
        N, M = A.shape
        self.S, self.M = S, M
        self.diag = tau * (N - 1) / N + gam2
        self.blocks, self.fallback = [], 0
        for grid, k, lo, hi in windows(S, M, W):
            B = tau * gram_dense(A, S, lo, hi) + gam2 * np.eye(hi - lo)
            inv = self._inverse(B)
            if inv is None:
                self.fallback += 1
                inv = np.eye(hi - lo) / self.diag
            self.blocks.append((lo - S, hi - S, inv))

    @staticmethod
    def _inverse(B):
        dmax = max(float(np.max(np.diag(B))), 0.0)
        n = B.shape[0]
        L = np.zeros_like(B)
        for j in range(n):                           # the pivots are those of a Cholesky factorisation
            piv = B[j, j] - L[j, :j] @ L[j, :j]
            if not (piv > 1e-12 * dmax) or not np.isfinite(piv):
                return None
            L[j, j] = np.sqrt(piv)
            L[j + 1:, j] = (B[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
        Li = np.linalg.inv(L)
        return Li.T @ Li

    def __call__(self, r):
        z = np.zeros_like(r)
        for lo, hi, inv in self.blocks:
            z[lo:hi] += inv @ r[lo:hi]
        return 0.5 * z


def pcg(A, v, tau, gam2, denoiser, max_iter, precond=None):
    """vamp::precondCG_solver from a zero start: ||r|| / ||v|| < 1e-5 (denoiser 1) or the Onsager rule, relative change of
    gam2 <v, mu> below 1e-8 (denoiser 0).  precond None = the scalar diag.  Returns (mu, steps, converged)."""
    N = A.shape[0]
    diag = tau * (N - 1) / N + gam2
    apply_m = precond if precond is not None else (lambda r: r / diag)
    Q = lambda x: tau * (A.T @ (A @ x)) + gam2 * x
    mu = np.zeros_like(v)
    r = v.copy()
    z = apply_m(r)
    p = z.copy()
    rz = r @ z
    nv = np.linalg.norm(v)
    prev = 0.0
    for it in range(1, max_iter + 1):
        d = Q(p)
        alpha = rz / (d @ p)
        mu = mu + alpha * p
        if denoiser == 0:
            ons = gam2 * (v @ mu)
            if (abs((ons - prev) / ons) if ons != 0 else 1.0) < 1e-8:
                return mu, it, True
            prev = ons
        r = r - alpha * d
        z = apply_m(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
        if np.linalg.norm(r) / nv < 1e-5:
            return mu, it, True
    return mu, max_iter, False
