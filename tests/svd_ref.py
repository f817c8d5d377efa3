"""numpy restatement of the device truncated SVD (gdd/svd.py, csrc/gdd_svd.hip): the same block
subspace iteration with Rayleigh-Ritz, CholeskyQR2 with the same breakdown rule, the same check
schedule, sign convention and scaling. The CPU tests hold it against np.linalg.svd; the GPU tests
hold the kernels against its pieces (spmm_ordered bit for bit)."""
import numpy as np
import scipy.sparse as sp


def interactions(m, n, nnz, seed):
    """m x n CSR of nnz random interactions, duplicates summed (fp32 counts)."""
    rs = np.random.RandomState(seed)
    u, i = rs.randint(0, m, nnz), rs.randint(0, n, nnz)
    R = sp.coo_matrix((np.ones(nnz, np.float32), (u, i)), shape=(m, n)).tocsr()
    R.sum_duplicates()
    return R


def low_rank_rows(m, n, distinct, per_row, seed):
    """m x n CSR whose rows repeat `distinct` random patterns: rank <= distinct."""
    rs = np.random.RandomState(seed)
    base = np.zeros((distinct, n), np.float32)
    for r in range(distinct):
        base[r, rs.choice(n, per_row, replace=False)] = rs.randint(1, 4, per_row)
    return sp.csr_matrix(base[rs.randint(0, distinct, m)])


def spmm_ordered(indptr, indices, data, X):
    """Y = A X with every element a multiply-then-add chain from +0 in CSR entry order."""
    n = len(indptr) - 1
    Y = np.zeros((n, X.shape[1]), np.float64)
    lens = np.diff(indptr)
    for p in range(int(lens.max(initial=0))):
        rows = np.nonzero(lens > p)[0]
        e = indptr[rows] + p
        a = np.ones(len(e)) if data is None else data[e].astype(np.float64)
        Y[rows] = Y[rows] + a[:, None] * X[indices[e]]
    return Y


def chol_inv(G):
    """(R⁻¹, breakdown) for G = Rᵀ R: right-looking Cholesky; a pivot at or below
    b 2^-52 max diag (or NaN) is a breakdown and gives the identity."""
    b = G.shape[0]
    A = np.array(G, np.float64)
    thresh = b * 2.0 ** -52 * np.max(np.diag(A))
    for j in range(b):
        p = A[j, j]
        if not p > thresh:
            return np.eye(b), True
        d = np.sqrt(p)
        A[j + 1:, j] = A[j + 1:, j] / d
        A[j, j] = d
        A[j + 1:, j + 1:] -= np.outer(A[j + 1:, j], A[j + 1:, j])
    L = np.tril(A)
    return np.linalg.solve(L, np.eye(b)).T, False


def cholqr2(Z):
    """(V, breakdown): two passes of gram, chol_inv, Z R⁻¹; a breakdown leaves its pass unchanged."""
    bad = False
    for _ in range(2):
        Rinv, b_ = chol_inv(Z.T @ Z)
        bad |= b_
        Z = Z @ Rinv
    return Z, bad


def block_size(shape, k, oversample=64):
    return int(min(k + oversample, min(shape)))


def truncated_svd(R, k, oversample=64, tol=1e-10, check_every=8, max_iter=800, seed=42):
    """(U, S, V, info) like gdd.svd.truncated_svd."""
    R = sp.csr_matrix(R).astype(np.float64)
    m, n = R.shape
    assert 0 < k < min(m, n)
    swapped = n > m
    A = R.T.tocsr() if swapped else R
    At = A.T.tocsr()
    ns = A.shape[1]
    b = block_size((m, n), k, oversample)
    Zc = np.random.RandomState(seed).standard_normal((ns, b))
    host_qr = False
    redone = steps = 0

    def qr(Z, host):
        if host:
            return np.linalg.qr(Z)[0], False
        return cholqr2(Z)

    def segment(V, s, host):
        bad = False
        for _ in range(s):
            V, b_ = qr(At @ (A @ V), host)
            bad |= b_
        return V, bad

    V, flag = qr(Zc, False)
    while True:
        seg = max(0, min(check_every - 1, max_iter - steps - 1))
        V, b_ = segment(V, seg, host_qr)
        flag |= b_
        steps += seg + 1
        if flag and not host_qr:
            host_qr, redone = True, redone + 1
            V, _ = qr(Zc, True)
            V, _ = segment(V, seg, True)
        W = A @ V
        lam, Q = np.linalg.eigh(W.T @ W)
        lam, Q = lam[::-1], Q[:, ::-1]
        V, W = V @ Q, W @ Q
        Z = At @ W
        resid = float(np.max(np.linalg.norm(Z[:, :k] - lam[:k] * V[:, :k], axis=0)))
        if resid <= tol * lam[0]:
            break
        if steps >= max_iter:
            raise RuntimeError(f"no convergence in {steps} steps")
        Zc = Z
        V, b_ = qr(Z, host_qr)
        flag |= b_
    S = np.sqrt(np.maximum(lam[:k], 0.0))
    small = V[:, :k].copy()
    with np.errstate(divide="ignore", invalid="ignore"):
        big = np.where(S > 0, W[:, :k] / S, 0.0)
    top = np.argmax(np.abs(small), axis=0)  # the first of equal magnitudes
    sign = np.where(small[top, np.arange(k)] < 0, -1.0, 1.0)
    small, big = small * sign, big * sign
    U, Vn = (small, big) if swapped else (big, small)
    return U, S, Vn, {"steps": steps, "residual": resid, "block": b, "host_qr_redone": redone}


def svd_embeddings(R, dim, seed=42):
    k = min(dim, min(R.shape) - 1)
    U, S, V, _ = truncated_svd(R, k, seed=seed)
    root = np.sqrt(np.maximum(S, 1e-12))
    return (U * root).astype(np.float32), (V * root).astype(np.float32)


def check_factors(R, k, U, S, V, tol=1e-10):
    """The issue's bounds against np.linalg.svd of the dense matrix: |σ̂² - σ²| <= 2 tol σ_1²,
    small-side orthonormality <= 1e-12, and the recomputed residual ||RᵀR v - σ² v|| <= 2 tol σ_1²
    (on the small side's operator). Returns the three figures."""
    D = np.asarray(sp.csr_matrix(R).todense(), np.float64)
    s = np.linalg.svd(D, compute_uv=False)
    small, op = (U, D @ D.T) if D.shape[1] > D.shape[0] else (V, D.T @ D)
    sig_err = float(np.max(np.abs(S ** 2 - s[:k] ** 2)))
    orth = float(np.max(np.abs(small.T @ small - np.eye(k))))
    res = float(np.max(np.linalg.norm(op @ small - small * S ** 2, axis=0)))
    bound = 2 * tol * s[0] ** 2
    return {"sigma2_err": sig_err, "orth": orth, "residual": res, "bound": bound}
