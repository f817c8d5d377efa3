"""Device truncated SVD of the recommender's interaction matrix (``compute_svd_embeddings``,
reference ``distill_recsys.py:124-155``): a deterministic fp64 block subspace iteration with
Rayleigh-Ritz on libgdd (``csrc/gdd_svd.hip``), so the embeddings are a pure function of
``(R, dim, seed)``.

With ``A`` the matrix oriented so that its column side is the smaller one, a block ``V`` of
``b = min(k + oversample, min(m, n))`` columns is iterated as ``W = A V``, ``Z = Aᵀ W``,
``V = CholeskyQR2(Z)``. ``check_every - 1`` such steps are enqueued back to back
(``gdd_svd_segment``); the next step is a check: ``G = WᵀW`` goes to the host, ``numpy.linalg.eigh``
rotates ``V`` and ``W`` to the Ritz vectors, and the residuals ``||Aᵀ A v_j - λ_j v_j||`` of the first
``k`` decide. A Cholesky breakdown (rank-deficient block) is read from the device flag at the check;
the segment since the last check is then redone with host Householder QR, which the rest of the run
keeps using. DESIGN.md "Device truncated SVD" has the details. There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib

MAX_BLOCK = 128  # gdd_svd_max_block(): a b x b fp64 matrix has to fit one workgroup's LDS


class DeviceCSR:
    """An m x n CSR matrix on the device: int32 ``rowptr`` / ``col``, fp32 ``val`` (or None: ones)."""

    def __init__(self, rowptr, col, val, n_rows, n_cols):
        self.rowptr, self.col, self.val = rowptr, col, val
        self.n_rows, self.n_cols = int(n_rows), int(n_cols)
        self.nnz = int(col.numel())

    @classmethod
    def from_scipy(cls, R, device="cuda", values=True):
        R = sp.csr_matrix(R, copy=True)
        R.sum_duplicates()
        dev = torch.device(device)
        rowptr = torch.from_numpy(R.indptr.astype(np.int32)).to(dev)
        col = torch.from_numpy(R.indices.astype(np.int32)).to(dev)
        val = torch.from_numpy(R.data.astype(np.float32)).to(dev) if values else None
        return cls(rowptr, col, val, R.shape[0], R.shape[1])

    @property
    def device(self):
        return self.rowptr.device

    def transpose(self) -> "DeviceCSR":
        lib = _lib.device_lib()
        dev = self.device
        rowptr = torch.empty(self.n_cols + 1, dtype=torch.int32, device=dev)
        col = torch.empty(max(self.nnz, 1), dtype=torch.int32, device=dev)
        val = None if self.val is None else torch.empty(max(self.nnz, 1), dtype=torch.float32, device=dev)
        ws = _lib.workspace(lib.gdd_csr_transpose_ws_bytes(self.n_rows, self.n_cols, self.nnz), dev)
        _lib.check(lib.gdd_csr_transpose(self.n_rows, self.n_cols, self.nnz, self.rowptr.data_ptr(),
                                         _lib.ptr(self.col), _lib.ptr(self.val), rowptr.data_ptr(),
                                         col.data_ptr(), _lib.ptr(val), None, ws.data_ptr(), ws.numel(),
                                         _lib.stream_ptr(dev)))
        return DeviceCSR(rowptr, col[:self.nnz], None if val is None else val[:self.nnz], self.n_cols,
                         self.n_rows)


def _f64(t: torch.Tensor) -> torch.Tensor:
    if t.dtype != torch.float64 or t.dim() != 2 or not t.is_cuda:
        raise ValueError(f"expected a 2-d float64 device tensor, got {t.dtype} {tuple(t.shape)} on {t.device}")
    return t.contiguous()


def _check_block(b: int):
    if not 1 <= b <= MAX_BLOCK:
        raise ValueError(f"device SVD supports blocks of 1 .. {MAX_BLOCK} columns, got {b}: "
                         "use the host backend (svd_backend='host')")


def spmm_f64(A: DeviceCSR, X: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """``A @ X`` in fp64, every element a multiply-then-add chain in CSR entry order."""
    X = _f64(X)
    if X.shape[0] != A.n_cols:
        raise ValueError(f"spmm_f64: X must have {A.n_cols} rows, got {X.shape[0]}")
    b = X.shape[1]
    _check_block(b)
    Y = torch.empty((A.n_rows, b), dtype=torch.float64, device=X.device) if out is None else out
    _lib.check(_lib.device_lib().gdd_spmm_f64(A.n_rows, A.n_cols, A.rowptr.data_ptr(), A.col.data_ptr(),
                                              _lib.ptr(A.val), b, X.data_ptr(), Y.data_ptr(),
                                              _lib.stream_ptr(X.device)))
    return Y


def gram_f64(W: torch.Tensor, form: int = -1) -> torch.Tensor:
    """``Wᵀ W`` (symmetric bit for bit). ``form``: 0 fp64 MFMA, 1 plain fma, -1 the default."""
    W = _f64(W)
    n, b = W.shape
    _check_block(b)
    lib = _lib.device_lib()
    G = torch.empty((b, b), dtype=torch.float64, device=W.device)
    ws = _lib.workspace(lib.gdd_gram_f64_ws_bytes(n, b), W.device)
    _lib.check(lib.gdd_gram_f64(n, b, W.data_ptr(), G.data_ptr(), form, ws.data_ptr(), ws.numel(),
                                _lib.stream_ptr(W.device)))
    return G


def tsmm_f64(W: torch.Tensor, Q: torch.Tensor) -> torch.Tensor:
    """``W @ Q`` for a b x b ``Q``."""
    W, Q = _f64(W), _f64(Q)
    n, b = W.shape
    _check_block(b)
    if tuple(Q.shape) != (b, b):
        raise ValueError(f"tsmm_f64: Q must be {b} x {b}, got {tuple(Q.shape)}")
    out = torch.empty_like(W)
    _lib.check(_lib.device_lib().gdd_tsmm_f64(n, b, W.data_ptr(), Q.data_ptr(), out.data_ptr(),
                                              _lib.stream_ptr(W.device)))
    return out


def chol_inv_f64(G: torch.Tensor):
    """``(R⁻¹, flag)`` for ``G = Rᵀ R``; ``flag`` (device int32) is 1 after a breakdown."""
    G = _f64(G)
    b = G.shape[0]
    _check_block(b)
    Rinv = torch.empty_like(G)
    flag = torch.zeros(1, dtype=torch.int32, device=G.device)
    _lib.check(_lib.device_lib().gdd_chol_inv_f64(b, G.data_ptr(), Rinv.data_ptr(), flag.data_ptr(),
                                                  _lib.stream_ptr(G.device)))
    return Rinv, flag


def cholqr2_f64(Z: torch.Tensor, flag: torch.Tensor | None = None):
    """``(V, flag)``: an orthonormal basis of ``Z``'s columns by CholeskyQR2."""
    Z = _f64(Z)
    n, b = Z.shape
    _check_block(b)
    lib = _lib.device_lib()
    V = torch.empty_like(Z)
    if flag is None:
        flag = torch.zeros(1, dtype=torch.int32, device=Z.device)
    ws = _lib.workspace(lib.gdd_cholqr2_ws_bytes(n, b), Z.device)
    _lib.check(lib.gdd_cholqr2_f64(n, b, Z.data_ptr(), V.data_ptr(), flag.data_ptr(), ws.data_ptr(),
                                   ws.numel(), _lib.stream_ptr(Z.device)))
    return V, flag


def block_size(shape, k: int, oversample: int = 64) -> int:
    return int(min(k + oversample, min(shape)))


class _Iteration:
    """The device state of one run: A, Aᵀ, the blocks and the workspaces, allocated once."""

    def __init__(self, R, b, k, device):
        self.lib = _lib.device_lib()
        dev = torch.device(device)
        Rd = DeviceCSR.from_scipy(R, dev)
        Rt = Rd.transpose()
        m, n = Rd.n_rows, Rd.n_cols
        self.swapped = n > m  # the block lives on the smaller side
        self.A, self.At = (Rt, Rd) if self.swapped else (Rd, Rt)
        self.nb, self.ns, self.b, self.k, self.dev = self.A.n_rows, self.A.n_cols, b, k, dev
        f64 = dict(dtype=torch.float64, device=dev)
        self.V = torch.empty((self.ns, b), **f64)
        self.Z = torch.empty((self.ns, b), **f64)
        self.W = torch.empty((self.nb, b), **f64)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ws = _lib.workspace(self.lib.gdd_svd_segment_ws_bytes(self.nb, self.ns, b), dev)
        self.rws = _lib.workspace(self.lib.gdd_svd_residuals_ws_bytes(self.ns, k), dev)
        self.r = torch.empty(k, **f64)

    def stream(self):
        return _lib.stream_ptr(self.dev)

    def qr(self, Z, host):
        """self.V = orthonormal basis of Z (device CholeskyQR2, or host Householder QR)."""
        if host:
            q, _ = np.linalg.qr(Z.cpu().numpy())
            self.V.copy_(torch.from_numpy(np.ascontiguousarray(q)))
        else:
            _lib.check(self.lib.gdd_cholqr2_f64(self.ns, self.b, Z.data_ptr(), self.V.data_ptr(),
                                                self.flag.data_ptr(), self.ws.data_ptr(),
                                                self.ws.numel(), self.stream()))

    def products(self):
        spmm_f64(self.A, self.V, out=self.W)
        spmm_f64(self.At, self.W, out=self.Z)

    def segment(self, steps, host):
        if steps <= 0:
            return
        if host:
            for _ in range(steps):
                self.products()
                self.qr(self.Z, True)
            return
        A, At = self.A, self.At
        _lib.check(self.lib.gdd_svd_segment(self.nb, self.ns, A.rowptr.data_ptr(), A.col.data_ptr(),
                                            _lib.ptr(A.val), At.rowptr.data_ptr(), At.col.data_ptr(),
                                            _lib.ptr(At.val), self.b, steps, self.V.data_ptr(),
                                            self.W.data_ptr(), self.Z.data_ptr(), self.flag.data_ptr(),
                                            self.ws.data_ptr(), self.ws.numel(), self.stream()))


def _iterate(R, k, oversample, tol, check_every, max_iter, seed, device):
    m, n = R.shape
    if not 0 < k < min(m, n):
        raise ValueError(f"truncated_svd: k must be in 1 .. min(shape) - 1, got k={k} for shape={R.shape}")
    if check_every < 1:
        raise ValueError("truncated_svd: check_every must be at least 1")
    b = block_size((m, n), k, oversample)
    _check_block(b)
    it = _Iteration(R, b, k, device)
    start = np.random.RandomState(seed).standard_normal((it.ns, b))
    Zc = torch.from_numpy(start).to(it.dev)
    host_qr = False
    it.qr(Zc, False)
    steps = redone = 0
    while True:
        seg = max(0, min(check_every - 1, max_iter - steps - 1))
        it.segment(seg, host_qr)
        steps += seg + 1
        spmm_f64(it.A, it.V, out=it.W)
        G = gram_f64(it.W)
        G_h = G.cpu().numpy()  # the check's one synchronisation before the rotation
        if not host_qr and int(it.flag.item()) != 0:
            # a Cholesky breakdown since the last check: redo that segment with Householder QR
            host_qr = True
            redone += 1
            it.qr(Zc, True)
            it.segment(seg, True)
            spmm_f64(it.A, it.V, out=it.W)
            G_h = gram_f64(it.W).cpu().numpy()
        lam, Q = np.linalg.eigh(G_h)
        lam, Q = lam[::-1].copy(), np.ascontiguousarray(Q[:, ::-1])
        Qd = torch.from_numpy(Q).to(it.dev)
        lam_d = torch.from_numpy(lam).to(it.dev)
        it.V = tsmm_f64(it.V, Qd)
        it.W = tsmm_f64(it.W, Qd)
        spmm_f64(it.At, it.W, out=it.Z)
        _lib.check(it.lib.gdd_svd_residuals(it.ns, b, k, it.Z.data_ptr(), it.V.data_ptr(), lam_d.data_ptr(),
                                            it.r.data_ptr(), it.rws.data_ptr(), it.rws.numel(),
                                            it.stream()))
        resid = float(it.r.max().item())
        if resid <= tol * lam[0]:
            break
        if steps >= max_iter:
            raise RuntimeError(f"truncated_svd: no convergence in {steps} steps "
                               f"(residual {resid:.3e}, target {tol * lam[0]:.3e})")
        Zc = it.Z.clone()
        it.qr(it.Z, host_qr)
    info = {"steps": steps, "residual": resid, "lambda_max": float(lam[0]), "block": b,
            "host_qr_redone": redone, "swapped": it.swapped}
    return it, lam_d, info


def _finalize(it, lam_d, want_f64, want_f32):
    k, dev = it.k, it.dev
    S = torch.empty(k, dtype=torch.float64, device=dev)
    sign = torch.empty(k, dtype=torch.float64, device=dev)
    Vo = torch.empty((it.ns, k), dtype=torch.float64, device=dev) if want_f64 else None
    Uo = torch.empty((it.nb, k), dtype=torch.float64, device=dev) if want_f64 else None
    es = torch.empty((it.ns, k), dtype=torch.float32, device=dev) if want_f32 else None
    eb = torch.empty((it.nb, k), dtype=torch.float32, device=dev) if want_f32 else None
    _lib.check(it.lib.gdd_svd_finalize(it.ns, it.nb, it.b, k, it.V.data_ptr(), it.W.data_ptr(),
                                       lam_d.data_ptr(), S.data_ptr(), _lib.ptr(Vo), _lib.ptr(Uo),
                                       _lib.ptr(es), _lib.ptr(eb), sign.data_ptr(), it.stream()))
    return S, Vo, Uo, es, eb


def truncated_svd(R, k, *, oversample=64, tol=1e-10, check_every=8, max_iter=800, seed=42, device="cuda"):
    """The ``k`` largest singular triplets of the sparse ``R`` (m x n), σ descending: ``(U, S, V, info)``
    as fp64 numpy arrays (``U`` m x k, ``V`` n x k, ``R ≈ U diag(S) Vᵀ``); ``info`` has the step count
    (``steps``) and the final residual ``max_j ||AᵀA v_j - σ_j² v_j||`` (``residual``).

    Deterministic: the start block is ``RandomState(seed).standard_normal`` and no sum depends on
    scheduling. Blocks above 128 columns (``k + oversample``, clamped to ``min(m, n)``) raise
    ``ValueError``; the host backend has no such limit."""
    it, lam_d, info = _iterate(R, int(k), int(oversample), float(tol), int(check_every), int(max_iter),
                               seed, device)
    S, Vo, Uo, _, _ = _finalize(it, lam_d, True, False)
    small, big = Vo.cpu().numpy(), Uo.cpu().numpy()
    U, V = (small, big) if it.swapped else (big, small)
    return U, S.cpu().numpy(), V, info


def svd_embeddings(R, dim, seed=42, device="cuda"):
    """``compute_svd_embeddings`` (distill_recsys.py:124-155) on the device: the fp32 numpy pair
    ``(U sqrt(S), V sqrt(S))`` with ``k = min(dim, min(R.shape) - 1)``."""
    k = min(int(dim), min(R.shape) - 1)
    if k <= 0:
        raise ValueError(f"Cannot compute SVD with shape={R.shape} and dim={dim}")
    it, lam_d, _ = _iterate(R, k, 64, 1e-10, 8, 800, seed, device)
    _, _, _, es, eb = _finalize(it, lam_d, False, True)
    small, big = es.cpu().numpy(), eb.cpu().numpy()
    return (small, big) if it.swapped else (big, small)
