"""The Rankformer teacher on MI355X (Rankformer/code/rec.py, model.py, main.py): the layer as two
fused row passes, the trainer, and the export that ``gdd.distill_recsys --teacher_path`` loads.

The layer (rec.py:143-274) is linear-time attention over the bipartite interaction graph. With
``x̂`` the L2-normalised rows of ``x`` (users first), ``v = x``, ``N_u`` / ``N_i`` the neighbours,
``d⁺_u = max(|N_u|, 1)``, ``d⁻_u = max(m − |N_u|, 1)``, ``s_ui = ⟨x̂_u, x̂_i⟩``,
``b⁺_u = Σ_{N_u} s_ui / d⁺_u``, ``b⁻_u = Σ_{∉N_u} s_uj / d⁻_u``,
``Ω⁺_ui = (s_ui − b⁻_u + α)/d⁺_u`` and ``Ω⁻_uj = (s_uj − b⁺_u − α)/d⁻_u``::

    z_u = (Σ_{N_u} Ω⁺_ui v_i + Σ_{∉N_u} Ω⁻_uj v_j) / (2 max(b⁺_u − b⁻_u + α, c))
    z_i = (Σ_{N_i} Ω⁺_ui v_u + Σ_{∉N_i} Ω⁻_ui v_u) / (max(Σ_{N_i} Ω⁺_ui, c) + max(−Σ_{∉N_i} Ω⁻_ui, c))

Every sum over non-neighbours is a global term minus a sum over neighbours, so the layer needs one
dot product and one scalar weight per interaction plus a few d × d products (DESIGN.md "Rankformer
teacher"). The per-interaction work is two HIP passes, ``gdd_rank_rowpass`` and ``gdd_rank_wsum``
(csrc/gdd_rankformer.hip), wrapped as autograd functions whose backwards are the same passes over the
transposed CSR plus ``gdd_edge_dots``. No ``index_add_`` on float tensors and no float atomics
anywhere in the forward or backward: two runs on the same input give the same bits. Nothing larger
than ``(n+m) × d`` or the number of interactions is allocated (the reference materialises two
``rows × d × d`` tensors).

* :class:`InteractionGraph` — the distinct training pairs as a canonical CSR and its transpose on
  the device (duplicate pairs raise ``ValueError``: the reference would count them twice);
* :class:`RankformerLayer`, :class:`GCNLayer` (rec.py:92-140);
* :class:`RankformerTeacher` — model.py:123-250 and the BPR loss of :402-468, with a device negative
  sampler that redraws until no ``(u, j)`` is a training pair, the contrastive branch (``use_cl``,
  ``cl_layer``, ``cl_lambda``, ``cl_eps``, ``cl_tau``) and the layer's three ablation switches
  (``del_neg``, ``del_benchmark``, ``del_omega_norm``);
* :func:`infonce`, :func:`infonce_rows` — model.py:10-24 as two streaming HIP passes
  (csrc/gdd_infonce.hip, DESIGN.md "Contrastive loss"): the ``B × B`` logits of the reference are
  never stored, forward and backward are bit-reproducible;
* :func:`train_teacher` (main.py:141-190 with parse.py's defaults), :func:`save_teacher`
  (main.py:219-227). The command line is :mod:`gdd.train_teacher`.

Not offered: the reference's random trajectory: the device RNG stream differs from the reference's,
results are deterministic for a seed on one device. With ``use_cl`` the reference evaluates the noisy
embeddings its last training step left behind; here evaluation is noise-free. There is no CPU path.

Validation is Recall@K by :class:`gdd.recsys.RecallEvaluator` by default; ``select_by="ndcg"`` is the
reference's loop (main.py:100-120): precision, recall and NDCG at ``topks`` by
:class:`gdd.rankeval.RankingEvaluator`, the epoch kept is the one with the best validation
NDCG@max(topks), and the test split is evaluated at every new best.
"""
from __future__ import annotations

import copy
import weakref
from typing import Dict, List, Optional, Tuple

import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F
from torch import nn

from . import _lib

MAX_DIM = 256  # gdd_rank_max_dim(): one wave per chunk of entries, four features per lane


def _check_dim(d: int) -> int:
    d = int(d)
    if d < 1 or d > MAX_DIM:
        raise ValueError(f"rankformer: embedding width {d} outside [1, {MAX_DIM}]")
    return d


class _Side:
    """One orientation of the interaction matrix as a device CSR: ``rowptr``/``col`` (int32), the row
    of every stored entry (``rows`` int32, ``rows_l`` int64), the other orientation ``T`` and the
    gather ``to_T`` that reorders an entry array of this side into ``T``'s entry order."""

    def __init__(self, n_rows: int, n_cols: int, rowptr: torch.Tensor, col: torch.Tensor, bad: torch.Tensor):
        self.n_rows, self.n_cols = int(n_rows), int(n_cols)
        self.rowptr, self.col, self.bad = rowptr, col, bad
        self.nnz = int(col.shape[0])
        dev = rowptr.device
        rp = rowptr.long()
        self.rows_l = torch.repeat_interleave(torch.arange(self.n_rows, device=dev), rp[1:] - rp[:-1])
        self.rows = self.rows_l.to(torch.int32)
        self.T: "_Side" = None  # type: ignore[assignment]
        self.to_T: torch.Tensor = None  # type: ignore[assignment]

    @property
    def device(self) -> torch.device:
        return self.rowptr.device


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def rank_rowpass(side: _Side, Q: torch.Tensor, K: torch.Tensor, V: torch.Tensor):
    """``gdd_rank_rowpass``: (s [nnz], s_sum [rows], SK, SV, A [rows, d]) for the CSR ``side``."""
    lib = _lib.device_lib()
    Q, K, V = _f32(Q), _f32(K), _f32(V)
    d = _check_dim(Q.shape[1])
    if Q.shape[0] != side.n_rows or K.shape != (side.n_cols, d) or V.shape != (side.n_cols, d):
        raise ValueError("rank_rowpass: table shapes do not match the CSR")
    dev = Q.device
    s = torch.empty(side.nnz, dtype=torch.float32, device=dev)
    s_sum = torch.empty(side.n_rows, dtype=torch.float32, device=dev)
    SK, SV, A = (torch.empty(side.n_rows, d, dtype=torch.float32, device=dev) for _ in range(3))
    ws = _lib.workspace(lib.gdd_rank_ws_bytes(side.nnz, d), dev)
    _lib.check(lib.gdd_rank_rowpass(side.n_rows, side.n_cols, side.nnz, side.rowptr.data_ptr(),
                                    _lib.ptr(side.col), d, Q.data_ptr(), K.data_ptr(), V.data_ptr(),
                                    s.data_ptr(), s_sum.data_ptr(), SK.data_ptr(), SV.data_ptr(),
                                    A.data_ptr(), side.bad.data_ptr(), ws.data_ptr(), ws.numel(),
                                    _lib.stream_ptr(dev)))
    return s, s_sum, SK, SV, A


def rank_wsum(side: _Side, w: torch.Tensor, V: torch.Tensor, a: Optional[torch.Tensor] = None,
              b: Optional[torch.Tensor] = None):
    """``gdd_rank_wsum``: (Y [rows, d], ta, tb [rows] or None); ``w``, ``a``, ``b`` in ``side``'s
    entry order."""
    lib = _lib.device_lib()
    w, V = _f32(w), _f32(V)
    d = _check_dim(V.shape[1])
    if w.shape != (side.nnz,) or V.shape[0] != side.n_cols:
        raise ValueError("rank_wsum: shapes do not match the CSR")
    dev = V.device
    Y = torch.empty(side.n_rows, d, dtype=torch.float32, device=dev)
    ta = tb = None
    if a is not None:
        a = _f32(a)
        ta = torch.empty(side.n_rows, dtype=torch.float32, device=dev)
    if b is not None:
        b = _f32(b)
        tb = torch.empty(side.n_rows, dtype=torch.float32, device=dev)
    ws = _lib.workspace(lib.gdd_rank_ws_bytes(side.nnz, d), dev)
    _lib.check(lib.gdd_rank_wsum(side.n_rows, side.n_cols, side.nnz, side.rowptr.data_ptr(),
                                 _lib.ptr(side.col), d, w.data_ptr(), V.data_ptr(), _lib.ptr(a), _lib.ptr(b),
                                 Y.data_ptr(), _lib.ptr(ta), _lib.ptr(tb), side.bad.data_ptr(),
                                 ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
    return Y, ta, tb


def _edge_dots(side: _Side, R: torch.Tensor, C: torch.Tensor) -> torch.Tensor:
    """out[e] = ⟨R[row(e)], C[col(e)]⟩ (``gdd_edge_dots``)."""
    lib = _lib.device_lib()
    R, C = _f32(R), _f32(C)
    out = torch.empty(side.nnz, dtype=torch.float32, device=R.device)
    _lib.check(lib.gdd_edge_dots(side.nnz, int(R.shape[1]), _lib.ptr(side.rows), R.data_ptr(), int(R.shape[0]),
                                 _lib.ptr(side.col), C.data_ptr(), int(C.shape[0]), out.data_ptr(),
                                 side.bad.data_ptr(), _lib.stream_ptr(R.device)))
    return out


def _add(a, b):
    if a is None:
        return b
    return a if b is None else a + b


def _check_infonce(a: torch.Tensor, y: torch.Tensor, tau: float) -> Tuple[int, int, float]:
    if a.dim() != 2 or a.shape != y.shape:
        raise ValueError("infonce: a and y must be two matrices of one shape")
    if not float(tau) > 0.0:
        raise ValueError(f"infonce: tau must be positive, got {tau!r}")
    return int(a.shape[0]), _check_dim(a.shape[1]), 1.0 / float(tau)


def infonce_row_pass(a: torch.Tensor, y: torch.Tensor, tau: float, want_R: bool = True):
    """``gdd_infonce_rows``: (lse [B], diag [B], pd [B], R [B, d]; pd and R None unless ``want_R``)
    with ``ℓ_rc = ⟨a_r, y_c⟩ / tau``, ``lse_r = log Σ_c exp ℓ_rc``, ``diag_r = ℓ_rr``,
    ``pd_r = exp(ℓ_rr − lse_r)``, ``R_r = Σ_c exp(ℓ_rc − lse_r) y_c``. No ``B × B`` object is built."""
    lib = _lib.device_lib()
    a, y = _f32(a), _f32(y)
    B, d, inv_tau = _check_infonce(a, y, tau)
    dev = a.device
    lse = torch.empty(B, dtype=torch.float32, device=dev)
    diag = torch.empty(B, dtype=torch.float32, device=dev)
    pd = torch.empty(B, dtype=torch.float32, device=dev) if want_R else None
    R = torch.empty(B, d, dtype=torch.float32, device=dev) if want_R else None
    ws = _lib.workspace(lib.gdd_infonce_ws_bytes(B, d), dev)
    _lib.check(lib.gdd_infonce_rows(B, d, a.data_ptr(), y.data_ptr(), inv_tau, lse.data_ptr(), diag.data_ptr(),
                                    _lib.ptr(pd), _lib.ptr(R), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
    return lse, diag, pd, R


def infonce_col_pass(a: torch.Tensor, y: torch.Tensor, tau: float, lse: torch.Tensor, pd: torch.Tensor,
                     G: torch.Tensor):
    """``gdd_infonce_cols``: ``C_c = Σ_r G_r exp(ℓ_rc − lse_r) a_r`` [B, d], ``lse`` and ``pd`` from
    :func:`infonce_row_pass`."""
    lib = _lib.device_lib()
    a, y, lse, pd, G = _f32(a), _f32(y), _f32(lse), _f32(pd), _f32(G)
    B, d, inv_tau = _check_infonce(a, y, tau)
    if lse.shape != (B,) or pd.shape != (B,) or G.shape != (B,):
        raise ValueError("infonce_col_pass: lse, pd and G must have one entry per row")
    dev = a.device
    C = torch.empty(B, d, dtype=torch.float32, device=dev)
    ws = _lib.workspace(lib.gdd_infonce_ws_bytes(B, d), dev)
    _lib.check(lib.gdd_infonce_cols(B, d, a.data_ptr(), y.data_ptr(), inv_tau, lse.data_ptr(), pd.data_ptr(),
                                    G.data_ptr(), C.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
    return C


class _InfoNCERows(torch.autograd.Function):
    """loss_r = lse_r − ℓ_rr. Backward, with P_rc = exp(ℓ_rc − lse_r) and R_r = Σ_c P_rc y_c saved
    from the forward: da_r = G_r (R_r − y_r) / tau; dy_c = (Σ_r G_r P_rc a_r − G_c a_c) / tau, the sum
    being one column pass. Both passes add their diagonal term last (``pd`` = P_rr goes from the row
    pass to the column pass), so the two subtractions do not keep a long chain's rounding of the part
    they remove."""

    @staticmethod
    def forward(ctx, a, y, tau, want):
        lse, diag, pd, R = infonce_row_pass(a, y, tau, want_R=want)
        ctx.tau = float(tau)
        if want:
            ctx.save_for_backward(a, y, lse, pd, R)
        return lse - diag

    @staticmethod
    def backward(ctx, g):
        a, y, lse, pd, R = ctx.saved_tensors
        inv_tau = 1.0 / ctx.tau
        G = _f32(g)
        Gc = G.unsqueeze(1)
        da = dy = None
        if ctx.needs_input_grad[0]:
            da = (inv_tau * (Gc * (R - y))).to(a.dtype)
        if ctx.needs_input_grad[1]:
            dy = (inv_tau * (infonce_col_pass(a, y, ctx.tau, lse, pd, G) - Gc * a)).to(y.dtype)
        return da, dy, None, None


def infonce_rows(a: torch.Tensor, y: torch.Tensor, tau: float) -> torch.Tensor:
    """The per-row InfoNCE losses ``−log softmax(a yᵀ / tau)_rr`` [B] of two fp32 ``B × d`` matrices
    (the caller normalises), by two streaming HIP passes (csrc/gdd_infonce.hip): no logit is stored,
    the forward and the backward give the same bits on every run. Under ``torch.no_grad()``, or when
    neither input needs a gradient, the backward's ``R`` is not computed."""
    want = torch.is_grad_enabled() and (a.requires_grad or y.requires_grad)  # ctx cannot tell no_grad
    return _InfoNCERows.apply(a, y, tau, want)


def infonce(x: torch.Tensor, y: torch.Tensor, tau: float = 0.15, b_cos: bool = True) -> torch.Tensor:
    """model.py:10-24: ``−diag(log_softmax(x̂ ŷᵀ / tau)).mean()``, rows L2-normalised when ``b_cos``."""
    if b_cos:
        x, y = F.normalize(x), F.normalize(y)
    return infonce_rows(x, y, tau).mean()


class _RowPass(torch.autograd.Function):
    """(s, s_sum, SK, SV, A) = rowpass(Q, K, V). Backward, with t_e = g_s[e] + g_sum[r] + ⟨gA_r, V_c⟩:
    dQ_r = Σ t_e K_c; dK_c = Σ_r (gSK_r + t_e Q_r); dV_c = Σ_r (gSV_r + s_e gA_r): an edge-dot pass
    and weighted row sums over the CSR and its transpose."""

    @staticmethod
    def forward(ctx, Q, K, V, side):
        ctx.set_materialize_grads(False)
        s, s_sum, SK, SV, A = rank_rowpass(side, Q, K, V)
        ctx.side = side
        ctx.save_for_backward(Q, K, V, s)
        return s, s_sum, SK, SV, A

    @staticmethod
    def backward(ctx, g_s, g_sum, gSK, gSV, gA):
        Q, K, V, s = ctx.saved_tensors
        side, T = ctx.side, ctx.side.T
        t = g_s
        if g_sum is not None:
            t = _add(t, g_sum[side.rows_l])
        if gA is not None:
            t = _add(t, _edge_dots(side, gA, V))
        dQ = dK = dV = None
        ones = None
        if ctx.needs_input_grad[0] and t is not None:
            dQ = rank_wsum(side, t, K)[0]
        if ctx.needs_input_grad[1]:
            if t is not None:
                dK = rank_wsum(T, t[side.to_T], Q)[0]
            if gSK is not None:
                ones = torch.ones(side.nnz, dtype=torch.float32, device=Q.device)
                dK = _add(dK, rank_wsum(T, ones, gSK)[0])
        if ctx.needs_input_grad[2]:
            if gSV is not None:
                if ones is None:
                    ones = torch.ones(side.nnz, dtype=torch.float32, device=Q.device)
                dV = rank_wsum(T, ones, gSV)[0]
            if gA is not None:
                dV = _add(dV, rank_wsum(T, s[side.to_T], gA)[0])
        return dQ, dK, dV, None


class _WSum(torch.autograd.Function):
    """(Y, ta, tb) = wsum(w, V, a, b). Backward: dw_e = ⟨gY_r, V_c⟩, dV the transposed wsum,
    da_e = gta[r], db_e = gtb[r]."""

    @staticmethod
    def forward(ctx, w, V, a, b, side):
        ctx.set_materialize_grads(False)
        Y, ta, tb = rank_wsum(side, w, V, a, b)
        ctx.side = side
        ctx.save_for_backward(w, V)
        if ta is None:
            ta = Y.new_zeros(0)
        if tb is None:
            tb = Y.new_zeros(0)
        return Y, ta, tb

    @staticmethod
    def backward(ctx, gY, gta, gtb):
        w, V = ctx.saved_tensors
        side = ctx.side
        dw = dV = da = db = None
        if gY is not None:
            if ctx.needs_input_grad[0]:
                dw = _edge_dots(side, gY, V)
            if ctx.needs_input_grad[1]:
                dV = rank_wsum(side.T, w[side.to_T], gY)[0]
        if gta is not None and ctx.needs_input_grad[2]:
            da = gta[side.rows_l]
        if gtb is not None and ctx.needs_input_grad[3]:
            db = gtb[side.rows_l]
        return dw, dV, da, db, None


class InteractionGraph:
    """The distinct training pairs of ``n`` users and ``m`` items as a canonical device CSR
    (``users``: n × m, ascending distinct columns per row) and its transpose (``items``: m × n)."""

    def __init__(self, train_u, train_i, num_users: int, num_items: int, device="cuda"):
        n, m = int(num_users), int(num_items)
        u = np.asarray(train_u.cpu() if isinstance(train_u, torch.Tensor) else train_u, dtype=np.int64).ravel()
        i = np.asarray(train_i.cpu() if isinstance(train_i, torch.Tensor) else train_i, dtype=np.int64).ravel()
        if u.shape != i.shape:
            raise ValueError("train_u and train_i differ in length")
        if n < 1 or m < 1 or n >= 2 ** 31 or m >= 2 ** 31 or u.shape[0] >= 2 ** 31:
            raise ValueError("InteractionGraph: sizes outside int32")
        if u.size and (u.min() < 0 or u.max() >= n or i.min() < 0 or i.max() >= m):
            raise IndexError("InteractionGraph: a user or item id is out of range")
        key = np.sort(u * m + i)
        if key.size and bool((key[1:] == key[:-1]).any()):
            raise ValueError("InteractionGraph: duplicate (user, item) pairs; the layer is defined over "
                             "distinct training pairs (the reference would count a repeat twice)")
        E = int(key.shape[0])
        lib = _lib.device_lib()  # after the host validation: a bad input raises without a device
        dev = torch.device(device)
        self.n, self.m, self.E, self.device = n, m, E, dev
        rowptr = np.zeros(n + 1, np.int64)
        np.cumsum(np.bincount(key // m, minlength=n), out=rowptr[1:])
        self.pair_ids = torch.from_numpy(key).to(dev)  # sorted u*m+i: the sampler's membership test
        self.bad = torch.zeros(1, dtype=torch.int32, device=dev)
        rp = torch.from_numpy(rowptr.astype(np.int32)).to(dev)
        col = torch.from_numpy((key % m).astype(np.int32)).to(dev)
        rp_t = torch.zeros(m + 1, dtype=torch.int32, device=dev)
        col_t = torch.empty(E, dtype=torch.int32, device=dev)
        perm = torch.empty(E, dtype=torch.int32, device=dev)
        if E:
            ws = _lib.workspace(lib.gdd_csr_transpose_ws_bytes(n, m, E), dev)
            _lib.check(lib.gdd_csr_transpose(n, m, E, rp.data_ptr(), col.data_ptr(), None, rp_t.data_ptr(),
                                             col_t.data_ptr(), None, perm.data_ptr(), ws.data_ptr(),
                                             ws.numel(), _lib.stream_ptr(dev)))
        self.users = _Side(n, m, rp, col, self.bad)
        self.items = _Side(m, n, rp_t, col_t, self.bad)
        perm_l = perm.long()
        inv = torch.empty_like(perm_l)
        inv[perm_l] = torch.arange(E, device=dev)
        self.users.T, self.users.to_T = self.items, perm_l
        self.items.T, self.items.to_T = self.users, inv
        deg_u = torch.from_numpy(np.diff(rowptr)).to(dev)
        self.deg_u = deg_u.clamp(min=1).to(torch.float32)  # GCN's clamped degrees
        self.deg_i = (rp_t[1:] - rp_t[:-1]).clamp(min=1).to(torch.float32)
        self.full_user = deg_u >= m  # users without a negative item
        self.dpos = self.deg_u.unsqueeze(1)  # d⁺ [n, 1]
        self.dneg = (m - deg_u).clamp(min=1).to(torch.float32).unsqueeze(1)  # d⁻ [n, 1]
        self.train_u = self.users.rows_l  # the pairs in CSR order (int64)
        self.train_i = col.long()
        self._pair_sets: Optional[Tuple[torch.Tensor, torch.Tensor]] = None

    def _pairs(self) -> Tuple[torch.Tensor, torch.Tensor]:
        if self._pair_sets is None:  # once per graph: the full-batch contrastive loss asks every epoch
            self._pair_sets = (torch.unique(self.train_u), torch.unique(self.train_i))
        return self._pair_sets

    @property
    def pair_users(self) -> torch.Tensor:
        """``unique(train_u)``: the users with a training pair, ascending (int64)."""
        return self._pairs()[0]

    @property
    def pair_items(self) -> torch.Tensor:
        """``unique(train_i)``: the items with a training pair, ascending (int64)."""
        return self._pairs()[1]

    def check(self) -> None:
        """Raise if a pass met a column outside its table (one host read)."""
        if int(self.bad.item()):
            raise IndexError("rankformer: a CSR column is out of range")

    def to_scipy(self) -> sp.csr_matrix:
        return sp.csr_matrix((np.ones(self.E, np.float32), self.users.col.cpu().numpy(),
                              self.users.rowptr.cpu().numpy()), shape=(self.n, self.m))


class RankformerLayer(nn.Module):
    """rec.py:143-274 in the fused form of the module docstring. ``forward(x, graph)``: x is
    ``(n+m, d)`` fp32, users first; returns ``cat(z_u, z_i)``.

    The ablation switches (rec.py:219-221, :263-274) change the algebra around the two row passes,
    not the passes. ``del_benchmark`` takes ``b⁺ = b⁻ = 0`` in Ω and in the second term of each
    denominator (the first term of the user denominators, ``b⁺`` resp. ``−b⁻`` itself, stays: the
    reference recomputes it from the sums). ``del_neg`` drops the negative numerator and denominator.
    ``del_omega_norm`` returns the numerator undivided. With all three off the layer computes what it
    always did, bit for bit."""

    def __init__(self, alpha: float = 2.0, clamp_value: float = 0.0, del_neg: bool = False,
                 del_benchmark: bool = False, del_omega_norm: bool = False):
        super().__init__()
        self.alpha, self.clamp_value = float(alpha), float(clamp_value)
        self.del_neg, self.del_benchmark = bool(del_neg), bool(del_benchmark)
        self.del_omega_norm = bool(del_omega_norm)

    def forward(self, x: torch.Tensor, graph: InteractionGraph) -> torch.Tensor:
        _check_dim(x.shape[1])
        n, m, al, c = graph.n, graph.m, self.alpha, self.clamp_value
        if x.shape[0] != n + m:
            raise ValueError("RankformerLayer: x must have num_users + num_items rows")
        xh = F.normalize(x)
        xu, xi = xh[:n], xh[n:]
        vu, vi = x[:n], x[n:]
        dp, dn = graph.dpos, graph.dneg
        s, S, _, SV, A = _RowPass.apply(xu, xi, vi, graph.users)
        S = S.unsqueeze(1)
        bp = S / dp
        bn = ((xu @ xi.sum(0)).unsqueeze(1) - S) / dn
        # the benchmarks as Ω and the second half of each denominator see them
        bpz, bnz = (torch.zeros_like(bp), torch.zeros_like(bn)) if self.del_benchmark else (bp, bn)
        num_u = (A + (al - bnz) * SV) / dp
        if not self.del_neg:
            num_u = num_u + (xu @ (xi.t() @ vi) - A - (bpz + al) * (vi.sum(0) - SV)) / dn
        if self.del_benchmark:
            d1, d2 = (bp + al).clamp(min=c), (al - bn).clamp(min=c)
        else:
            d1 = d2 = (bp - bn + al).clamp(min=c)
        den_u = d1 if self.del_neg else d1 + d2
        # the item side: one weight and two scalars per interaction, in the transposed entry order
        ru, pt = graph.users.rows_l, graph.users.to_T
        op = ((s - bnz[:, 0][ru] + al) / dp[:, 0][ru])[pt]
        if self.del_neg:
            num_i, ta, _ = _WSum.apply(op, vu, op, None, graph.items)
            den_i = ta.clamp(min=c)
        else:
            om = ((s - bpz[:, 0][ru] - al) / dn[:, 0][ru])[pt]
            Y, ta, tb = _WSum.apply(op - om, vu, op, om, graph.items)
            xun = xu / dn
            coef = (bpz + al) / dn
            num_i = Y + xi @ (xun.t() @ vu) - (coef * vu).sum(0)
            den_i = ta.clamp(min=c) + (-(xi @ xun.sum(0) - coef.sum() - tb)).clamp(min=c)
        if self.del_omega_norm:
            return torch.cat([num_u, num_i], 0)
        return torch.cat([num_u / den_u, num_i / den_i.unsqueeze(1)], 0)


class GCNLayer(nn.Module):
    """rec.py:92-140: z_u = Σ_{N_u} x_i / (du^left di^right), z_i = Σ_{N_i} x_u / (du^right di^left),
    degrees clamped at 1: two weighted row sums with fixed weights."""

    def __init__(self, left: float = 1.0, right: float = 0.0):
        super().__init__()
        self.left, self.right = float(left), float(right)
        self._weights = weakref.WeakKeyDictionary()  # graph -> (w1, w2), built on first use

    def _w(self, graph: InteractionGraph):
        w = self._weights.get(graph)
        if w is None:
            du = graph.deg_u.double()[graph.train_u]
            di = graph.deg_i.double()[graph.train_i]
            w1 = (1.0 / du.pow(self.left) / di.pow(self.right)).float()
            w2 = (1.0 / du.pow(self.right) / di.pow(self.left)).float()[graph.users.to_T]
            w = self._weights[graph] = (w1, w2)
        return w

    def forward(self, x: torch.Tensor, graph: InteractionGraph) -> torch.Tensor:
        n = graph.n
        _check_dim(x.shape[1])
        w1, w2 = self._w(graph)
        z_u = _WSum.apply(w1, x[n:], None, None, graph.users)[0]
        z_i = _WSum.apply(w2, x[:n], None, None, graph.items)[0]
        return torch.cat([z_u, z_i], 0)


class NegativeSampler:
    """model.py:103-120 on the device: j uniform in [0, m), redrawn until no (u, j) is a training
    pair; the membership test is a binary search in the sorted pair ids. A user who holds every item
    has no negative and keeps its first draw."""

    def __init__(self, graph: InteractionGraph, seed: int = 0):
        self.graph = graph
        self.gen = torch.Generator(device=graph.device)
        self.gen.manual_seed(int(seed))

    def _is_pair(self, u: torch.Tensor, j: torch.Tensor) -> torch.Tensor:
        g = self.graph
        if g.E == 0:
            return torch.zeros_like(u, dtype=torch.bool)
        q = u * g.m + j
        pos = torch.searchsorted(g.pair_ids, q).clamp(max=g.E - 1)
        return (g.pair_ids[pos] == q) & ~g.full_user[u]

    def __call__(self, u: torch.Tensor) -> torch.Tensor:
        m, dev = self.graph.m, self.graph.device
        u = u.to(dev).long()
        j = torch.randint(0, m, u.shape, generator=self.gen, device=dev)
        mask = self._is_pair(u, j)
        while bool(mask.any()):
            idx = mask.nonzero(as_tuple=True)[0]
            j[idx] = torch.randint(0, m, idx.shape, generator=self.gen, device=dev)
            mask = self._is_pair(u, j)
        return j


class RankformerTeacher(nn.Module):
    """model.py:123-250: embeddings ``normal_(std=0.1)``, optional GCN layers (``gcn_mean`` averages
    the layer outputs), then ``rankformer_layers`` layers blended with ``rankformer_tau``; the BPR
    loss of :402-468, with the contrastive term of :449-465 when ``use_cl``.

    The contrastive branch follows model.py:194-250, quirks included. With ``use_cl`` every GCN
    layer's output gets ``sign(x) · normalize(rand_like(x)) · cl_eps`` added, and the noisy output is
    what the next layer and ``gcn_mean`` see. The contrastive view is the output of GCN layer
    ``cl_layer`` (1-based, noise included, whatever ``gcn_mean``); without GCN layers, or with
    ``cl_layer`` outside ``1 .. gcn_layers``, it is the raw embedding table. The noise is drawn only
    in training mode, from a generator seeded from ``seed``, so a seed reproduces a run. The
    reference's evaluation reuses whatever noisy embeddings the last training step left behind
    (model.py:279-280); this project evaluates noise-free embeddings instead. :meth:`computer`
    returns ``(users, items)`` as before and keeps the contrastive view in ``cl_view`` for
    :meth:`loss_bpr`. ``del_neg`` / ``del_benchmark`` / ``del_omega_norm`` are the layer's ablation
    switches (:class:`RankformerLayer`)."""

    def __init__(self, graph: InteractionGraph, hidden_dim: int = 64, use_gcn: bool = False,
                 gcn_layers: int = 1, gcn_left: float = 1.0, gcn_right: float = 0.0, gcn_mean: bool = False,
                 use_rankformer: bool = True, rankformer_layers: int = 1, rankformer_tau: float = 0.5,
                 rankformer_alpha: float = 2.0, rankformer_clamp_value: float = 0.0, seed: int = 12345,
                 use_cl: bool = False, cl_layer: int = 1, cl_lambda: float = 0.05, cl_eps: float = 0.1,
                 cl_tau: float = 0.15, del_neg: bool = False, del_benchmark: bool = False,
                 del_omega_norm: bool = False):
        super().__init__()
        self.graph = graph
        self.hidden_dim = _check_dim(hidden_dim)
        self.use_gcn, self.gcn_layers, self.gcn_mean = bool(use_gcn), int(gcn_layers), bool(gcn_mean)
        self.use_rankformer, self.rankformer_layers = bool(use_rankformer), int(rankformer_layers)
        self.rankformer_tau = float(rankformer_tau)
        self.use_cl, self.cl_layer = bool(use_cl), int(cl_layer)
        self.cl_lambda, self.cl_eps, self.cl_tau = float(cl_lambda), float(cl_eps), float(cl_tau)
        if self.use_cl and not self.cl_tau > 0.0:
            raise ValueError(f"RankformerTeacher: cl_tau must be positive, got {cl_tau!r}")
        self.embedding_user = nn.Embedding(graph.n, self.hidden_dim)
        self.embedding_item = nn.Embedding(graph.m, self.hidden_dim)
        nn.init.normal_(self.embedding_user.weight, std=0.1)
        nn.init.normal_(self.embedding_item.weight, std=0.1)
        self.GCN = GCNLayer(gcn_left, gcn_right)
        self.Rankformer = RankformerLayer(rankformer_alpha, rankformer_clamp_value, del_neg, del_benchmark,
                                          del_omega_norm)
        self.to(graph.device)
        self.sampler = NegativeSampler(graph, seed)
        self.noise_gen = torch.Generator(device=graph.device)  # its own stream: the sampler's is untouched
        self.noise_gen.manual_seed(int(seed) + 2)
        self.cl_view: Optional[Tuple[torch.Tensor, torch.Tensor]] = None

    def computer(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """The propagated (user, item) embeddings (model.py:166-250). With ``use_cl`` the contrastive
        view of the same pass is left in ``cl_view``."""
        g = self.graph
        x = torch.cat([self.embedding_user.weight, self.embedding_item.weight], 0)
        x_cl = x
        noisy = self.use_cl and self.training
        if self.use_gcn:
            outs = [x]
            for layer in range(self.gcn_layers):
                x = self.GCN(x, g)
                if noisy:
                    r = torch.rand(x.shape, generator=self.noise_gen, dtype=x.dtype, device=x.device)
                    x = x + torch.sign(x) * F.normalize(r, dim=-1) * self.cl_eps
                if layer == self.cl_layer - 1:
                    x_cl = x
                outs.append(x)
            if self.gcn_mean:
                x = torch.stack(outs, dim=-1).mean(dim=-1)
        if self.use_rankformer:
            tau = self.rankformer_tau
            for _ in range(self.rankformer_layers):
                x = (1 - tau) * x + tau * self.Rankformer(x, g)
        self.cl_view = (x_cl[:g.n], x_cl[g.n:]) if self.use_cl else None
        return x[:g.n], x[g.n:]

    def loss_bpr(self, users: torch.Tensor, items: torch.Tensor, u: torch.Tensor, i: torch.Tensor,
                 reg_lambda: float = 1e-4, j: Optional[torch.Tensor] = None) -> torch.Tensor:
        """softplus(s_uj − s_ui).mean() + reg_lambda · ½(‖u₀‖² + ‖i₀‖² + ‖j₀‖²)/B (model.py:402-468);
        with ``use_cl`` plus ``cl_lambda · (infonce(users[uu], users_cl[uu]) + infonce(items[ii],
        items_cl[ii]))`` over ``uu = unique(u)``, ``ii = unique(i)`` and the contrastive view the
        last :meth:`computer` left (:449-465)."""
        if j is None:
            j = self.sampler(u)
        u0, i0, j0 = self.embedding_user(u), self.embedding_item(i), self.embedding_item(j)
        ue = users[u]
        s_ui = (ue * items[i]).sum(-1)
        s_uj = (ue * items[j]).sum(-1)
        reg = 0.5 * (u0.norm(2).pow(2) + i0.norm(2).pow(2) + j0.norm(2).pow(2)) / u.shape[0]
        if not self.use_cl:
            return F.softplus(s_uj - s_ui).mean() + reg_lambda * reg
        if self.cl_view is None:
            raise RuntimeError("RankformerTeacher.loss_bpr: use_cl needs the contrastive view of computer()")
        users_cl, items_cl = self.cl_view
        g = self.graph
        if u is g.train_u and i is g.train_i:  # full batch: the same two sets every epoch
            uu, ii = g.pair_users, g.pair_items
        else:
            uu, ii = torch.unique(u), torch.unique(i)
        cl = infonce(users[uu], users_cl[uu], self.cl_tau) + infonce(items[ii], items_cl[ii], self.cl_tau)
        return F.softplus(s_uj - s_ui).mean() + reg_lambda * reg + self.cl_lambda * cl


def train_teacher(num_users: int, num_items: int, train_u, train_i, valid_u, valid_i, *,
                  hidden_dim: int = 64, learning_rate: float = 0.1, reg_lambda: float = 1e-4,
                  loss_batch_size: int = 0, max_epochs: int = 2000, valid_interval: int = 20,
                  stopping_step: int = 10, topk: int = 20, seed: int = 12345, device="cuda", log=None,
                  drop_repeats: bool = False, select_by: str = "recall", topks=None, test_u=None, test_i=None,
                  **model_kwargs):
    """main.py:141-190 with parse.py's defaults: Adam, full-batch BPR (``loss_batch_size = 0``) or
    shuffled mini-batches, validation every ``valid_interval`` epochs by Recall@``topk`` over all
    validation users (:class:`gdd.recsys.RecallEvaluator`), stop after ``stopping_step`` validations
    without a new best, and restore the best epoch's weights. Returns ``(model, history)``;
    ``history`` has ``loss`` (per epoch), ``valid`` ([(epoch, recall)]), ``best_epoch``,
    ``best_recall``. Repeated training pairs raise ``ValueError`` unless ``drop_repeats`` keeps one
    of each (the shipped Ali-Display split repeats 5,296 of its 121,178 lines).

    ``select_by="ndcg"`` follows main.py:100-120 instead: every validation computes precision, recall
    and NDCG at ``topks`` (default ``[topk]``) over all validation users with
    :class:`gdd.rankeval.RankingEvaluator` and logs them in the reference's wording, the epoch kept
    is the one whose NDCG@max(topks) is strictly greater than every earlier one (starting from 0, as
    the reference does), and ``test_u`` / ``test_i`` (optional) are evaluated at each new best.
    ``history`` then has ``valid`` as [(epoch, metrics dict)], ``test`` (the metrics at the best
    epoch, or None), ``best_ndcg`` and ``best_epoch``. The early stop is the same."""
    from .recsys import RecallEvaluator

    if select_by not in ("recall", "ndcg"):
        raise ValueError(f"train_teacher: select_by must be 'recall' or 'ndcg', got {select_by!r}")
    if select_by == "ndcg":
        from .rankeval import check_topks
        topks = check_topks(topks if topks is not None else [topk], int(num_items))

    if not torch.cuda.is_available():
        raise RuntimeError("gdd.rankformer: no HIP device visible (the MI355X path has no CPU fallback)")
    dev = torch.device(device)
    torch.manual_seed(int(seed))
    say = log if log is not None else (lambda *_: None)
    if drop_repeats:
        key = np.unique(np.asarray(train_u, np.int64) * int(num_items) + np.asarray(train_i, np.int64))
        if key.shape[0] != np.asarray(train_u).shape[0]:
            say(f"[data] dropped {np.asarray(train_u).shape[0] - key.shape[0]} repeated training pairs")
        train_u, train_i = key // int(num_items), key % int(num_items)
    graph = InteractionGraph(train_u, train_i, num_users, num_items, dev)
    model = RankformerTeacher(graph, hidden_dim=hidden_dim, seed=seed, **model_kwargs)
    opt = torch.optim.Adam(model.parameters(), lr=learning_rate)
    if select_by == "ndcg":
        return _train_select_ndcg(model, graph, opt, valid_u, valid_i, test_u, test_i, topks, reg_lambda,
                                  loss_batch_size, max_epochs, valid_interval, stopping_step, seed, say)
    evaluator = RecallEvaluator(graph.to_scipy(), valid_u, valid_i, topk, dev, max_users=max(1, int(num_users)))
    shuffle = torch.Generator(device=dev)
    shuffle.manual_seed(int(seed) + 1)

    def validate() -> float:
        model.eval()
        with torch.no_grad():
            users, items = model.computer()
            r = evaluator(users, items)
        model.train()
        graph.check()
        return r

    def one_batch(u, i):
        users, items = model.computer()
        loss = model.loss_bpr(users, items, u, i, reg_lambda)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss.detach()

    best = validate()
    best_epoch = 0
    best_state = copy.deepcopy(model.state_dict())
    say(f"[teacher] epoch 0 Recall@{topk}={best:.6f}")
    losses: List[torch.Tensor] = []
    valid_hist = [(0, best)]
    model.train()
    E = graph.E
    for epoch in range(1, int(max_epochs) + 1):
        if loss_batch_size == 0:
            losses.append(one_batch(graph.train_u, graph.train_i))
        else:
            order = torch.randperm(E, generator=shuffle, device=dev)
            u_s, i_s = graph.train_u[order], graph.train_i[order]
            parts = [one_batch(u_s[b:b + loss_batch_size], i_s[b:b + loss_batch_size])
                     for b in range(0, E, int(loss_batch_size))]
            losses.append(torch.stack(parts).mean())
        if epoch % int(valid_interval) == 0:
            r = validate()
            valid_hist.append((epoch, r))
            say(f"[teacher] epoch {epoch} loss={float(losses[-1]):.6f} Recall@{topk}={r:.6f}")
            if r > best:
                best, best_epoch = r, epoch
                best_state = copy.deepcopy(model.state_dict())
            elif epoch - best_epoch >= int(stopping_step) * int(valid_interval):
                say(f"[teacher] early stop at epoch {epoch}; best epoch {best_epoch}")
                break
    model.load_state_dict(best_state)
    graph.check()
    history = {"loss": [float(x) for x in torch.stack(losses).cpu()] if losses else [],
               "valid": valid_hist, "best_epoch": best_epoch, "best_recall": best}
    return model, history


def _train_select_ndcg(model, graph, opt, valid_u, valid_i, test_u, test_i, topks, reg_lambda,
                       loss_batch_size, max_epochs, valid_interval, stopping_step, seed, say):
    """train_teacher's loop with the reference's model selection (main.py:73-134, :161-190)."""
    from .rankeval import RankingEvaluator, format_metrics

    dev = graph.device
    R_train = graph.to_scipy()
    valid_eval = RankingEvaluator(R_train, valid_u, valid_i, topks, dev)
    test_eval = RankingEvaluator(R_train, test_u, test_i, topks, dev) if test_u is not None else None
    shuffle = torch.Generator(device=dev)
    shuffle.manual_seed(int(seed) + 1)

    def evaluate(ev) -> dict:
        model.eval()
        with torch.no_grad():
            users, items = model.computer()
            m = ev(users, items)
        model.train()
        graph.check()
        return m

    def one_batch(u, i):
        users, items = model.computer()
        loss = model.loss_bpr(users, items, u, i, reg_lambda)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss.detach()

    state = {"ndcg": 0.0, "epoch": 0, "weights": copy.deepcopy(model.state_dict()), "test": None}
    valid_hist = []

    def validate(epoch: int) -> bool:
        m = evaluate(valid_eval)
        valid_hist.append((epoch, m))
        say(f"[teacher] ----- epoch {epoch} validation -----")
        for line in format_metrics(topks, m):
            say(f"[teacher] {line}")
        if not float(m["ndcg"][-1]) > state["ndcg"]:
            return False
        state.update(ndcg=float(m["ndcg"][-1]), epoch=epoch, weights=copy.deepcopy(model.state_dict()))
        if test_eval is not None:
            state["test"] = evaluate(test_eval)
            say(f"[teacher] ===== test result (at {epoch} epoch) =====")
            for line in format_metrics(topks, state["test"]):
                say(f"[teacher] {line}")
        return True

    validate(0)
    losses: List[torch.Tensor] = []
    model.train()
    E = graph.E
    for epoch in range(1, int(max_epochs) + 1):
        if loss_batch_size == 0:
            losses.append(one_batch(graph.train_u, graph.train_i))
        else:
            order = torch.randperm(E, generator=shuffle, device=dev)
            u_s, i_s = graph.train_u[order], graph.train_i[order]
            parts = [one_batch(u_s[b:b + loss_batch_size], i_s[b:b + loss_batch_size])
                     for b in range(0, E, int(loss_batch_size))]
            losses.append(torch.stack(parts).mean())
        if epoch % int(valid_interval) == 0:
            say(f"[teacher] epoch {epoch} loss={float(losses[-1]):.6f}")
            if not validate(epoch) and epoch - state["epoch"] >= int(stopping_step) * int(valid_interval):
                say(f"[teacher] early stop at epoch {epoch}; best epoch {state['epoch']}")
                break
    model.load_state_dict(state["weights"])
    graph.check()
    history = {"loss": [float(x) for x in torch.stack(losses).cpu()] if losses else [],
               "valid": valid_hist, "test": state["test"], "best_epoch": state["epoch"],
               "best_ndcg": state["ndcg"], "topks": list(topks)}
    return model, history


def teacher_state(user_emb: torch.Tensor, item_emb: torch.Tensor) -> Dict[str, torch.Tensor]:
    """The export's contents: the raw embedding weights as fp32 CPU tensors."""
    return {"user_emb": user_emb.detach().to("cpu", torch.float32).contiguous(),
            "item_emb": item_emb.detach().to("cpu", torch.float32).contiguous()}


def save_teacher(path: str, model) -> None:
    """main.py:219-227: ``{"user_emb", "item_emb"}``, the raw embedding weights (not the propagated
    ones) as fp32 CPU tensors: the file ``gdd.distill_recsys --teacher_path`` loads. ``model`` is a
    :class:`RankformerTeacher` or anything with ``embedding_user`` / ``embedding_item``."""
    torch.save(teacher_state(model.embedding_user.weight, model.embedding_item.weight), path)
