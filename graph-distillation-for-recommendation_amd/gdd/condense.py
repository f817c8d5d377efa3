"""Graph condensation of ClustGDD on MI355X: sparsification and the cluster-level graph.

Drop-in for (same names, argument meaning and return structure):

* ``utils_clustgdd.ER_estimator(adj, src, dst)`` (ClustGDD/utils_clustgdd.py:149-159) —
  :func:`ER_estimator`;
* ``utils_clustgdd.attaw_ER_estimator(adj, ebd, src, dst)`` (:162-182) — :func:`attaw_ER_estimator`;
* ``ClustGDD.graph_sparse(adj, ratio, ebd, sp_type)`` (clustgdd_agent_transduct.py:131-232,
  clustgdd_agent_induct.py:156-256) — :func:`graph_sparse`, sp_type 'vanilla', 'attaw', 'single'
  'no_sp' and 'rand' (uniform edge samples from torch's global CPU generator, as the reference);
* ``ClustGDD.graph_compress(cluster_labels, adj_norm, adj_list)`` (:234-250, induct :258-274) —
  :func:`graph_compress`, returning torch sparse COO tensors like the reference's ``.to_sparse()``.

Graphs are :class:`gdd.graph.CSRGraph` (anything :func:`gdd.graph.to_csr` accepts is converted).
The reference builds a dense N x k one-hot matrix and runs two GEMMs per graph (~0.7 s each on
the arxiv CPU path) and a host ``torch.topk`` per class; here every step is an O(nnz) kernel in
libgdd (csrc/gdd_condense.hip). Orders and tolerances: oracle/condense.py.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .graph import CSRGraph, to_csr


def _csr(adj, device=None) -> CSRGraph:
    if isinstance(adj, CSRGraph):
        return adj
    return to_csr(adj, device=device or "cuda", binary=False)


def coo_rows(adj: CSRGraph) -> torch.Tensor:
    """Row index of every CSR entry (int32 [nnz]), cached on the graph object."""
    rows = getattr(adj, "_rows", None)
    if rows is None:
        lib = _lib.device_lib()
        rows = torch.empty(adj.nnz, dtype=torch.int32, device=adj.device)
        _lib.check(lib.gdd_coo_rows(adj.n, adj.rowptr.data_ptr(), _lib.ptr(rows),
                                    _lib.stream_ptr(adj.device)))
        adj._rows = rows
    return rows


def ER_estimator(adj, src=None, dst=None) -> torch.Tensor:
    """Effective-resistance lower bound per edge: v/deg[src] + v/deg[dst] (utils_clustgdd:149-159).

    ``src``/``dst`` are accepted for signature compatibility; the edges are the CSR entries of
    ``adj`` in order (the reference passes exactly ``adj.coalesce()._indices()``).
    """
    adj = _csr(adj)
    lib = _lib.device_lib()
    dev = adj.device
    er = torch.empty(adj.nnz, dtype=torch.float32, device=dev)
    ws = _lib.workspace(lib.gdd_er_ws_bytes(adj.n, 1), dev)
    _lib.check(lib.gdd_vanilla_er(adj.n, adj.nnz, adj.rowptr.data_ptr(), _lib.ptr(coo_rows(adj)),
                                  _lib.ptr(adj.col), _lib.ptr(adj.val), _lib.ptr(er), ws.data_ptr(),
                                  ws.numel(), _lib.stream_ptr(dev)))
    return er


def attaw_ER_estimator(adj, ebd: torch.Tensor, src=None, dst=None):
    """(ER_lower, reweighted graph) with edge values ``val * cos(ebd[src], ebd[dst])``
    (utils_clustgdd.py:162-182)."""
    adj = _csr(adj)
    lib = _lib.device_lib()
    dev = adj.device
    ebd = ebd.detach().to(dev, torch.float32).contiguous()
    if ebd.dim() != 2 or ebd.shape[0] != adj.n:
        raise ValueError(f"ebd must be [{adj.n}, C], got {tuple(ebd.shape)}")
    C = ebd.shape[1]
    er = torch.empty(adj.nnz, dtype=torch.float32, device=dev)
    rew = torch.empty(adj.nnz, dtype=torch.float32, device=dev)
    ws = _lib.workspace(lib.gdd_er_ws_bytes(adj.n, C), dev)
    _lib.check(lib.gdd_attaw_er(adj.n, adj.nnz, adj.rowptr.data_ptr(), _lib.ptr(coo_rows(adj)),
                                _lib.ptr(adj.col), _lib.ptr(adj.val), C, ebd.data_ptr(), _lib.ptr(rew),
                                _lib.ptr(er), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
    g = CSRGraph(adj.rowptr, adj.col, rew, adj.n)
    g._rows = coo_rows(adj)
    return er, g


def softmax_rows(x: torch.Tensor) -> torch.Tensor:
    """F.softmax(x, dim=-1) for an n x C fp32 matrix."""
    lib = _lib.device_lib()
    x = x.detach().to(torch.float32).contiguous()
    p = torch.empty_like(x)
    _lib.check(lib.gdd_softmax_rows(x.shape[0], x.shape[1], x.data_ptr(), p.data_ptr(),
                                    _lib.stream_ptr(x.device)))
    return p


def topk_edges(adj: CSRGraph, er: torch.Tensor, m: int, probs: Optional[torch.Tensor] = None):
    """Ascending edge ids of the m largest weights per set (int32 [sets, m])."""
    lib = _lib.device_lib()
    dev = adj.device
    nsets = 1 if probs is None else int(probs.shape[1])
    sel = torch.empty((nsets, m), dtype=torch.int32, device=dev)
    ws = _lib.workspace(lib.gdd_topk_ws_bytes(adj.nnz, nsets), dev)
    _lib.check(lib.gdd_class_topk(adj.nnz, _lib.ptr(coo_rows(adj)), _lib.ptr(adj.col), _lib.ptr(er),
                                  nsets, _lib.ptr(probs), int(m), _lib.ptr(sel), ws.data_ptr(),
                                  ws.numel(), _lib.stream_ptr(dev)))
    return sel


def select_graph(adj: CSRGraph, sel: torch.Tensor, values: torch.Tensor) -> CSRGraph:
    """The sub-graph of the selected CSR entries (ascending ids), carrying ``values[sel]``."""
    lib = _lib.device_lib()
    dev = adj.device
    m = int(sel.numel())
    rowptr = torch.empty(adj.n + 1, dtype=torch.int32, device=dev)
    col = torch.empty(m, dtype=torch.int32, device=dev)
    val = torch.empty(m, dtype=torch.float32, device=dev)
    ws = _lib.workspace(lib.gdd_select_csr_ws_bytes(adj.n), dev)
    _lib.check(lib.gdd_select_csr(adj.n, _lib.ptr(coo_rows(adj)), _lib.ptr(adj.col),
                                  _lib.ptr(values), m, _lib.ptr(sel), rowptr.data_ptr(), _lib.ptr(col),
                                  _lib.ptr(val), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev)))
    return CSRGraph(rowptr, col, val, adj.n)


def graph_sparse(adj, ratio: float, ebd: Optional[torch.Tensor] = None,
                 sp_type: str = "vanilla") -> List[CSRGraph]:
    """ClustGDD.graph_sparse (clustgdd_agent_transduct.py:131-232): the sparsified graph(s).

    'attaw' returns one graph per class (``ebd.shape[-1]`` of them): the ``int(nnz*ratio)`` edges
    with the largest ``softmax(ebd)[src,i] * softmax(ebd)[dst,i] * ER_attaw``, carrying the
    cosine-reweighted values. 'single' selects on ``ER_attaw`` alone (reweighted values),
    'vanilla' on ``ER_estimator`` (original values). torch.topk leaves the choice among exactly
    tied boundary weights unspecified; here ties go to the lower edge index.
    """
    adj = _csr(adj)
    if sp_type == "no_sp":
        return [adj]
    m = int(adj.nnz * ratio)
    if sp_type == "rand":
        # per class a uniform edge sample: torch.randperm on torch's global CPU generator (the
        # reference's call, on whatever device it runs), the first m edges carrying their
        # ER_estimator weight ("tried version", :208-222); the edge set is rebuilt in CSR order
        if ebd is None:
            raise ValueError("sp_type='rand' needs the embeddings (one graph per class)")
        er = ER_estimator(adj)
        out = []
        for _ in range(int(ebd.shape[-1])):
            pick = torch.randperm(adj.nnz)[:m]
            sel = torch.sort(pick).values.to(device=adj.device, dtype=torch.int32)
            out.append(select_graph(adj, sel, er))
        return out
    if sp_type == "vanilla":
        er = ER_estimator(adj)
        return [select_graph(adj, topk_edges(adj, er, m)[0], adj.values())]
    if ebd is None:
        raise ValueError(f"sp_type={sp_type!r} needs the embeddings")
    er, rew = attaw_ER_estimator(adj, ebd)
    if sp_type == "single":
        return [select_graph(adj, topk_edges(adj, er, m)[0], rew.val)]
    if sp_type == "attaw":
        probs = softmax_rows(ebd.to(adj.device))
        sel = topk_edges(adj, er, m, probs)
        return [select_graph(adj, sel[i], rew.val) for i in range(sel.shape[0])]
    raise ValueError(f"unknown sp_type {sp_type!r}")


def _labels_device(cluster_labels, device) -> torch.Tensor:
    if isinstance(cluster_labels, torch.Tensor):
        return cluster_labels.to(device=device, dtype=torch.int32).contiguous()
    return torch.from_numpy(np.asarray(cluster_labels, dtype=np.int32)).to(device)


def _label_range(labels: torch.Tensor, n: int):
    """(min, max) of the labels on the host (one transfer), after the shape check."""
    if labels.dim() != 1 or labels.numel() != n or n == 0:
        raise ValueError(f"cluster labels must be one per node ([{n}]), got {tuple(labels.shape)}")
    lo, hi = torch.aminmax(labels)
    lo, hi = torch.stack([lo, hi]).tolist()
    if lo < 0:
        raise ValueError(f"cluster labels must be >= 0, got {lo} (an unassigned node?): the "
                         "reference's one_hot rejects it too")
    return lo, hi


def compress_dense(labels: torch.Tensor, adj: CSRGraph, kk: int) -> torch.Tensor:
    """P^T A P with the diagonal removed, dense kk x kk fp32 on the device. Labels outside
    [0, kk) are refused before any launch."""
    hi = _label_range(labels, adj.n)[1]
    if hi >= kk:
        raise ValueError(f"cluster label {hi} is outside [0, {int(kk)})")
    return _compress_dense(labels, adj, kk)


def _compress_dense(labels: torch.Tensor, adj: CSRGraph, kk: int) -> torch.Tensor:
    lib = _lib.device_lib()
    dev = adj.device
    out = torch.empty((kk, kk), dtype=torch.float32, device=dev)
    ws = _lib.workspace(lib.gdd_compress_ws_bytes(kk), dev)
    _lib.check(lib.gdd_graph_compress(adj.n, labels.data_ptr(), int(kk), adj.nnz,
                                      _lib.ptr(coo_rows(adj)), _lib.ptr(adj.col), _lib.ptr(adj.val),
                                      None, out.data_ptr(), ws.data_ptr(), ws.numel(),
                                      _lib.stream_ptr(dev)))
    return out


def _stack_to_sparse(stack: torch.Tensor):
    """[G, kk, kk] dense -> G coalesced sparse COO tensors (what ``.to_sparse()`` gives each),
    with two host round trips for all G instead of one per matrix."""
    G, kk = stack.shape[0], stack.shape[1]
    idx = stack.nonzero()  # row-major: graph, row, col (NaN counts as nonzero, as in to_sparse)
    vals = stack[idx[:, 0], idx[:, 1], idx[:, 2]]
    counts = torch.bincount(idx[:, 0], minlength=G).cpu().tolist()
    out, o = [], 0
    for c in counts:
        ij = idx[o:o + c, 1:].t().contiguous()
        out.append(torch.sparse_coo_tensor(ij, vals[o:o + c], (kk, kk), is_coalesced=True))
        o += c
    return out


def graph_compress(cluster_labels, adj_norm, adj_list: Sequence, dense: bool = False):
    """ClustGDD.graph_compress (clustgdd_agent_transduct.py:234-250) -> (compressed_graph_list,
    adj_syn), each ``(P^T A P - diag).to_sparse()`` with P the size-normalised one-hot cluster
    matrix of ``cluster_num = max(label) + 1`` columns. ``dense=True`` returns the dense matrices
    (what graph_refusion consumes via ``.to_dense()``, :276) and skips the sparse conversion."""
    adj_norm = _csr(adj_norm)
    dev = adj_norm.device
    labels = _labels_device(cluster_labels, dev)
    kk = _label_range(labels, adj_norm.n)[1] + 1  # raises on a negative label, before any launch
    graphs = [_csr(a, dev) for a in adj_list] + [adj_norm]
    for g in graphs:
        if g.n != adj_norm.n:
            raise ValueError(f"adj_list graph has {g.n} nodes, adj_norm {adj_norm.n}")
    stack = torch.stack([_compress_dense(labels, g, kk) for g in graphs])
    mats = list(stack.unbind(0)) if dense else _stack_to_sparse(stack)
    return mats[:-1], mats[-1]
