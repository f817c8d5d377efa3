"""Ranked top-K lists straight from a condensed recommender (DESIGN.md "Top-K from the condensed
model"): the lists :func:`gdd.rankeval.recommend` gives on the expanded tables ``cu_z[u2cu]``,
``ci_z[i2ci]``, in every item and every score bit, without building either table.

* stage A — one ``gdd_score_topk`` launch ranks the ``L = min(num_ci, 256)`` best item clusters of
  each of the ``G`` distinct user clusters of the request (``G * num_ci * d`` fmas instead of
  ``B * I * d``; the score of a pair is a function of its two rows alone, so the bits are those of
  the expanded tables);
* stage B — ``gdd_cluster_expand_topk``, one wave per user, expands that ranking into item ids
  through the membership CSR, drops the user's excluded items (which enter with ``mask_value``, as
  in ``recommend``) and stops once ``k`` items beat everything not yet examined;
* a user whose ``L`` clusters do not settle its list (``L < num_ci`` only) is recomputed by
  ``gdd_score_topk`` against ``ci_z[i2ci]``, built at that point and kept.

:class:`CondensedRecommender` holds what is prepared once (tables, maps, membership CSR) and can be
loaded from the artefact :func:`gdd.recsys.save_distilled` writes; :func:`recommend_condensed` is
the one-call form. The exclude rows of a call come from :func:`mask_rows`, which slices a scipy CSR in
canonical form instead of sorting it. Argument errors raise ``ValueError`` before the device is touched. There is no
CPU path.
"""
from __future__ import annotations

import os
from typing import Optional, Tuple

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from .rankeval import (MAX_K, _check_k, _check_tables, _check_users, _f32, _gather_rows, _np_ids, _raise_bad,
                       _rows_of, _score_topk, _to_dev)

MAX_LIST = MAX_K  # clusters ranked per user cluster: one gdd_score_topk list


def membership_csr(i2ci, num_ci: int) -> Tuple[np.ndarray, np.ndarray]:
    """``(mem_ptr int32 [num_ci + 1], mem_item int32 [I])``: the items of every cluster in ascending
    id (a stable host argsort of the labels). Empty clusters are empty rows."""
    lab = _np_ids(i2ci)
    num_ci = int(num_ci)
    if lab.size and (lab.min() < 0 or lab.max() >= num_ci):
        raise ValueError(f"i2ci holds a cluster id outside [0, {num_ci})")
    if lab.size >= 2 ** 31:
        raise ValueError("i2ci outside int32 item ids")
    ptr = np.zeros(num_ci + 1, np.int64)
    np.cumsum(np.bincount(lab, minlength=num_ci), out=ptr[1:])
    return ptr.astype(np.int32), np.argsort(lab, kind="stable").astype(np.int32)


def _check_model(cu_z, ci_z, u2cu, i2ci) -> Tuple[np.ndarray, np.ndarray]:
    num_cu, num_ci, _ = _check_tables(cu_z, ci_z)
    a, b = _np_ids(u2cu), _np_ids(i2ci)
    if a.size and (a.min() < 0 or a.max() >= num_cu):
        raise ValueError(f"u2cu holds a cluster id outside [0, {num_cu})")
    if b.size and (b.min() < 0 or b.max() >= num_ci):
        raise ValueError(f"i2ci holds a cluster id outside [0, {num_ci})")
    if a.size < 1 or b.size < 1 or a.size >= 2 ** 31 or b.size >= 2 ** 31:
        raise ValueError("u2cu / i2ci must map 1 to 2^31 - 1 users / items")
    return a, b


def _distinct_columns(ptr: np.ndarray, col: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Rows sorted by column with repeats removed (the expansion enters each masked item once)."""
    if col.size < 2:
        return ptr, col
    row = np.repeat(np.arange(ptr.shape[0] - 1), np.diff(ptr.astype(np.int64)))
    rep = np.zeros(col.shape[0], bool)
    rep[1:] = (col[1:] == col[:-1]) & (row[1:] == row[:-1])
    if not rep.any():
        return ptr, col
    out = np.zeros(ptr.shape[0], np.int64)
    np.cumsum(np.bincount(row[~rep], minlength=ptr.shape[0] - 1), out=out[1:])
    return out.astype(np.int32), col[~rep]


def mask_rows(exclude, ids: Optional[np.ndarray], num_users: int, num_items: int) -> Tuple[np.ndarray, np.ndarray]:
    """The rows ``ids`` (None: the first ``num_users`` rows, in order) of ``exclude`` as an int32 CSR
    with strictly ascending columns: what ``gdd_cluster_expand_topk`` takes as its mask. A scipy
    matrix in canonical CSR form (sorted, distinct columns: what ``tocsr()`` gives) is sliced without
    a sort; anything else goes through :func:`gdd.rankeval._rows_of` and loses its repeats."""
    if sp.issparse(exclude):
        m = sp.csr_matrix(exclude)
        if not m.has_canonical_format:
            m = m.copy()
            m.sum_duplicates()
        n_rows = int(m.shape[0])
        if m.indptr[-1] >= 2 ** 31:
            raise ValueError("exclude rows outside int32")
        if ids is None:
            if n_rows < num_users:
                raise ValueError("exclude has no row for some selected user")
            ptr = m.indptr[:num_users + 1]
            return ptr.astype(np.int32), m.indices[:ptr[-1]].astype(np.int32)
        ptr, col = _gather_rows(m.indptr, m.indices, ids)
        return ptr, col.astype(np.int32)
    return _distinct_columns(*_rows_of(exclude, ids if ids is not None else np.arange(num_users), num_items))


class CondensedRecommender:
    """The condensed model ready to rank: ``cu_z`` (num_cu x d) and ``ci_z`` (num_ci x d) on the
    device, ``u2cu`` / ``i2ci`` the cluster of every original user / item. ``last_info`` describes
    the last :meth:`recommend`: ``fallback_users`` (recomputed against the expanded item table),
    ``ranked_clusters`` (G) and ``list_len`` (L)."""

    def __init__(self, cu_z: torch.Tensor, ci_z: torch.Tensor, u2cu, i2ci):
        self._u2cu, self._i2ci = _check_model(cu_z, ci_z, u2cu, i2ci)
        self.num_cu, self.num_ci, self.dim = _check_tables(cu_z, ci_z)
        self.num_users, self.num_items = int(self._u2cu.shape[0]), int(self._i2ci.shape[0])
        self._mem_host = membership_csr(self._i2ci, self.num_ci)
        self._tables = (cu_z, ci_z)
        self.device = ci_z.device
        self._dev = None
        self._expanded: Optional[torch.Tensor] = None
        self.last_info: dict = {}

    # ---- construction ---------------------------------------------------------------------------
    @classmethod
    def from_model(cls, model, u2cu, i2ci) -> "CondensedRecommender":
        """From a live :class:`gdd.recsys.LightGCNCondensed`: its propagated tables."""
        with torch.no_grad():
            cu_z, ci_z = model.propagate()
        return cls(cu_z.detach(), ci_z.detach(), u2cu, i2ci)

    @classmethod
    def load(cls, path: str, device="cuda", num_layers: int = 2) -> "CondensedRecommender":
        """From the directory :func:`gdd.recsys.save_distilled` writes: ``condensed_graph.npz``
        {cu, ci, w, num_cu, num_ci}, ``u2cu.npy``, ``i2ci.npy``, ``condensed_embeddings.pt``. The
        tables are recomputed by :func:`gdd.recsys.lightgcn_propagate` from the saved edge weights
        ``w`` (``num_layers``: the ``--lgn_layers`` of the run, which the artefact does not hold)."""
        from .recsys import _Bipartite, lightgcn_propagate
        with np.load(os.path.join(path, "condensed_graph.npz")) as z:
            cu, ci, w = z["cu"], z["ci"], z["w"]
            num_cu, num_ci = int(z["num_cu"]), int(z["num_ci"])
        u2cu, i2ci = np.load(os.path.join(path, "u2cu.npy")), np.load(os.path.join(path, "i2ci.npy"))
        emb = torch.load(os.path.join(path, "condensed_embeddings.pt"), map_location="cpu", weights_only=True)
        if tuple(emb["user_emb"].shape[:1]) != (num_cu,) or tuple(emb["item_emb"].shape[:1]) != (num_ci,):
            raise ValueError(f"{path}: embeddings of {emb['user_emb'].shape[0]} x {emb['item_emb'].shape[0]} "
                             f"clusters for a graph of {num_cu} x {num_ci}")
        _lib.device_lib()
        dev = torch.device(device)
        with torch.no_grad():
            u0 = (emb["user_emb"] + emb["user_delta"]).to(dev)
            i0 = (emb["item_emb"] + emb["item_delta"]).to(dev)
            edge_index = torch.from_numpy(np.stack([cu, ci]).astype(np.int64)).to(dev)
            graph = _Bipartite(edge_index, num_cu, num_ci)
            cu_z, ci_z = lightgcn_propagate(u0, i0, torch.from_numpy(w.astype(np.float32)).to(dev), edge_index,
                                            graph, num_layers)
        return cls(cu_z, ci_z, u2cu, i2ci)

    # ---- device state ---------------------------------------------------------------------------
    def _prepare(self):
        if self._dev is None:
            _lib.device_lib()
            t = lambda a, dt=None: _to_dev(a, self.device, dt)  # noqa: E731
            mp, mi = self._mem_host
            self._dev = dict(cu_z=_f32(self._tables[0]), ci_z=_f32(self._tables[1]), mem_ptr=t(mp), mem_item=t(mi),
                             u2cu=t(self._u2cu, np.int32), i2ci=t(self._i2ci))
        return self._dev

    def _grouped(self, ids: Optional[np.ndarray]):
        """The user clusters of a request (``ids``: checked user ids or None, every user), at least one
        user: ``(cl_of, groups_t, row_t)``, the cluster of each user on the host, the distinct clusters
        and each user's index into them as int32 device tensors (``G = groups_t.numel()``)."""
        cl_of = self._u2cu if ids is None else self._u2cu[ids]
        groups, row = np.unique(cl_of, return_inverse=True)
        return cl_of, _to_dev(groups, self.device, np.int32), _to_dev(row.ravel(), self.device, np.int32)

    @property
    def cu_z(self) -> torch.Tensor:
        return self._prepare()["cu_z"]

    @property
    def ci_z(self) -> torch.Tensor:
        return self._prepare()["ci_z"]

    def expanded_items(self) -> torch.Tensor:
        """``ci_z[i2ci]`` (I x d), built on first use and kept: the fallback's item table."""
        if self._expanded is None:
            g = self._prepare()
            self._expanded = g["ci_z"][g["i2ci"]].contiguous()
        return self._expanded

    def workspace_bytes(self, batch: int, groups: int) -> int:
        """Device bytes one :meth:`recommend` allocates besides its outputs and its copy of the mask:
        the cluster lists (ids and scores), each user's row of them, the distinct clusters, the
        incomplete flags and the two counters."""
        L = min(self.num_ci, MAX_LIST)
        return 8 * groups * L + 4 * batch + 4 * groups + 4 * batch + 8

    # ---- the lists ------------------------------------------------------------------------------
    def _lists(self, k: int, ids: Optional[np.ndarray], mask_np, mask_value: float, return_scores: bool):
        """``ids``: checked int64 user ids or None (every user); ``mask_np``: their mask rows as an
        int32 host CSR with strictly ascending columns (:func:`mask_rows`) or None."""
        g = self._prepare()
        dev = self.device
        B = self.num_users if ids is None else int(ids.shape[0])
        L = min(self.num_ci, MAX_LIST)
        items = torch.empty(B, k, dtype=torch.int32, device=dev)
        scores = torch.empty(B, k, dtype=torch.float32, device=dev) if return_scores else None
        if B == 0:
            self.last_info = {"fallback_users": 0, "ranked_clusters": 0, "list_len": L}
            return items, scores
        cl_of, groups_t, row_t = self._grouped(ids)
        G = int(groups_t.numel())
        t = lambda a: _to_dev(a, dev, np.int32)  # noqa: E731
        users_t = None if ids is None else t(ids)
        mask = None
        if mask_np is not None and int(mask_np[1].shape[0]):
            mask = (t(mask_np[0]), t(mask_np[1]))
        counters = torch.zeros(2, dtype=torch.int32, device=dev)  # bad rows, incomplete rows
        cl_item, cl_score = _score_topk(g["cu_z"], g["ci_z"], L, groups_t, None, 0.0, True, counters[:1])
        incomplete = torch.empty(B, dtype=torch.int32, device=dev)
        mp, mc = mask if mask is not None else (None, None)
        lib = _lib.device_lib()
        _lib.check(lib.gdd_cluster_expand_topk(
            B, self.num_items, self.num_ci, L, k, _lib.ptr(users_t), self.num_users, row_t.data_ptr(), G,
            cl_item.data_ptr(), cl_score.data_ptr(), g["mem_ptr"].data_ptr(), g["mem_item"].data_ptr(),
            _lib.ptr(mp), _lib.ptr(mc), float(mask_value), items.data_ptr(), _lib.ptr(scores),
            incomplete.data_ptr(), counters[1:].data_ptr(), counters[:1].data_ptr(), _lib.stream_ptr(dev)))
        n_bad, n_inc = (int(v) for v in counters.cpu())
        if n_bad:
            _raise_bad(n_bad)
        if n_inc:
            sel = torch.nonzero(incomplete, as_tuple=False).ravel()
            sel_np = sel.cpu().numpy()
            fb_mask = None
            if mask is not None:
                fb_mask = tuple(t(a) for a in _rows_of(mask_np, sel_np, self.num_items))
            fb_items, fb_scores = _score_topk(g["cu_z"], self.expanded_items(), k, t(cl_of[sel_np]), fb_mask,
                                              mask_value, return_scores, counters[:1])
            items[sel] = fb_items
            if return_scores:
                scores[sel] = fb_scores
        self.last_info = {"fallback_users": n_inc, "ranked_clusters": G, "list_len": L}
        return items, scores

    @torch.no_grad()
    def recommend(self, k: int, users=None, exclude=None, mask_value: float = -1024.0,
                  return_scores: bool = False):
        """As :func:`gdd.rankeval.recommend` on ``(cu_z[u2cu], ci_z[i2ci])``: ``users`` are original
        user ids (default: every user, in order; repeats allowed), ``exclude`` a scipy sparse matrix
        or ``(ptr, col)`` CSR over the original users and items."""
        k = _check_k(k, self.num_items)
        ids = _check_users(users, self.num_users)
        mask_np = None
        if exclude is not None:
            mask_np = mask_rows(exclude, ids, self.num_users, self.num_items)
        items, scores = self._lists(k, ids, mask_np, mask_value, return_scores)
        return (items, scores) if return_scores else items

    def positions(self, targets, users=None, exclude=None, mask_value: float = -1024.0) -> torch.Tensor:
        """As :func:`gdd.rankpos.rank_positions` on ``(cu_z[u2cu], ci_z[i2ci])``: the number of items
        ranked above each target, int32 on the device, from the cluster tables
        (``gdd_cluster_positions``). ``last_info`` then holds ``ranked_clusters`` and
        ``workspace_bytes``."""
        from .rankpos import condensed_positions
        return condensed_positions(self, targets, users, exclude, mask_value)


def recommend_condensed(cu_z: torch.Tensor, ci_z: torch.Tensor, u2cu, i2ci, k: int, users=None, exclude=None,
                        mask_value: float = -1024.0, return_scores: bool = False):
    """The ``k`` best items of each user under the condensed model, best first: what
    ``recommend(cu_z[u2cu], ci_z[i2ci], k, users=, exclude=, mask_value=, return_scores=)`` returns,
    item for item and bit for bit. ``u2cu`` entries lie in ``[0, num_cu)``, ``i2ci`` entries in
    ``[0, num_ci)`` (an empty item cluster is legal), ``1 <= k <= min(256, I)``."""
    _check_model(cu_z, ci_z, u2cu, i2ci)
    _check_k(k, int(_np_ids(i2ci).shape[0]))
    return CondensedRecommender(cu_z, ci_z, u2cu, i2ci).recommend(k, users, exclude, mask_value, return_scores)
