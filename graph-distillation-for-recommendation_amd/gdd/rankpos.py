"""Full-ranking positions on MI355X (DESIGN.md "Full-ranking positions"): where a model ranks given
items among all items, and what follows from that (Rankformer/code/model.py:252-343 ``evaluate``,
:27-53 ``test``, without the limit of a 256-item list).

For a user ``b`` and a target item ``t``, ``pos(b, t)`` is the number of items that rank above ``t``
in exactly the order of :func:`gdd.rankeval.recommend` (fp32 fma-chain scores, an excluded item scores
``mask_value``, equal scores by ascending item id): the index at which ``recommend(k = I)`` would list
``t``. No ``B x I`` score matrix is built.

* :func:`rank_positions` — ``gdd_score_positions`` on (user, item) embeddings;
* :func:`rank_positions_condensed` / :meth:`gdd.condrank.CondensedRecommender.positions` — the same
  integers from a condensed model's cluster tables (``gdd_cluster_positions``: an item's position is a
  sum of cluster sizes, a count inside tied clusters and a correction per excluded item);
* :func:`metrics_from_positions` — precision, recall, NDCG at any cut-offs up to ``I``, the reciprocal
  rank of the best held-out item and the mean rank, on the host in fp64;
* :class:`PositionEvaluator` — those over an evaluation split, the counterpart of
  :class:`gdd.rankeval.RankingEvaluator` without its limits on the cut-offs;
* :func:`fidelity` / :func:`ranking_fidelity` — how much of a teacher's top-k lists a student keeps.

Positions are 0-based; a rank is ``pos + 1``. Argument errors raise ``ValueError`` before the device
is touched. There is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib
from .rankeval import (RankingEvaluator, _check_tables, _check_users, _f32, _np_ids, _parse_int_list, _rows_of,
                       _to_dev, recommend)

_BLOCK_ELEMS = 1 << 22  # metrics_from_positions: padded doubles per block of users


def check_cutoffs(topks, num_items: Optional[int] = None) -> Tuple[int, ...]:
    """Any number >= 1 of strictly ascending cut-offs in ``[1, num_items]``."""
    try:
        t = tuple(int(k) for k in topks)
    except TypeError:
        raise ValueError(f"topks must be a sequence of integers, got {topks!r}") from None
    if len(t) < 1:
        raise ValueError("topks must hold at least one cut-off")
    if t[0] < 1 or any(b <= a for a, b in zip(t, t[1:])):
        raise ValueError(f"topks must be strictly ascending positive integers, got {list(t)}")
    if num_items is not None and t[-1] > int(num_items):
        raise ValueError(f"cut-off {t[-1]} exceeds the number of items ({int(num_items)})")
    return t


def parse_cutoffs(text, num_items: Optional[int] = None) -> Tuple[int, ...]:
    """``--report_topks "[20, 500]"`` as a tuple of ints (``ast.literal_eval``), without the limits of
    :func:`gdd.rankeval.parse_topks`."""
    return check_cutoffs(_parse_int_list(text), num_items)


def _raise_bad(n: int) -> None:
    raise RuntimeError(f"rank positions: {n} row(s) with a user id, an excluded item id or a target item id out "
                       "of range (those rows are -1)")


def _check_targets(targets, batch: int, num_items: int):
    """``targets`` as ``(ptr int32 host [batch + 1], col, width)``: ``col`` an int32 host array, or the
    caller's device tensor flattened (a 2-D device tensor is not copied to the host: the kernel checks
    its ids); ``width`` is T for a 2-D ``[batch, T]`` input, None for a ``(ptr, col)`` CSR."""
    if isinstance(targets, tuple):
        if len(targets) != 2:
            raise ValueError("targets must be (ptr, col) or a 2-D integer array")
        ptr, col = (_np_ids(x) for x in targets)
        if ptr.shape[0] != batch + 1:
            raise ValueError(f"targets: ptr of {ptr.shape[0]} entries for {batch} rows")
        if ptr[0] != 0 or (np.diff(ptr) < 0).any() or ptr[-1] != col.shape[0]:
            raise ValueError("targets: ptr must start at 0, not decrease and end at len(col)")
        if col.shape[0] >= 2 ** 31:
            raise ValueError("targets outside int32")
        if col.size and (col.min() < 0 or col.max() >= num_items):
            raise ValueError(f"targets hold an item id outside [0, {num_items})")
        return ptr.astype(np.int32), col.astype(np.int32), None
    on_device = isinstance(targets, torch.Tensor) and targets.device.type != "cpu"
    if on_device:
        a = targets
        if a.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
            raise ValueError(f"targets must hold integers, got {a.dtype}")
        shape = tuple(a.shape)
    else:
        a = targets.detach().numpy() if isinstance(targets, torch.Tensor) else np.asarray(targets)
        if a.dtype.kind not in "iu":
            raise ValueError(f"targets must hold integers, got {a.dtype}")
        shape = a.shape
    if len(shape) != 2 or shape[0] != batch:
        raise ValueError(f"targets of shape {tuple(shape)} for {batch} rows: expected [{batch}, T]")
    width = int(shape[1])
    if batch * width >= 2 ** 31:
        raise ValueError("targets outside int32")
    ptr = (np.arange(batch + 1, dtype=np.int64) * width).astype(np.int32)
    if on_device:
        return ptr, a.detach().to(torch.int32).contiguous().view(-1), width
    if a.size and (a.min() < 0 or a.max() >= num_items):
        raise ValueError(f"targets hold an item id outside [0, {num_items})")
    return ptr, np.ascontiguousarray(a, dtype=np.int32).ravel(), width


def _score_positions(user_emb, item_emb, users_t, mask, mask_value, tg_ptr, tg_col, bad) -> torch.Tensor:
    """One ``gdd_score_positions`` launch on prepared int32 device tensors (``users_t`` / ``mask`` may
    be None)."""
    lib = _lib.device_lib()
    U, V = _f32(user_emb), _f32(item_emb)
    dev = V.device
    B = int(users_t.numel()) if users_t is not None else int(U.shape[0])
    pos = torch.empty(int(tg_col.numel()), dtype=torch.int32, device=dev)
    mp, mc = mask if mask is not None and int(mask[1].numel()) else (None, None)
    _lib.check(lib.gdd_score_positions(B, int(V.shape[0]), int(V.shape[1]), _lib.ptr(users_t), U.data_ptr(),
                                       int(U.shape[0]), V.data_ptr(), _lib.ptr(mp), _lib.ptr(mc),
                                       float(mask_value), tg_ptr.data_ptr(), _lib.ptr(tg_col), pos.data_ptr(),
                                       bad.data_ptr(), _lib.stream_ptr(dev)))
    return pos


@torch.no_grad()
def rank_positions(user_emb: torch.Tensor, item_emb: torch.Tensor, targets, users=None, exclude=None,
                   mask_value: float = -1024.0) -> torch.Tensor:
    """``pos(b, t)`` for the targets of every selected user: int32 on the device, one per target in the
    order given (shape ``[B, T]`` for a 2-D ``targets``, flat for a ``(ptr, col)`` CSR with one row per
    selected user in call order). ``users`` and ``exclude`` as in :func:`gdd.rankeval.recommend`; a
    target may be excluded (it then carries ``mask_value``), repeat, and come in any order.
    ``recommend(...)[b, pos]`` is the target whenever ``pos < k``."""
    nu, ni, _ = _check_tables(user_emb, item_emb)
    ids = _check_users(users, nu)
    B = nu if ids is None else int(ids.shape[0])
    ptr, col, width = _check_targets(targets, B, ni)
    mask_np = None if exclude is None else _rows_of(exclude, ids if ids is not None else np.arange(nu), ni)
    dev = item_emb.device
    _lib.device_lib()
    users_t = None if ids is None else _to_dev(ids, dev, np.int32)
    mask = None if mask_np is None else tuple(_to_dev(a, dev) for a in mask_np)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    pos = _score_positions(user_emb, item_emb, users_t, mask, mask_value, _to_dev(ptr, dev), _to_dev(col, dev),
                           bad)
    n_bad = int(bad.item())
    if n_bad:
        _raise_bad(n_bad)
    return pos if width is None else pos.view(B, width)


def condensed_workspace_bytes(groups: int, num_ci: int) -> int:
    """``gdd_cluster_positions_ws_bytes``: the score of every (user cluster of the call, item cluster)
    and, up to 4096 item clusters, each row of them in ranked order with the prefix cluster sizes."""
    return int(_lib.load().gdd_cluster_positions_ws_bytes(int(groups), int(num_ci)))


def _cluster_positions(rec, ids: Optional[np.ndarray], mask_np, mask_value: float, tg_ptr, tg_col) -> torch.Tensor:
    """``gdd_cluster_positions`` for a :class:`gdd.condrank.CondensedRecommender`. ``ids``: checked
    user ids or None; ``mask_np``: int32 CSR with strictly ascending columns or None; ``tg_ptr`` /
    ``tg_col``: int32; each as host arrays or device tensors."""
    g = rec._prepare()
    dev = rec.device
    B = rec.num_users if ids is None else int(ids.shape[0])
    tg_ptr, tg_col = _to_dev(tg_ptr, dev), _to_dev(tg_col, dev)
    pos = torch.empty(int(tg_col.numel()), dtype=torch.int32, device=dev)
    if B == 0:
        return pos
    if "i2ci32" not in g:
        g["i2ci32"] = g["i2ci"].to(torch.int32)
    _, groups_t, row_t = rec._grouped(ids)  # named, so that they live until the launch is enqueued
    G = int(groups_t.numel())
    users_t = None if ids is None else _to_dev(ids, dev, np.int32)
    mp = mc = None
    if mask_np is not None and int(mask_np[1].shape[0]):
        mp, mc = (_to_dev(a, dev) for a in mask_np)
    lib = _lib.device_lib()
    ws_bytes = int(lib.gdd_cluster_positions_ws_bytes(G, rec.num_ci))
    ws = _lib.workspace(ws_bytes, dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.gdd_cluster_positions(
        B, rec.num_items, rec.num_cu, rec.num_ci, rec.dim, g["cu_z"].data_ptr(), g["ci_z"].data_ptr(),
        _lib.ptr(users_t), rec.num_users, row_t.data_ptr(), G, groups_t.data_ptr(), g["i2ci32"].data_ptr(),
        g["mem_ptr"].data_ptr(),
        g["mem_item"].data_ptr(), _lib.ptr(mp), _lib.ptr(mc), float(mask_value), tg_ptr.data_ptr(),
        _lib.ptr(tg_col), pos.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws_bytes, _lib.stream_ptr(dev)))
    n_bad = int(bad.item())
    if n_bad:
        _raise_bad(n_bad)
    rec.last_info = {"ranked_clusters": G, "workspace_bytes": ws_bytes}
    return pos


@torch.no_grad()
def condensed_positions(rec, targets, users=None, exclude=None, mask_value: float = -1024.0) -> torch.Tensor:
    """:meth:`gdd.condrank.CondensedRecommender.positions`."""
    from .condrank import mask_rows
    ids = _check_users(users, rec.num_users)
    B = rec.num_users if ids is None else int(ids.shape[0])
    ptr, col, width = _check_targets(targets, B, rec.num_items)
    mask_np = None if exclude is None else mask_rows(exclude, ids, rec.num_users, rec.num_items)
    pos = _cluster_positions(rec, ids, mask_np, mask_value, ptr, col)
    return pos if width is None else pos.view(B, width)


def rank_positions_condensed(cu_z: torch.Tensor, ci_z: torch.Tensor, u2cu, i2ci, targets, users=None,
                             exclude=None, mask_value: float = -1024.0) -> torch.Tensor:
    """What ``rank_positions(cu_z[u2cu], ci_z[i2ci], targets, users, exclude, mask_value)`` returns,
    integer for integer, from the cluster tables and maps alone."""
    from .condrank import CondensedRecommender
    return CondensedRecommender(cu_z, ci_z, u2cu, i2ci).positions(targets, users, exclude, mask_value)


def metrics_from_positions(pos, tg_ptr, deg, topks: Sequence[int]) -> dict:
    """Ranking metrics from the positions of every user's distinct relevant items (host numpy, fp64).
    ``pos``: int positions, CSR rows ``tg_ptr`` (one per user); ``deg``: the relevant count n of every
    user (None: the row length); ``topks``: strictly ascending cut-offs >= 1. Per user with n > 0 and
    cut-off k: ``hits`` = positions below k, precision = hits / k, recall = hits / min(n, k),
    ndcg = DCG / IDCG with weights 1 / log2(pos + 2), DCG added in ascending position from 0 one term
    at a time (the additions of ``gdd_rank_metrics``, so the per-user values are its bits); ``rr`` =
    1 / (best position + 1) and ``mean_rank`` = the mean of pos + 1 over the row. A user with n <= 0
    gets zeros and is not counted. Returns ``per_user`` [B, 3, nk], ``rr`` [B], ``rank`` [B],
    ``precision`` / ``recall`` / ``ndcg`` (means over the counted users, arrays over ``topks``),
    ``mrr``, ``mean_rank`` and ``users``."""
    topks = check_cutoffs(topks)
    if isinstance(pos, torch.Tensor):
        pos = pos.detach().cpu().numpy()
    pos = np.asarray(pos, np.int64).ravel()
    ptr = _np_ids(tg_ptr)
    B = ptr.shape[0] - 1
    if B < 0 or (B >= 0 and (ptr[0] != 0 or ptr[-1] != pos.shape[0] or (np.diff(ptr) < 0).any())):
        raise ValueError("metrics_from_positions: tg_ptr does not describe pos")
    if pos.size and pos.min() < 0:
        raise ValueError("metrics_from_positions: negative position")
    lens = np.diff(ptr)
    n = lens.copy() if deg is None else _np_ids(deg)
    if n.shape[0] != B:
        raise ValueError("metrics_from_positions: deg does not match the number of rows")
    nk = len(topks)
    ks = np.asarray(topks, np.int64)
    per = np.zeros((B, 3, nk))
    rr, rank = np.zeros(B), np.zeros(B)
    counted = n > 0
    top = int(max(ks[-1], 1))
    inv = 1.0 / np.log2(np.arange(top, dtype=np.float64) + 2.0)
    idcg_all = np.cumsum(inv)  # idcg_all[c - 1]: the first c weights, added in order
    row = np.repeat(np.arange(B), lens)
    order = np.lexsort((pos, row))
    spos = pos[order]  # ascending within each row
    maxlen = int(lens.max()) if B else 0
    step = max(1, _BLOCK_ELEMS // max(maxlen, 1))
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        ln = lens[b0:b1]
        w = int(ln.max()) if ln.size else 0
        if w == 0:
            continue
        P = np.full((b1 - b0, w), np.iinfo(np.int64).max, np.int64)
        col = np.arange(ptr[b0], ptr[b1]) - np.repeat(ptr[b0:b1], ln)
        r = row[ptr[b0]:ptr[b1]] - b0
        P[r, col] = spos[ptr[b0]:ptr[b1]]
        W = np.where(P < top, inv[np.minimum(P, top - 1)], 0.0)
        cum = np.cumsum(W, axis=1)  # sequential along the row; the padding adds +0
        nn = n[b0:b1]
        ok = counted[b0:b1]
        for j, k in enumerate(topks):
            hits = (P < k).sum(1)
            cut = np.minimum(np.maximum(nn, 1), k)
            dcg = np.where(hits > 0, cum[np.arange(b1 - b0), np.maximum(hits, 1) - 1], 0.0)
            per[b0:b1, 0, j] = np.where(ok, hits / float(k), 0.0)
            per[b0:b1, 1, j] = np.where(ok, hits / cut.astype(np.float64), 0.0)
            per[b0:b1, 2, j] = np.where(ok, dcg / idcg_all[cut - 1], 0.0)
        has = ok & (ln > 0)
        best = P[:, 0]
        rr[b0:b1] = np.where(has, 1.0 / (np.where(has, best, 0) + 1.0), 0.0)
        tot = (np.where(P < np.iinfo(np.int64).max, P, -1) + 1).sum(1)  # the padding adds 0
        rank[b0:b1] = np.where(has, tot / np.maximum(ln, 1), 0.0)
    count = int(counted.sum())
    means = per[counted].sum(0) / max(count, 1) if B else np.zeros((3, nk))
    return {"per_user": per, "rr": rr, "rank": rank, "precision": means[0].copy(), "recall": means[1].copy(),
            "ndcg": means[2].copy(), "mrr": float(rr[counted].sum() / max(count, 1)),
            "mean_rank": float(rank[counted].sum() / max(count, 1)), "users": count}


class PositionEvaluator:
    """Precision@K, Recall@K, NDCG@K at any cut-offs up to the number of items, MRR and the mean rank
    of the held-out items over an evaluation split: :class:`gdd.rankeval.RankingEvaluator`'s numbers
    (the same evaluated users, mask, relevant items and counts, prepared once by that class) from the
    position of every held-out item instead of a list of 256. Each call is one positions launch, one
    copy of the positions to the host and :func:`metrics_from_positions`; it returns ``precision``,
    ``recall``, ``ndcg`` (float64 arrays over ``topks``), ``mrr``, ``mean_rank`` and ``users``."""

    def __init__(self, train_R, eval_u, eval_i, topks: Sequence[int] = (20,), device="cuda",
                 mask_value: float = -1024.0, count_repeats: bool = True, max_users: Optional[int] = None):
        train_R = sp.csr_matrix(train_R)
        self.topks = check_cutoffs(topks, int(train_R.shape[1]))
        self._prep = RankingEvaluator(train_R, eval_u, eval_i, (1,), device, mask_value, count_repeats, max_users)
        self.num_users, self.num_items = self._prep.num_users, self._prep.num_items
        self.mask_value = float(mask_value)
        self.users = self._prep.users
        self.device = self._prep.device
        self.last: dict = {}  # the last call's full metrics_from_positions result

    def _result(self, pos: torch.Tensor) -> dict:
        _, te_ptr, _, deg = self._prep._host
        m = metrics_from_positions(pos.cpu().numpy(), te_ptr, deg, self.topks)
        self.last = m
        return {k: m[k] for k in ("precision", "recall", "ndcg", "mrr", "mean_rank", "users")}

    def _empty(self) -> dict:
        return {**self._prep._empty(len(self.topks)), "mrr": 0.0, "mean_rank": 0.0}

    @torch.no_grad()
    def positions(self, user_emb: torch.Tensor, item_emb: torch.Tensor) -> torch.Tensor:
        """The positions of the evaluated users' distinct held-out items (CSR order of the split)."""
        nu, ni, _ = _check_tables(user_emb, item_emb)
        self._prep._check_size(nu, ni, "embeddings")
        g = self._prep._prepare()
        bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        pos = _score_positions(user_emb, item_emb, g["users"], g["mask"], self.mask_value, g["te_ptr"],
                               g["te_col"], bad)
        n_bad = int(bad.item())
        if n_bad:
            _raise_bad(n_bad)
        return pos

    @torch.no_grad()
    def __call__(self, user_emb: torch.Tensor, item_emb: torch.Tensor) -> dict:
        if self.users.size == 0:
            _check_tables(user_emb, item_emb)
            return self._empty()
        return self._result(self.positions(user_emb, item_emb))

    @torch.no_grad()
    def condensed(self, cu_z: torch.Tensor, ci_z: torch.Tensor, u2cu, i2ci) -> dict:
        """What ``self(cu_z[u2cu], ci_z[i2ci])`` returns, from the cluster tables
        (``gdd_cluster_positions``: the same positions, so the same numbers)."""
        from .condrank import CondensedRecommender, _distinct_columns
        rec = CondensedRecommender(cu_z, ci_z, u2cu, i2ci)
        self._prep._check_size(rec.num_users, rec.num_items, "cluster maps")
        if self.users.size == 0:
            return self._empty()
        g = self._prep._prepare()
        mask_np = _distinct_columns(*self._prep._host[0])
        return self._result(_cluster_positions(rec, self.users, mask_np, self.mask_value, g["te_ptr"],
                                               g["te_col"]))


def fidelity(teacher_lists, student_positions, topks: Sequence[int]) -> dict:
    """How much of the teacher's ranking the student keeps. ``teacher_lists`` [B, K]: the teacher's
    ranked items, best first; ``student_positions`` [B, K]: the student's position of each of them.
    Per cut-off k <= K: ``overlap`` = the share of the teacher's first k items that the student ranks
    below position k (the size of the intersection of the two top-k sets over k), ``mean_position`` =
    the student's mean position of those k items; both averaged over the users (host fp64). A student
    that ranks as the teacher does gives 1.0 and (k - 1) / 2."""
    to_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)  # noqa: E731
    lists, pos = to_np(teacher_lists), to_np(student_positions)
    if lists.ndim != 2 or pos.shape != lists.shape:
        raise ValueError(f"fidelity: lists of shape {lists.shape} and positions of shape {pos.shape}")
    topks = check_cutoffs(topks, None)
    if topks[-1] > lists.shape[1]:
        raise ValueError(f"topks reach {topks[-1]} but the lists hold {lists.shape[1]} items")
    if pos.size and pos.min() < 0:
        raise ValueError("fidelity: negative position")
    B = lists.shape[0]
    pos = pos.astype(np.int64)
    overlap, mean_pos = np.zeros(len(topks)), np.zeros(len(topks))
    for j, k in enumerate(topks):
        if B:
            overlap[j] = ((pos[:, :k] < k).sum(1) / float(k)).mean()
            mean_pos[j] = pos[:, :k].mean(1).mean()
    return {"overlap": overlap, "mean_position": mean_pos, "users": int(B)}


@torch.no_grad()
def ranking_fidelity(teacher, student, topks: Sequence[int], users=None, exclude=None,
                     mask_value: float = -1024.0) -> dict:
    """:func:`fidelity` of ``student`` against ``teacher = (user_emb, item_emb)``: one teacher
    ``recommend`` of ``max(topks)`` items (at most 256) plus one positions call. ``student`` is
    ``(user_emb, item_emb)`` or a :class:`gdd.condrank.CondensedRecommender` (which goes through
    ``gdd_cluster_positions``); ``users`` / ``exclude`` / ``mask_value`` apply to both."""
    tu, ti = teacher
    topks = check_cutoffs(topks, int(ti.shape[0]))
    lists = recommend(tu, ti, topks[-1], users=users, exclude=exclude, mask_value=mask_value)
    if isinstance(student, tuple):
        pos = rank_positions(student[0], student[1], lists, users=users, exclude=exclude, mask_value=mask_value)
    else:
        pos = student.positions(lists, users=users, exclude=exclude, mask_value=mask_value)
    return fidelity(lists, pos, topks)


def format_full_metrics(topks: Sequence[int], m: dict) -> list:
    """The lines of ``distill_recsys --report_full_ranking``: one per cut-off in the wording of
    :func:`gdd.rankeval.format_metrics`, then MRR and the mean rank."""
    from .rankeval import format_metrics
    return format_metrics(topks, m) + [f"mrr = {m['mrr']:f}, mean rank = {m['mean_rank']:f}"]


def format_fidelity(topks: Sequence[int], f: dict) -> list:
    return [f"overlap@{k:d} = {f['overlap'][i]:f}, mean position of the teacher's top {k:d} = "
            f"{f['mean_position'][i]:f}" for i, k in enumerate(topks)]
