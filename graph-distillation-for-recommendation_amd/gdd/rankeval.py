"""Ranked top-K lists and ranking metrics on MI355X (Rankformer/code/model.py:252-343 ``evaluate``,
:27-53 ``test``; main.py:100-120 selects the teacher's epoch on them).

* :func:`recommend` — the ``k`` best items per user in rank order (``gdd_score_topk``): scores are
  computed tile by tile and never written to memory, a masked item (``exclude``) scores
  ``mask_value`` instead of being removed (model.py:313), equal scores rank in ascending item id;
* :func:`rank_metrics` — precision, recall and NDCG at several cut-offs from ranked lists
  (``gdd_rank_metrics``), fp64, per user and summed in a fixed order;
* :class:`RankingEvaluator` — both with the host preparation done once, the counterpart of
  :class:`gdd.recsys.RecallEvaluator` for the reference teacher's three metrics. Recall here is
  ``hits / min(n, k)`` averaged over users (model.py:43-47), not the driver's micro
  ``hits / total``. ``RankingEvaluator.condensed`` evaluates a condensed model from its cluster
  tables (:mod:`gdd.condrank`): the same lists, so the same numbers.

Argument errors raise ``ValueError`` before the device is touched. There is no CPU path.
"""
from __future__ import annotations

import ast
from typing import Optional, Sequence, Tuple

import numpy as np
import scipy.sparse as sp
import torch

from . import _lib

MAX_K = 256  # gdd_score_topk: the append buffer of one user is at most 512 keys of LDS
MAX_DIM = 256  # gdd_rank_max_dim()
MAX_TOPKS = 8  # gdd_rank_metrics: one lane per cut-off


def _parse_int_list(text) -> list:
    """``"[20, 50]"``, ``"20"`` or the value itself as a list or tuple of integers
    (``ast.literal_eval``; the reference uses ``eval``, parse.py:85)."""
    v = ast.literal_eval(text) if isinstance(text, str) else text
    if isinstance(v, (int, np.integer)) and not isinstance(v, bool):
        v = [v]
    if not isinstance(v, (list, tuple)) or any(isinstance(k, bool) or not isinstance(k, (int, np.integer))
                                                for k in v):
        raise ValueError(f"topks must be a list of integers, got {text!r}")
    return v


def parse_topks(text) -> Tuple[int, ...]:
    """``--topks "[20, 50]"`` as a tuple of ints."""
    return check_topks(_parse_int_list(text))


def check_topks(topks, num_items: Optional[int] = None) -> Tuple[int, ...]:
    t = tuple(int(k) for k in topks)
    if not 1 <= len(t) <= MAX_TOPKS:
        raise ValueError(f"topks must hold 1 to {MAX_TOPKS} cut-offs, got {len(t)}")
    if t[0] < 1 or any(b <= a for a, b in zip(t, t[1:])):
        raise ValueError(f"topks must be strictly ascending positive integers, got {list(t)}")
    _check_k(t[-1], num_items)
    return t


def _check_k(k: int, num_items: Optional[int]) -> int:
    k = int(k)
    if k < 1 or k > MAX_K:
        raise ValueError(f"k = {k} outside [1, {MAX_K}]")
    if num_items is not None and k > int(num_items):
        raise ValueError(f"k = {k} exceeds the number of items ({int(num_items)})")
    return k


def _check_tables(user_emb, item_emb) -> Tuple[int, int, int]:
    if user_emb.dim() != 2 or item_emb.dim() != 2 or user_emb.shape[1] != item_emb.shape[1]:
        raise ValueError(f"user and item embeddings differ in width: {tuple(user_emb.shape)} vs "
                         f"{tuple(item_emb.shape)}")
    d = int(user_emb.shape[1])
    if d < 1 or d > MAX_DIM:
        raise ValueError(f"embedding width {d} outside [1, {MAX_DIM}]")
    if int(item_emb.shape[0]) >= 2 ** 31 or int(user_emb.shape[0]) >= 2 ** 31:
        raise ValueError("tables outside int32 row ids")
    return int(user_emb.shape[0]), int(item_emb.shape[0]), d


def _np_ids(a) -> np.ndarray:
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.int64).ravel()


def _check_users(users, num_users: int) -> Optional[np.ndarray]:
    if users is None:
        return None
    ids = _np_ids(users)
    if ids.size and (ids.min() < 0 or ids.max() >= num_users):
        raise ValueError(f"users holds an id outside [0, {num_users})")
    return ids


def _gather_rows(ptr: np.ndarray, col: np.ndarray, users: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """The rows ``users`` of the CSR ``(ptr, col)`` in that order, columns as stored: ``(int32 ptr,
    col)``."""
    ptr = np.asarray(ptr, np.int64)
    if users.size and (users.min() < 0 or users.max() >= ptr.shape[0] - 1):
        raise ValueError("exclude has no row for some selected user")
    lens = ptr[users + 1] - ptr[users]
    out_ptr = np.zeros(users.shape[0] + 1, np.int64)
    np.cumsum(lens, out=out_ptr[1:])
    if out_ptr[-1] >= 2 ** 31:
        raise ValueError("exclude rows outside int32")
    gather = np.repeat(ptr[users] - out_ptr[:-1], lens) + np.arange(out_ptr[-1])
    return out_ptr.astype(np.int32), col[gather]


def _rows_of(exclude, users: np.ndarray, num_items: int) -> Tuple[np.ndarray, np.ndarray]:
    """The rows ``users`` of ``exclude`` (scipy sparse, or ``(ptr, col)`` over all users) as an int32
    CSR in the order of ``users``, columns ascending."""
    if sp.issparse(exclude):
        m = sp.csr_matrix(exclude)
        ptr, col = m.indptr, np.asarray(m.indices, np.int64)
    else:
        ptr, col = (_np_ids(x) for x in exclude)
    out_ptr, c = _gather_rows(ptr, col, users)
    row = np.repeat(np.arange(users.shape[0]), np.diff(out_ptr))
    c = c[np.lexsort((c, row))]  # rows stay in place, each sorted by column
    return out_ptr, c.astype(np.int32)


def _f32(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to(torch.float32).contiguous()


def _to_dev(a, dev, dtype=None) -> torch.Tensor:
    """A host array (as ``dtype``, if given) or a tensor on ``dev``."""
    if isinstance(a, torch.Tensor):
        return a.to(dev)
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)


def _score_topk(user_emb, item_emb, k, users_t, mask, mask_value, return_scores, bad):
    """One ``gdd_score_topk`` launch. ``users_t``: int32 device ids or None; ``mask``: (ptr, col)
    int32 device tensors or None; ``bad``: int32 device counter."""
    lib = _lib.device_lib()
    U, V = _f32(user_emb), _f32(item_emb)
    dev = V.device
    B = int(users_t.numel()) if users_t is not None else int(U.shape[0])
    items = torch.empty(B, k, dtype=torch.int32, device=dev)
    scores = torch.empty(B, k, dtype=torch.float32, device=dev) if return_scores else None
    mp, mc = mask if mask is not None and int(mask[1].numel()) else (None, None)  # no entry: no mask
    _lib.check(lib.gdd_score_topk(B, int(V.shape[0]), int(V.shape[1]), k, _lib.ptr(users_t), U.data_ptr(),
                                  int(U.shape[0]), V.data_ptr(), _lib.ptr(mp), _lib.ptr(mc), float(mask_value),
                                  items.data_ptr(), _lib.ptr(scores), bad.data_ptr(), _lib.stream_ptr(dev)))
    return items, scores


def _raise_bad(n: int) -> None:
    raise RuntimeError(f"gdd_score_topk: {n} row(s) with a user id or an excluded item id out of range "
                       "(those rows are -1)")


def recommend(user_emb: torch.Tensor, item_emb: torch.Tensor, k: int, users=None, exclude=None,
              mask_value: float = -1024.0, return_scores: bool = False):
    """The ``k`` highest-scoring items of each user, best first: int32 ``[B, k]`` on the device (and the
    fp32 scores with ``return_scores``). ``users``: ids into ``user_emb`` (default: every row, in
    order; repeats allowed). ``exclude``: a scipy sparse matrix or ``(ptr, col)`` CSR over all users,
    e.g. the training interactions; an excluded item scores ``mask_value``, so it can still fill the
    tail of a list longer than the user's other items. Scores are fp32 fma chains over the features
    in ascending order; equal scores rank in ascending item id."""
    nu, ni, _ = _check_tables(user_emb, item_emb)
    k = _check_k(k, ni)
    ids = _check_users(users, nu)
    mask_np = None
    if exclude is not None:
        # item ids are checked by the kernel (a row with one outside [0, I) comes back as -1)
        mask_np = _rows_of(exclude, ids if ids is not None else np.arange(nu), ni)
    dev = item_emb.device
    _lib.device_lib()
    users_t = None if ids is None else _to_dev(ids, dev, np.int32)
    mask = None if mask_np is None else tuple(_to_dev(a, dev) for a in mask_np)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    items, scores = _score_topk(user_emb, item_emb, k, users_t, mask, mask_value, return_scores, bad)
    n_bad = int(bad.item())
    if n_bad:
        _raise_bad(n_bad)
    return (items, scores) if return_scores else items


def rank_metrics(top_item: torch.Tensor, te_ptr: torch.Tensor, te_col: torch.Tensor,
                 te_deg: Optional[torch.Tensor], topks: Sequence[int], out: Optional[torch.Tensor] = None):
    """``gdd_rank_metrics`` on ranked lists (int32 ``[B, K]``, device): ``te_ptr`` / ``te_col`` the
    users' sorted distinct relevant items (int32 CSR, B rows), ``te_deg`` (int32, optional) the
    relevant count n of each user where it differs from the row length. Returns ``(per_user, sums,
    count)``: float64 ``[B, 3, nk]`` (precision, recall, ndcg), their sums over users ``[3, nk]`` and
    the number of users with n > 0 (a one-element int64 tensor), all on the device. ``out``: a
    float64 device buffer of at least ``3 nk + 1`` elements that receives sums and count."""
    B, K = int(top_item.shape[0]), int(top_item.shape[1])
    topks = check_topks(topks)
    if topks[-1] > K:
        raise ValueError(f"topks reach {topks[-1]} but the lists hold {K} items")
    nk = len(topks)
    if int(te_ptr.numel()) != B + 1 or (te_deg is not None and int(te_deg.numel()) != B):
        raise ValueError("rank_metrics: te_ptr / te_deg do not match the number of lists")
    lib = _lib.device_lib()
    dev = top_item.device
    tk = torch.tensor(topks, dtype=torch.int32).to(dev)
    inv = torch.from_numpy(1.0 / np.log2(np.arange(K, dtype=np.float64) + 2.0)).to(dev)
    return _rank_metrics(lib, top_item.contiguous(), te_ptr, te_col, te_deg, tk, inv, nk, out)


def _rank_metrics(lib, top_item, te_ptr, te_col, te_deg, tk, inv, nk, out):
    B, K = int(top_item.shape[0]), int(top_item.shape[1])
    dev = top_item.device
    per_user = torch.empty(B, 3, nk, dtype=torch.float64, device=dev)
    if out is None:
        out = torch.empty(3 * nk + 1, dtype=torch.float64, device=dev)
    sums, count = out[:3 * nk].view(3, nk), out[3 * nk:3 * nk + 1].view(torch.int64)
    _lib.check(lib.gdd_rank_metrics(B, K, top_item.data_ptr(), te_ptr.data_ptr(), _lib.ptr(te_col),
                                    _lib.ptr(te_deg), nk, tk.data_ptr(), inv.data_ptr(), per_user.data_ptr(),
                                    sums.data_ptr(), count.data_ptr(), _lib.stream_ptr(dev)))
    return per_user, sums, count


class RankingEvaluator:
    """Precision@K, Recall@K and NDCG@K of (user, item) embeddings over an evaluation split, as
    model.py:252-343 computes them, with the host preparation done once: the evaluated users (the
    sorted users of the split, the first ``max_users`` of them if given; a user without an item in
    the split counts for nothing in the reference either), their training items as the mask, their
    distinct evaluation items, and their relevant counts n. ``count_repeats`` (default) takes n as
    the reference does, the user's number of lines in the split, repeated lines included
    (dataloader.py:65-70); otherwise n is the number of distinct items.

    Each call is one ``gdd_score_topk`` launch, one ``gdd_rank_metrics`` call and one small copy to
    the host; it returns ``{"precision", "recall", "ndcg"}`` as float64 arrays over ``topks`` (means
    over the counted users) and ``"users"``, their number."""

    def __init__(self, train_R, eval_u, eval_i, topks: Sequence[int] = (20,), device="cuda",
                 mask_value: float = -1024.0, count_repeats: bool = True, max_users: Optional[int] = None):
        train_R = sp.csr_matrix(train_R)
        self.num_users, self.num_items = int(train_R.shape[0]), int(train_R.shape[1])
        self.topks = check_topks(topks, self.num_items)
        self.k = self.topks[-1]
        self.mask_value = float(mask_value)
        eu, ei = _np_ids(eval_u), _np_ids(eval_i)
        if eu.shape != ei.shape:
            raise ValueError("eval_u and eval_i differ in length")
        if eu.size and (eu.min() < 0 or eu.max() >= self.num_users or ei.min() < 0 or ei.max() >= self.num_items):
            raise ValueError("the evaluation split holds an id outside the interaction matrix")
        users = np.unique(eu)
        if max_users is not None and users.size > int(max_users):
            users = users[:int(max_users)]
        keep = np.isin(eu, users)
        eu, ei = eu[keep], ei[keep]
        pairs = np.unique(np.stack([eu, ei], 1), axis=0) if eu.size else np.zeros((0, 2), np.int64)
        edge = np.concatenate([users, [np.iinfo(np.int64).max]])
        te_ptr = np.searchsorted(pairs[:, 0], edge)
        lines = np.searchsorted(np.sort(eu), edge)
        deg = np.diff(lines) if count_repeats else np.diff(te_ptr)
        self.users = users
        self._host = (_rows_of(train_R, users, self.num_items), te_ptr.astype(np.int32),
                      pairs[:, 1].astype(np.int32), deg.astype(np.int32))
        self.device = torch.device(device)
        self._dev = None

    def _prepare(self):
        if self._dev is None:
            _lib.device_lib()
            dev = self.device
            (mp, mc), te_ptr, te_col, deg = self._host
            t = lambda a, dt=None: _to_dev(a, dev, dt)  # noqa: E731
            nk = len(self.topks)
            self._dev = dict(users=t(self.users, np.int32), mask=(t(mp), t(mc)), te_ptr=t(te_ptr),
                             te_col=t(te_col), deg=t(deg), tk=t(self.topks, np.int32),
                             inv=t(1.0 / np.log2(np.arange(self.k, dtype=np.float64) + 2.0)),
                             out=torch.zeros(3 * nk + 2, dtype=torch.float64, device=dev))
        return self._dev

    def _check_size(self, num_users: int, num_items: int, what: str) -> None:
        if num_users != self.num_users or num_items != self.num_items:
            raise ValueError(f"{what} of {num_users} users x {num_items} items for an evaluator of "
                             f"{self.num_users} x {self.num_items}")

    def _empty(self, nk: Optional[int] = None) -> dict:
        """The result over no users (``nk`` cut-offs, default: this evaluator's)."""
        z = np.zeros(len(self.topks) if nk is None else nk)
        return {"precision": z.copy(), "recall": z.copy(), "ndcg": z.copy(), "users": 0}

    def _metrics(self, items: torch.Tensor) -> torch.Tensor:
        """``gdd_rank_metrics`` on the evaluated users' lists; the host copy of ``out``: sums, count and
        the bad-row counter in one copy."""
        g = self._dev
        _rank_metrics(_lib.device_lib(), items, g["te_ptr"], g["te_col"], g["deg"], g["tk"], g["inv"],
                      len(self.topks), g["out"])
        return g["out"].cpu()

    def _means(self, host: torch.Tensor) -> dict:
        nk = len(self.topks)
        count = int(host[3 * nk:3 * nk + 1].view(torch.int64)[0])
        means = host[:3 * nk].view(3, nk).numpy() / max(count, 1)
        return {"precision": means[0].copy(), "recall": means[1].copy(), "ndcg": means[2].copy(),
                "users": count}

    def _lists(self, user_emb, item_emb, return_scores=False):
        nu, ni, _ = _check_tables(user_emb, item_emb)
        self._check_size(nu, ni, "embeddings")
        g = self._prepare()
        bad = g["out"][-1:].view(torch.int32)[:1]
        return _score_topk(user_emb, item_emb, self.k, g["users"], g["mask"], self.mask_value, return_scores,
                           bad)

    @torch.no_grad()
    def ranked(self, user_emb: torch.Tensor, item_emb: torch.Tensor, return_scores: bool = False):
        """The ranked lists of the evaluated users (``self.users``): int32 ``[B, max(topks)]``."""
        items, scores = self._lists(user_emb, item_emb, return_scores)
        n_bad = int(self._dev["out"][-1:].view(torch.int32)[0].item())
        if n_bad:
            self._dev["out"][-1:].zero_()
            _raise_bad(n_bad)
        return (items, scores) if return_scores else items

    @torch.no_grad()
    def __call__(self, user_emb: torch.Tensor, item_emb: torch.Tensor) -> dict:
        if self.users.size == 0:
            return self._empty()
        items, _ = self._lists(user_emb, item_emb)
        host = self._metrics(items)
        n_bad = int(host[-1:].view(torch.int32)[0])
        if n_bad:
            self._dev["out"][-1:].zero_()
            _raise_bad(n_bad)
        return self._means(host)

    @torch.no_grad()
    def condensed(self, cu_z: torch.Tensor, ci_z: torch.Tensor, u2cu, i2ci) -> dict:
        """What ``self(cu_z[u2cu], ci_z[i2ci])`` returns, from the condensed model itself: the lists of
        :class:`gdd.condrank.CondensedRecommender` (the same items, so the same metrics) and
        ``gdd_rank_metrics``."""
        from .condrank import CondensedRecommender, _distinct_columns
        rec = CondensedRecommender(cu_z, ci_z, u2cu, i2ci)
        self._check_size(rec.num_users, rec.num_items, "cluster maps")
        if self.users.size == 0:
            return self._empty()
        self._prepare()
        items, _ = rec._lists(self.k, self.users, _distinct_columns(*self._host[0]), self.mask_value, False)
        return self._means(self._metrics(items))  # rec._lists has its own bad-row counter


def format_metrics(topks: Sequence[int], m: dict) -> list:
    """One line per cut-off in the reference's wording (main.py:46, :108)."""
    return [f"ndcg@{k:d} = {m['ndcg'][i]:f}, recall@{k:d} = {m['recall'][i]:f}, pre@{k:d} = {m['precision'][i]:f}"
            for i, k in enumerate(topks)]
