"""The plain numpy side of the gdd.rankpos tests.

* ``ord32`` / ``positions``: the definition. ``pos(b, t)`` counts the items whose key is above the
  target's, the key being (score word, then ascending item id) with the score word of
  ``score_key`` (gdd_common.hpp): the fp32 bits made orderable, so +0 ranks above -0. ``S`` holds
  fp32 scores with the mask already applied; for grid tables (tests/rankeval_ref.py ``grid``) the
  fp64 product cast to fp32 is exact, so ``positions`` is the reference of the device kernels.
* ``cluster_positions``: a model of the formula of ``gdd_cluster_positions`` (DESIGN.md "Full-ranking
  positions"): cluster sizes above the target's score word, members below the target inside tied
  clusters, and one correction per masked item. tests/test_rankpos_host.py holds it against
  ``positions`` on the expanded tables.
* ``direct_metrics``: MRR and mean rank straight from the positions.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rankeval_ref import csr_of, grid, ranked, scores64, take_rows  # noqa: E402,F401


def ord32(x):
    """The high word of score_key: larger float -> larger word, +0 above -0."""
    b = np.ascontiguousarray(np.asarray(x, np.float32)).view(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def positions(S, tg_ptr, tg_col):
    """int32 positions of the targets (CSR, one row per row of ``S``) under fp32 scores ``S``."""
    o = ord32(S).astype(np.int64)
    B, n_items = o.shape
    ids = np.arange(n_items)
    out = np.zeros(len(tg_col), np.int32)
    for b in range(B):
        t = np.asarray(tg_col[tg_ptr[b]:tg_ptr[b + 1]], np.int64)
        if t.size == 0:
            continue
        ot = o[b, t][:, None]
        above = (o[b][None, :] > ot) | ((o[b][None, :] == ot) & (ids[None, :] < t[:, None]))
        out[tg_ptr[b]:tg_ptr[b + 1]] = above.sum(1)
    return out


def masked_scores32(U, V, users=None, mask=None, mask_value=-1024.0):
    """fp32 scores [B, I] of grid tables (exact), the mask rows set to fp32(mask_value) (its sign kept)."""
    S = (scores64(U, V, users, None) + 0.0).astype(np.float32)  # the chain starts from +0: never -0
    if mask is not None:
        ptr, col = mask
        for b in range(S.shape[0]):
            S[b, col[ptr[b]:ptr[b + 1]]] = np.float32(mask_value)
    return S


def cluster_positions(cu_z, ci_z, u2cu, i2ci, tg_ptr, tg_col, users=None, mask=None, mask_value=-1024.0):
    """The formula of gdd_cluster_positions; cluster scores in fp64 cast to fp32 (exact on a grid)."""
    cu_z, ci_z = np.asarray(cu_z, np.float64), np.asarray(ci_z, np.float64)
    u2cu, i2ci = np.asarray(u2cu), np.asarray(i2ci)
    num_ci = ci_z.shape[0]
    sel = np.arange(u2cu.shape[0]) if users is None else np.asarray(users)
    mem = [np.nonzero(i2ci == c)[0] for c in range(num_ci)]
    size = np.array([m.shape[0] for m in mem], np.int64)
    omv = int(ord32([mask_value])[0])
    out = np.zeros(len(tg_col), np.int32)
    for b, u in enumerate(sel):
        o = ord32((cu_z[u2cu[u]] @ ci_z.T + 0.0).astype(np.float32)).astype(np.int64)
        row = np.asarray(mask[1][mask[0][b]:mask[0][b + 1]], np.int64) if mask is not None else np.zeros(0, np.int64)
        for e in range(tg_ptr[b], tg_ptr[b + 1]):
            t = int(tg_col[e])
            ot = omv if t in row else int(o[i2ci[t]])
            pos = int(size[o > ot].sum())
            for c in np.nonzero(o == ot)[0]:
                pos += int(np.searchsorted(mem[c], t))
            om = o[i2ci[row]]
            as_masked = (omv > ot) | ((omv == ot) & (row < t))
            as_member = (om > ot) | ((om == ot) & (row < t))
            pos += int(as_masked.sum()) - int(as_member.sum())
            out[e] = pos
    return out


def direct_metrics(pos, tg_ptr, deg):
    """(mrr, mean_rank, count): per counted user (deg > 0) 1 / (best position + 1) and the mean of
    position + 1 over its row, averaged over the counted users."""
    rr, rk, count = [], [], 0
    for b in range(len(tg_ptr) - 1):
        if deg[b] <= 0:
            continue
        count += 1
        p = np.asarray(pos[tg_ptr[b]:tg_ptr[b + 1]], np.float64)
        rr.append(1.0 / (p.min() + 1.0) if p.size else 0.0)
        rk.append((p + 1.0).mean() if p.size else 0.0)
    return float(np.sum(rr) / max(count, 1)), float(np.sum(rk) / max(count, 1)), count
