"""The plain numpy side of the gdd.condrank tests: the expanded-table reference (through
tests/rankeval_ref.py) and a model of the completion rule of gdd_cluster_expand_topk, which says
which users of a request must be recomputed against the expanded item table.

The rule, for one user with its L = min(num_ci, 256) best item clusters c_0 .. c_{L-1} in rank order
(descending score, equal scores by ascending cluster id), scores s_0 >= .. >= s_{L-1}, and n_j the
number of unmasked members of c_j that are examined (at most K per cluster): the list is complete if
L == num_ci, or if for some j <= L-1 the members of c_0 .. c_j scoring strictly above s_{j+1} number
at least K, where s_L := s_{L-1} (an unseen cluster may tie the last seen one)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from rankeval_ref import csr_of, grid, ranked, scores64, take_rows  # noqa: E402,F401

MAX_LIST = 256


def rule_incomplete(scores, counts, k, num_ci):
    """True if the rule leaves the list open. ``scores``: the L ranked clusters' scores, descending;
    ``counts``: their unmasked member counts."""
    s = np.asarray(scores, np.float64)
    n = np.minimum(np.asarray(counts, np.int64), k)
    L = s.shape[0]
    if L == num_ci:
        return False
    for j in range(L):
        nxt = s[j + 1] if j + 1 < L else s[L - 1]
        if int(n[:j + 1][s[:j + 1] > nxt].sum()) >= k:
            return False
    return True


def membership(i2ci, num_ci):
    """The members of every cluster in ascending item id, as a list of arrays."""
    i2ci = np.asarray(i2ci)
    return [np.nonzero(i2ci == c)[0] for c in range(num_ci)]


def must_fall_back(cu_z, ci_z, u2cu, i2ci, k, users=None, mask=None):
    """bool [B]: the users of the request that the rule leaves open. ``mask``: (ptr, col) with one
    row per selected user. Cluster scores in fp64: exact for grid tables."""
    cu_z, ci_z = np.asarray(cu_z, np.float64), np.asarray(ci_z, np.float64)
    u2cu = np.asarray(u2cu)
    num_ci = ci_z.shape[0]
    L = min(num_ci, MAX_LIST)
    sel = np.arange(u2cu.shape[0]) if users is None else np.asarray(users)
    mem = membership(i2ci, num_ci)
    out = np.zeros(sel.shape[0], bool)
    for b, u in enumerate(sel):
        s = cu_z[u2cu[u]] @ ci_z.T
        order = np.argsort(-s, kind="stable")[:L]
        row = mask[1][mask[0][b]:mask[0][b + 1]] if mask is not None else np.zeros(0, np.int64)
        counts = [int((~np.isin(mem[c], row)).sum()) for c in order]
        out[b] = rule_incomplete(s[order], counts, k, num_ci)
    return out


def expanded_reference(cu_z, ci_z, u2cu, i2ci, k, users=None, mask=None, mask_value=-1024.0):
    """(items, scores fp64) of the expanded tables by the plain definition."""
    U, V = np.asarray(cu_z)[np.asarray(u2cu)], np.asarray(ci_z)[np.asarray(i2ci)]
    sel = np.arange(U.shape[0]) if users is None else np.asarray(users)
    return ranked(scores64(U, V, sel, mask, mask_value), k)
