"""The Rankformer and GCN layers as dense definitions in CPU torch (fp64 by default): every sum is
written over the full n x m mask, nothing is linearised. The yardstick the fixture
(tests/golden/rankformer_layer.npz, recorded from the reference layer) and the device layer are
compared against."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rankformer_layer.npz")
CASES = ("small", "wide")  # 37 x 29 x 8 and 61 x 45 x 64


def load_case(name):
    """The fixture's arrays of one case, keys without the case prefix."""
    z = np.load(GOLDEN)
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}


def mask_of(u, i, n, m, dtype=torch.float64):
    M = torch.zeros(n, m, dtype=dtype)
    M[torch.as_tensor(u, dtype=torch.long), torch.as_tensor(i, dtype=torch.long)] = 1
    return M


def dense_rankformer(x, M, alpha=2.0, clamp=0.0):
    """cat(z_u, z_i) for x (n+m, d), users first, and the n x m 0/1 mask M of training pairs."""
    n, m = M.shape
    xh = F.normalize(x)  # eps 1e-12
    xu, xi, vu, vi = xh[:n], xh[n:], x[:n], x[n:]
    N = 1 - M
    dp = M.sum(1, keepdim=True).clamp(min=1)
    dn = (m - M.sum(1, keepdim=True)).clamp(min=1)
    s = xu @ xi.t()
    bp = (M * s).sum(1, keepdim=True) / dp
    bn = (N * s).sum(1, keepdim=True) / dn
    Op = M * (s - bn + alpha) / dp  # Ω⁺ on the pairs, 0 elsewhere
    Om = N * (s - bp - alpha) / dn  # Ω⁻ on the non-pairs
    D = (bp - bn + alpha).clamp(min=clamp)  # the closed form, not the row sums of Ω
    z_u = ((Op + Om) @ vi) / (D + D)
    den_i = Op.sum(0).clamp(min=clamp) + (-Om.sum(0)).clamp(min=clamp)
    z_i = ((Op + Om).t() @ vu) / den_i.unsqueeze(1)
    return torch.cat([z_u, z_i], 0)


def dense_gcn(x, M, left=1.0, right=0.0):
    n, m = M.shape
    du = M.sum(1, keepdim=True).clamp(min=1)
    di = M.sum(0, keepdim=True).clamp(min=1)
    z_u = (M / du.pow(left) / di.pow(right)) @ x[n:]
    z_i = (M / du.pow(right) / di.pow(left)).t() @ x[:n]
    return torch.cat([z_u, z_i], 0)


def planted_blocks(n_users=120, n_items=80, blocks=4, per_user=6, held_out=2, seed=0):
    """The training test's data: every user holds ``per_user`` items of its own block,
    ``held_out`` of them kept for the test split. Returns (train_u, train_i, test_u, test_i)."""
    rng = np.random.RandomState(seed)
    ub, ib = n_users // blocks, n_items // blocks
    tr, te = [], []
    for u in range(n_users):
        b = u // ub
        items = b * ib + rng.choice(ib, per_user, replace=False)
        te += [(u, int(i)) for i in items[:held_out]]
        tr += [(u, int(i)) for i in items[held_out:]]
    tr, te = np.asarray(tr, np.int64), np.asarray(te, np.int64)
    return tr[:, 0], tr[:, 1], te[:, 0], te[:, 1]
