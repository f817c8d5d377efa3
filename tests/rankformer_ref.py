"""The Rankformer and GCN layers as dense definitions in CPU torch (fp64 by default): every sum is
written over the full n x m mask, nothing is linearised. The yardstick the fixture
(tests/golden/rankformer_layer.npz, recorded from the reference layer) and the device layer are
compared against.

Also here: the second fixture's loader (tests/golden/rankformer_layer_more.npz: the clamp settings,
the cut-row case, d = 193 and two stacked layers), the three denominators the clamp acts on, the two
row passes as plain gather / multiply / ``index_add_`` definitions for fp64 autograd, and the
graph and row-length patterns the edge tests share."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rankformer_layer.npz")
GOLDEN_MORE = os.path.join(os.path.dirname(GOLDEN), "rankformer_layer_more.npz")
CASES = ("small", "wide")  # 37 x 29 x 8 and 61 x 45 x 64
# the second fixture: case -> (case whose pairs it runs on, alpha, clamp, layers)
MORE_CASES = {
    "small_c05": ("small", 0.5, 0.6, 1), "small_c025": ("small", 0.25, 0.3, 1),
    "wide_c05": ("wide", 0.5, 0.6, 1), "wide_c025": ("wide", 0.25, 0.3, 1),
    "cut": ("cut", 2.0, 0.0, 1), "cut_c05": ("cut", 0.5, 0.6, 1),  # 100 x 80 x 65
    "small193": ("small", 2.0, 0.0, 1),  # its own x of width 193
    "stack2": ("small", 2.0, 0.0, 2),  # x <- (1 - tau) x + tau layer(x), twice, tau = 0.5
}
TAU = 0.5


def load_case(name):
    """The fixture's arrays of one case, keys without the case prefix."""
    z = np.load(GOLDEN)
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "_")}


def load_more_case(name):
    """One case of the second fixture: its own arrays, and what it does not store (the pairs, ``x``
    and ``W`` of the case it runs on) from that case; ``x`` and ``W`` as fp64 (stored as fp32)."""
    base, alpha, clamp, layers = MORE_CASES[name]
    z = np.load(GOLDEN_MORE)
    c = {k: v for k, v in load_case(base).items() if k in ("n", "m", "u", "i", "x", "W")} if base in CASES else {}
    for src in (base, name):  # keys are "<case>.<field>"
        c.update({k[len(src) + 1:]: z[k] for k in z.files if k.startswith(src + ".")})
    c["x"], c["W"] = c["x"].astype(np.float64), c["W"].astype(np.float64)
    assert (float(c["alpha"]), float(c["clamp"]), int(c["layers"])) == (alpha, clamp, layers)
    c.update(name=name, alpha=alpha, clamp=clamp, layers=layers)
    return c


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


def dense_rankformer_terms(x, M, alpha=2.0, clamp=0.0):
    """Σ|terms| of the layer's two final sums, per output element: Σ_j |Ω_uj| |v_j| / (2 D_u) and
    Σ_u |Ω_ui| |v_u| / den_i, with Ω, D and den exact (the magnitude a forward bound scales with)."""
    n, m = M.shape
    xh = F.normalize(x)
    xu, xi, vu, vi = xh[:n], xh[n:], x[:n], x[n:]
    N = 1 - M
    dp = M.sum(1, keepdim=True).clamp(min=1)
    dn = (m - M.sum(1, keepdim=True)).clamp(min=1)
    s = xu @ xi.t()
    bp = (M * s).sum(1, keepdim=True) / dp
    bn = (N * s).sum(1, keepdim=True) / dn
    Op, Om = M * (s - bn + alpha) / dp, N * (s - bp - alpha) / dn
    D = (bp - bn + alpha).clamp(min=clamp)
    den_i = Op.sum(0).clamp(min=clamp) + (-Om.sum(0)).clamp(min=clamp)
    Oabs = (Op + Om).abs()
    return torch.cat([(Oabs @ vi.abs()) / (D + D), (Oabs.t() @ vu.abs()) / den_i.unsqueeze(1)], 0)


def dense_stack(x, M, alpha=2.0, clamp=0.0, layers=1, tau=TAU):
    """``layers == 1``: the layer itself; more: the model's blend x <- (1 - tau) x + tau layer(x)."""
    if layers == 1:
        return dense_rankformer(x, M, alpha, clamp)
    for _ in range(layers):
        x = (1 - tau) * x + tau * dense_rankformer(x, M, alpha, clamp)
    return x


def dense_denominators(x, M, alpha):
    """The three quantities the layer clamps, before the clamp: D_u [n], the items' sum of Ω⁺ [m] and
    minus their sum of Ω⁻ [m] (the same expressions as in :func:`dense_rankformer`)."""
    n, m = M.shape
    xh = F.normalize(x)
    N = 1 - M
    dp = M.sum(1, keepdim=True).clamp(min=1)
    dn = (m - M.sum(1, keepdim=True)).clamp(min=1)
    s = xh[:n] @ xh[n:].t()
    bp = (M * s).sum(1, keepdim=True) / dp
    bn = (N * s).sum(1, keepdim=True) / dn
    return ((bp - bn + alpha)[:, 0], (M * (s - bn + alpha) / dp).sum(0), -(N * (s - bp - alpha) / dn).sum(0))


def clamp_conditions(x, M, alpha, clamp):
    """What keeps a clamp test honest: per denominator (rows clamped, rows in all), and the smallest
    distance of any denominator to the clamp value (a kink closer than the fp32 error of a
    denominator would make the fp32 and fp64 gradients differ legitimately)."""
    dens = dense_denominators(x, M, alpha)
    counts = [(int((t < clamp).sum()), int(t.numel())) for t in dens]
    return counts, min(float((t - clamp).abs().min()) for t in dens)


# ---- the two row passes as plain definitions (gather, multiply, index_add_) for fp64 autograd ----
def plain_rowpass(rows, col, n_rows, Q, K, V):
    """(s, s_sum, SK, SV, A) of ``gdd_rank_rowpass`` for the entries (rows[e], col[e])."""
    k, v = K[col], V[col]
    s = (Q[rows] * k).sum(1)
    zero = torch.zeros(n_rows, Q.shape[1], dtype=Q.dtype)
    return (s, torch.zeros(n_rows, dtype=Q.dtype).index_add_(0, rows, s), zero.clone().index_add_(0, rows, k),
            zero.clone().index_add_(0, rows, v), zero.clone().index_add_(0, rows, s.unsqueeze(1) * v))


def plain_wsum(rows, col, n_rows, w, V, a=None, b=None):
    """(Y, ta, tb) of ``gdd_rank_wsum``; ta / tb are None without a / b."""
    Y = torch.zeros(n_rows, V.shape[1], dtype=V.dtype).index_add_(0, rows, w.unsqueeze(1) * V[col])
    ta = None if a is None else torch.zeros(n_rows, dtype=V.dtype).index_add_(0, rows, a)
    tb = None if b is None else torch.zeros(n_rows, dtype=V.dtype).index_add_(0, rows, b)
    return Y, ta, tb


def autograd_pairs(n=70, m=40, density=0.15, seed=21):
    """The autograd tests' graph: column 0 held by every row (a transposed row of 70 entries, cut
    into three chunks), row 3 holding every column but the empty one, row 5 empty, column 7 empty."""
    rng = np.random.RandomState(seed)
    M = rng.random_sample((n, m)) < density
    M[:, 0] = True
    M[3, :] = True
    M[5, :] = False
    M[:, 7] = False
    u, i = np.nonzero(M)
    return u.astype(np.int64), i.astype(np.int64), n, m


# row lengths against the kernels' chunk of 32 consecutive entries (tests of the chunk geometry)
PATTERNS = [
    [0, 0, 0, 0, 0],  # no entry at all: only the fix-up launch runs
    [0, 0, 1, 0],
    [31],
    [32],
    [33],
    [32, 32, 32],  # every row boundary on a chunk boundary
    [64, 0, 32],  # a row of two whole chunks, an empty row on the boundary
    [16, 48, 0, 0, 32],  # starts mid-chunk, ends on a boundary, empties on the boundary
    [32, 40, 24],
    [20, 20, 5, 30],  # a chunk holding three rows, cut at both ends
    [100],  # middle chunks wholly inside the one row
    [0] * 40 + [3] + [0] * 40 + [70] + [0] * 3,
]


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
