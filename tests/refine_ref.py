"""An fp64 restatement of the refinement epoch's loss (the LightGCN forward over the condensed graph,
the softplus BPR loss, its three regularisers and the KD term) in plain torch on the CPU, with
``index_add_`` scatters and autograd for the gradients: the yardstick of tests/test_gpu_refine.py and
tests/test_gpu_refine_forms.py. Also the seeded inputs of the former's edge cases, ``manual_adam_step``
in fp64, and the error measure of the latter with its per-case bound (``references``)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import refine_cases

NAMES = ("user_emb.weight", "item_emb.weight", "user_delta", "item_delta", "edge_logit")


DROPS = ("reg", "delta", "weight", "kd")  # the sampled rows', the deltas' and the weights' regulariser, KD


def loss_and_grads(params, edge_index, num_layers, u, pos_i, neg_i, reg_lambda, teacher=None, kd_lambda=0.01,
                   dtype=torch.float64, drop=None, reverse=False):
    """``params``: {name: array} (any float dtype); returns (loss, {name: gradient}) computed in ``dtype``.
    ``drop``: one of DROPS, the loss term to leave out. ``reverse``: the edges and the triplets reach the
    ``index_add_`` scatters and the sums last first (the CPU scatter adds in the order given: a second
    summation order in fp32, the same value in exact arithmetic)."""
    if drop is not None and drop not in DROPS:
        raise ValueError(f"drop must be one of {DROPS}")
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in params.items()}
    ue, ie, ud, idl, logit = (p[n] for n in NAMES)
    cu, ci = (torch.as_tensor(np.asarray(a), dtype=torch.int64) for a in edge_index)
    u, pos_i, neg_i = (torch.as_tensor(np.asarray(a), dtype=torch.int64) for a in (u, pos_i, neg_i))
    if reverse:
        cu, ci, logit = cu.flip(0), ci.flip(0), logit.flip(0)
        u, pos_i, neg_i = u.flip(0), pos_i.flip(0), neg_i.flip(0)
    num_cu, num_ci = ue.shape[0], ie.shape[0]
    w = F.softplus(logit) + 1e-8
    deg_u = torch.zeros(num_cu, dtype=dtype).index_add_(0, cu, w)
    deg_i = torch.zeros(num_ci, dtype=dtype).index_add_(0, ci, w)
    norm = w / (torch.sqrt(deg_u[cu] + 1e-8) * torch.sqrt(deg_i[ci] + 1e-8))
    x_u, x_i = ue + ud, ie + idl
    sum_u, sum_i = x_u, x_i
    for _ in range(int(num_layers)):
        nxt_u = torch.zeros_like(x_u).index_add_(0, cu, x_i[ci] * norm[:, None])
        nxt_i = torch.zeros_like(x_i).index_add_(0, ci, x_u[cu] * norm[:, None])
        x_u, x_i = nxt_u, nxt_i
        sum_u, sum_i = sum_u + x_u, sum_i + x_i
    z_u, z_i = sum_u / (num_layers + 1), sum_i / (num_layers + 1)
    s_pos = (z_u[u] * z_i[pos_i]).sum(-1)
    s_neg = (z_u[u] * z_i[neg_i]).sum(-1)
    loss = F.softplus(s_neg - s_pos).mean()
    reg = torch.zeros((), dtype=dtype)
    if drop != "reg":
        reg = reg + ((ue[u] ** 2).sum() + (ie[pos_i] ** 2).sum() + (ie[neg_i] ** 2).sum()) / max(1, u.shape[0])
    if drop != "delta":
        reg = reg + 1e-3 * ((ud ** 2).sum() + (idl ** 2).sum()) / (num_cu + num_ci)
    if drop != "weight":
        reg = reg + 1e-6 * (w ** 2).sum()
    loss = loss + reg_lambda * reg
    if teacher is not None and drop != "kd":
        t_u, t_i = (torch.tensor(np.asarray(t), dtype=dtype) for t in teacher)
        loss = loss + kd_lambda * (((z_u - t_u) ** 2).mean() + ((z_i - t_i) ** 2).mean())
    loss.backward()
    return float(loss.detach()), {k: (v.grad if v.grad is not None else torch.zeros_like(v)).numpy() for k, v in p.items()}


def edge_case(num_cu, num_ci, d, num_layers, batch, seed, no_edges=False):
    """Seeded inputs of one case: a graph in CSR order with (where the shape allows) user row 0 full,
    the last user row empty and the last item column empty; fp32 parameters with non-zero deltas;
    ``batch`` uniform triplets (far more than rows: shared users and items, some rows never drawn when
    the batch is small); teacher tables."""
    rng = np.random.default_rng(seed)
    dense = rng.random((num_cu, num_ci)) < 0.3
    if num_cu > 1 and num_ci > 1:
        dense[0, :] = True
        dense[-1, :] = False
        dense[:, -1] = False
    if no_edges:
        dense[:] = False
    cu, ci = np.nonzero(dense)  # row-major: CSR order
    f32 = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    params = {"user_emb.weight": 0.1 * f32(num_cu, d), "item_emb.weight": 0.1 * f32(num_ci, d),
              "user_delta": 0.05 * f32(num_cu, d), "item_delta": 0.05 * f32(num_ci, d),
              "edge_logit": (1.5 * f32(cu.shape[0]) + 0.5).astype(np.float32)}
    u = rng.integers(0, num_cu, batch)
    pos_i = rng.integers(0, num_ci, batch)
    neg_i = rng.integers(0, num_ci, batch)
    if batch > 2:
        neg_i[1] = pos_i[0]  # one item positive and negative in the same batch
    teacher = (0.1 * f32(num_cu, d), 0.1 * f32(num_ci, d))
    return {"params": params, "edge_index": np.stack([cu, ci]).astype(np.int64), "u": u, "pos_i": pos_i,
            "neg_i": neg_i, "teacher": teacher, "num_layers": num_layers}


# ---- Adam in fp64 ----------------------------------------------------------------------------------------
def adam_step64(p, m, v, g, lr, step, betas=(0.9, 0.999), eps=1e-8):
    """manual_adam_step (distill_recsys.py:402-439) on numpy arrays, in fp64: the new (p, m, v)."""
    p, m, v, g = (np.asarray(a, np.float64) for a in (p, m, v, g))
    b1, b2 = betas
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    p = p - lr * (m / (1.0 - b1 ** step)) / (np.sqrt(v / (1.0 - b2 ** step)) + eps)
    return p, m, v


# ---- the error measure of tests/test_gpu_refine_forms.py and its yardstick ---------------------------------
FLOOR = 2.0 ** -23
TENSORS = NAMES + ("loss",)


def measure(x, g64):
    """e(x) = max |x - g64| / max |g64|, the absolute maximum where g64 is identically zero (or empty: 0)."""
    x, g64 = np.asarray(x, np.float64), np.asarray(g64, np.float64)
    if g64.size == 0:
        return 0.0
    top = float(np.abs(g64).max())
    err = float(np.abs(x - g64).max())
    return err / top if top > 0.0 else err


def measures(got, want):
    """{tensor: e} of (loss, grads) against the fp64 (loss, grads)."""
    out = {k: measure(got[1][k], want[1][k]) for k in NAMES}
    out["loss"] = measure(got[0], want[0])
    return out


def run_case(c, **kw):
    return loss_and_grads(c["params"], c["edge_index"], c["num_layers"], c["u"], c["pos_i"], c["neg_i"],
                          c["reg_lambda"], c["teacher"], c["kd_lambda"], **kw)


@functools.lru_cache(maxsize=None)
def references(name):
    """Of the case ``name`` of tests/refine_cases.py: ``ref`` the fp64 (loss, grads), ``e32`` and ``e32r``
    the measures of the fp32 restatement in the given and in the reversed order, ``yard`` per tensor the
    largest of the two and 2^-23. Computed once; the tests read it and leave it unchanged."""
    c = refine_cases.case(name)
    ref = run_case(c)
    e32 = measures(run_case(c, dtype=torch.float32), ref)
    e32r = measures(run_case(c, dtype=torch.float32, reverse=True), ref)
    yard = {k: max(e32[k], e32r[k], FLOOR) for k in TENSORS}
    return {"ref": ref, "e32": e32, "e32r": e32r, "yard": yard}
