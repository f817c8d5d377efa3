"""An fp64 restatement of the refinement epoch's loss (the LightGCN forward over the condensed graph,
the softplus BPR loss, its three regularisers and the KD term) in plain torch on the CPU, with
``index_add_`` scatters and autograd for the gradients: the yardstick of tests/test_gpu_refine.py.
Also the seeded inputs of its edge cases."""
import numpy as np
import torch
import torch.nn.functional as F

NAMES = ("user_emb.weight", "item_emb.weight", "user_delta", "item_delta", "edge_logit")


def loss_and_grads(params, edge_index, num_layers, u, pos_i, neg_i, reg_lambda, teacher=None, kd_lambda=0.01,
                   dtype=torch.float64):
    """``params``: {name: array} (any float dtype); returns (loss, {name: gradient}) computed in ``dtype``."""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in params.items()}
    ue, ie, ud, idl, logit = (p[n] for n in NAMES)
    cu, ci = (torch.as_tensor(np.asarray(a), dtype=torch.int64) for a in edge_index)
    u, pos_i, neg_i = (torch.as_tensor(np.asarray(a), dtype=torch.int64) for a in (u, pos_i, neg_i))
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
    reg = ((ue[u] ** 2).sum() + (ie[pos_i] ** 2).sum() + (ie[neg_i] ** 2).sum()) / max(1, u.shape[0])
    reg = reg + 1e-3 * ((ud ** 2).sum() + (idl ** 2).sum()) / (num_cu + num_ci)
    reg = reg + 1e-6 * (w ** 2).sum()
    loss = loss + reg_lambda * reg
    if teacher is not None:
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
