"""One Rankformer layer at the Ali-Display shape, fused passes against a composition of torch ops.

    python tools/bench_rankformer.py [--out profiles/rankformer_layer.json]

The interaction data is the training split under tests/golden/ (17,730 users x 10,036 items,
121,178 lines of which 115,882 are distinct pairs: the layer is defined over distinct pairs, so the
repeats are dropped), d = 64, x ~ N(0, 0.1²). Both paths evaluate the same fused formulas
(DESIGN.md "Rankformer teacher") on the same device in the same process:

* fused: gdd.rankformer.RankformerLayer (gdd_rank_rowpass / gdd_rank_wsum, no float atomics);
* composed: the per-interaction sums as gathered ``index_add_`` (the reference's kind of
  evaluation; float atomics), everything else the same torch expressions. It never builds a
  rows x d x d tensor.

Timing: after a warm-up of both, ``--rounds`` rounds alternate the two paths; a round runs
``--iters`` layers back to back between two device synchronisations and a host clock. Reported per
path: the median round's time per layer, forward only (no autograd graph) and forward + backward
(gradient of sum(z * W) with respect to x). Also the largest difference between the two paths'
outputs and gradients.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "graph-distillation-for-recommendation_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def composed_layer(x, u, i, n, m, dp, dn, alpha=2.0, c=0.0):
    """The fused formulas with every per-interaction sum as a gathered index_add_."""
    d = x.shape[1]
    xh = F.normalize(x)
    xu, xi, vu, vi = xh[:n], xh[n:], x[:n], x[n:]
    z = lambda *shape: torch.zeros(*shape, dtype=x.dtype, device=x.device)  # noqa: E731
    vi_e = vi[i]
    s = (xu[u] * xi[i]).sum(1)
    S = z(n).index_add_(0, u, s).unsqueeze(1)
    SV = z(n, d).index_add_(0, u, vi_e)
    A = z(n, d).index_add_(0, u, s.unsqueeze(1) * vi_e)
    bp = S / dp
    bn = ((xu @ xi.sum(0)).unsqueeze(1) - S) / dn
    num_u = (A + (alpha - bn) * SV) / dp + (xu @ (xi.t() @ vi) - A - (bp + alpha) * (vi.sum(0) - SV)) / dn
    D = (bp - bn + alpha).clamp(min=c)
    z_u = num_u / (D + D)
    op = (s - bn[:, 0][u] + alpha) / dp[:, 0][u]
    om = (s - bp[:, 0][u] - alpha) / dn[:, 0][u]
    Y = z(m, d).index_add_(0, i, (op - om).unsqueeze(1) * vu[u])
    ta = z(m).index_add_(0, i, op)
    tb = z(m).index_add_(0, i, om)
    xun = xu / dn
    coef = (bp + alpha) / dn
    num_i = Y + xi @ (xun.t() @ vu) - (coef * vu).sum(0)
    den_i = ta.clamp(min=c) + (-(xi @ xun.sum(0) - coef.sum() - tb)).clamp(min=c)
    return torch.cat([z_u, num_i / den_i.unsqueeze(1)], 0)


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3  # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rankformer_layer.json"))
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rankformer: no HIP device visible; nothing is measured without one")
    from golden_util import load
    from gdd.rankformer import InteractionGraph, RankformerLayer

    zf = load("golden_alidisplay.npz")
    n, m = 17730, 10036
    key = np.unique(zf["train_u"].astype(np.int64) * m + zf["train_i"].astype(np.int64))
    lines, E = int(zf["train_u"].shape[0]), int(key.shape[0])
    graph = InteractionGraph(key // m, key % m, n, m, "cuda")
    u, i = graph.train_u, graph.train_i
    gen = torch.Generator(device="cuda").manual_seed(0)
    x0 = 0.1 * torch.randn(n + m, a.dim, device="cuda", generator=gen)
    W = torch.randn(n + m, a.dim, device="cuda", generator=gen)
    layer = RankformerLayer(2.0, 0.0)

    def fused(x):
        return layer(x, graph)

    def composed(x):
        return composed_layer(x, u, i, n, m, graph.dpos, graph.dneg)

    def fwd(path):
        def run():
            with torch.no_grad():
                path(x0)
        return run

    def fwd_bwd(path):
        def run():
            x = x0.detach().requires_grad_(True)
            (path(x) * W).sum().backward()
            return x.grad
        return run

    # the two paths compute the same thing
    with torch.no_grad():
        zd = float((fused(x0) - composed(x0)).abs().max())
        zs = float(fused(x0).abs().max())
    gf, gc = fwd_bwd(fused)(), fwd_bwd(composed)()
    gd, gs = float((gf - gc).abs().max()), float(gf.abs().max())
    graph.check()
    same_bits = bool(torch.equal(gf, fwd_bwd(fused)()))

    runs = {"fused_fwd": fwd(fused), "composed_fwd": fwd(composed),
            "fused_fwd_bwd": fwd_bwd(fused), "composed_fwd_bwd": fwd_bwd(composed)}
    for fn in runs.values():
        timed(fn, a.warmup)
    times = {k: [] for k in runs}
    for _ in range(a.rounds):
        for k, fn in runs.items():  # alternating: the paths share whatever else the host is doing
            times[k].append(timed(fn, a.iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    result = {
        "what": "one Rankformer layer, Ali-Display training split, ms per layer (median round)",
        "device": torch.cuda.get_device_name(0), "users": n, "items": m, "train_lines": lines,
        "distinct_pairs": E, "dim": a.dim, "iters_per_round": a.iters, "rounds": a.rounds,
        "fused_fwd_ms": med["fused_fwd"], "composed_fwd_ms": med["composed_fwd"],
        "fwd_ratio_composed_over_fused": med["composed_fwd"] / med["fused_fwd"],
        "fused_fwd_bwd_ms": med["fused_fwd_bwd"], "composed_fwd_bwd_ms": med["composed_fwd_bwd"],
        "fwd_bwd_ratio_composed_over_fused": med["composed_fwd_bwd"] / med["fused_fwd_bwd"],
        "rounds_ms": {k: [round(t, 4) for t in v] for k, v in times.items()},
        "max_abs_diff_forward": zd, "max_abs_forward": zs, "max_abs_diff_gradient": gd, "max_abs_gradient": gs,
        "fused_gradient_bit_identical_between_runs": same_bits,
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "rounds_ms"}))


if __name__ == "__main__":
    main()
