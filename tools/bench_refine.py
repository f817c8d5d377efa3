#!/usr/bin/env python3
"""The refinement loop (distill_recsys.py:640-733), torch backend against device backend, in one
process on the same inputs: per-epoch wall time of `--epochs` epochs (default 500, the driver's
default), the minimum and the spread of `--repeats` timed runs of each backend after a warm-up,
the two backends alternating. The torch backend is the driver's loop: sample, bpr_loss (+ KD),
backward, manual_adam_step. The device backend is gdd.recsys.DeviceRefiner.run. Both end in a device
synchronise. Also recorded: the device backend's host time per epoch (sampling plus grouping).

Shapes: the condensed Ali-Display shape (1,773 x 1,004 clusters, 51,539 edges) and the condensed
ML-1M shape (604 x 371, 180,000 edges), synthetic (gdd.synth.condensed_bipartite), d = 64, L = 2,
4,096 triplets; each with and without a teacher.

usage: bench_refine.py [--epochs 500] [--repeats 5] [--out profiles/refine_device.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-distillation-for-recommendation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from gdd import recsys as R  # noqa: E402
from gdd import synth  # noqa: E402

SHAPES = {"alidisplay": (1773, 1004, 51539), "ml1m": (604, 371, 180000)}
DIM, LAYERS, BATCH, LR, REG, KD = 64, 2, 4096, 1e-2, 1e-4, 0.01


def make(shape, seed=42):
    num_cu, num_ci, nnz = shape
    C = synth.condensed_bipartite(num_cu, num_ci, nnz, seed)
    dev = torch.device("cuda")
    ei, w0 = R.condensed_csr_to_edge_index(C, device=dev)
    torch.manual_seed(seed)
    model = R.LightGCNCondensed(num_cu, num_ci, DIM, LAYERS, ei, w0, device=dev).to(dev)
    model.train()
    g = torch.Generator().manual_seed(seed)
    teacher = (0.1 * torch.randn(num_cu, DIM, generator=g).to(dev), 0.1 * torch.randn(num_ci, DIM, generator=g).to(dev))
    return model, R._csr_row_to_set_list(C), teacher


def torch_epochs(model, pos, teacher, n, rng, adam_state, first_step):
    params = [p for p in model.parameters() if p.requires_grad]
    dev = params[0].device
    for ep in range(first_step, first_step + n):
        u, pos_i, neg_i = (torch.from_numpy(a).to(dev) for a in
                           R.sample_bpr_triplets_from_condensed(pos, model.num_ci, BATCH, rng))
        loss = model.bpr_loss(u, pos_i, neg_i, reg_lambda=REG)
        if teacher is not None:
            su, si = model.propagate()
            loss = loss + KD * (F.mse_loss(su, teacher[0]) + F.mse_loss(si, teacher[1]))
        loss.backward()
        R.manual_adam_step(params, adam_state, lr=LR, step=ep)
        model.zero_grad(set_to_none=True)
    return float(loss.item())


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def bench(name, with_teacher, epochs, repeats):
    m_t, pos, teacher = make(SHAPES[name])
    m_d, _, _ = make(SHAPES[name])
    teacher = teacher if with_teacher else None
    rng_t, rng_d = np.random.RandomState(42), np.random.RandomState(42)
    adam_state, step = {}, [1]
    refiner = R.DeviceRefiner(m_d, pos, lr=LR, reg_lambda=REG, batch_size=BATCH, rng=rng_d, teacher=teacher,
                              kd_lambda=KD)

    def run_torch():
        torch_epochs(m_t, pos, teacher, epochs, rng_t, adam_state, step[0])
        step[0] += epochs

    def run_device():
        refiner.run(epochs)
    warm = min(50, epochs)
    torch_epochs(m_t, pos, teacher, warm, rng_t, adam_state, step[0])
    step[0] += warm
    refiner.run(warm)
    t_torch, t_dev, host = [], [], []
    for _ in range(repeats):  # alternating
        t_torch.append(timed(run_torch) / epochs * 1e6)
        h0 = refiner.host_s
        t_dev.append(timed(run_device) / epochs * 1e6)
        host.append((refiner.host_s - h0) / epochs * 1e6)
    out = {"shape": name, "num_cu": SHAPES[name][0], "num_ci": SHAPES[name][1], "edges": SHAPES[name][2],
           "teacher": with_teacher, "epochs": epochs, "repeats": repeats,
           "torch_us_per_epoch": {"min": min(t_torch), "max": max(t_torch), "all": t_torch},
           "device_us_per_epoch": {"min": min(t_dev), "max": max(t_dev), "all": t_dev},
           "device_host_sample_group_us_per_epoch": {"min": min(host), "max": max(host)},
           "launches_per_epoch": 7 + 2 * LAYERS}
    out["faster_beyond_spread"] = max(t_dev) < min(t_torch)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "refine_device.json"))
    a = ap.parse_args()
    rows = [bench(name, t, a.epochs, a.repeats) for name in SHAPES for t in (False, True)]
    doc = {"tool": "tools/bench_refine.py", "device": torch.cuda.get_device_name(0), "dim": DIM, "layers": LAYERS,
           "batch": BATCH, "timing": "host clock around epochs ending in a device synchronise; microseconds per epoch",
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
