#!/usr/bin/env python3
"""The recommender's SVD embeddings (compute_svd_embeddings, k = 64): host scipy svds against the
device block subspace iteration (gdd.svd), on the real Ali-Display interactions (the fixture
tests/golden/golden_alidisplay.npz) and on the ML-1M-shaped synthetic of tools/bench_recsys_e2e.py.

For each input, in one process: host svds once; the device path cold, then warm as the median of 5
with a synchronise around each; both forms of the Gram kernel (fp64 MFMA, plain fp64 fma) on the
big-side block, median of 20 by device events. Writes the record to --out (default
profiles/svd_device.json) and prints it as one JSON line.
usage: bench_svd.py [--out PATH] [--inputs alidisplay,ml1m]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "graph-distillation-for-recommendation_amd"), os.path.join(ROOT, "tests"),
          os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gdd import distill_recsys as D  # noqa: E402
from gdd import svd as S  # noqa: E402


def load_alidisplay():
    from golden_util import load
    z = load("golden_alidisplay.npz")
    nu, ni = z["user_emb"].shape[0], z["item_emb"].shape[0]
    return D.build_interaction_matrix(nu, ni, z["train_u"], z["train_i"])


def load_ml1m():
    from bench_recsys_e2e import write_dataset
    with tempfile.TemporaryDirectory() as tmp:
        write_dataset(tmp)
        ds = D.load_rankformer_dataset(tmp, "ml1m")
    return D.build_interaction_matrix(ds.num_users, ds.num_items, ds.train_u, ds.train_i)


def time_gram(n, b, form, reps=20):
    W = torch.randn((n, b), dtype=torch.float64, device="cuda")
    S.gram_f64(W, form)
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        S.gram_f64(W, form)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def measure(name, R, dim=64):
    rec = {"input": name, "shape": list(R.shape), "nnz": int(R.nnz), "dim": dim}
    t0 = time.perf_counter()
    hu, hi = D.compute_svd_embeddings(R, dim, 42, backend="host")
    rec["host_svds_s"] = time.perf_counter() - t0
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    k = min(dim, min(R.shape) - 1)
    _, sig, _, info = S.truncated_svd(R, k)
    torch.cuda.synchronize()
    rec["device_cold_s"] = time.perf_counter() - t0
    rec["steps"], rec["residual"], rec["block"] = info["steps"], info["residual"], info["block"]
    warm = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        du, di = S.svd_embeddings(R, dim, seed=42)
        torch.cuda.synchronize()
        warm.append(time.perf_counter() - t0)
    rec["device_warm_s"] = statistics.median(warm)
    rec["device_warm_all_s"] = warm
    rec["device_beats_host"] = bool(rec["device_warm_s"] < rec["host_svds_s"])
    # agreement with the host factors: per-column |cos| (svds is converged to its own tolerance)
    cos = []
    for o, h in ((du, hu), (di, hi)):
        o, h = o.astype(np.float64), h.astype(np.float64)
        cos.append(np.abs((o * h).sum(0)) / (np.linalg.norm(o, axis=0) * np.linalg.norm(h, axis=0)))
    rec["min_abs_cos_vs_host"] = float(min(c.min() for c in cos))
    nb, b = max(R.shape), info["block"]
    rec["gram_rows"] = nb
    rec["gram_mfma_ms"] = time_gram(nb, b, 0)
    rec["gram_fma_ms"] = time_gram(nb, b, 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "svd_device.json"))
    ap.add_argument("--inputs", default="alidisplay,ml1m")
    a = ap.parse_args()
    loaders = {"alidisplay": load_alidisplay, "ml1m": load_ml1m}
    recs = [measure(n, loaders[n]()) for n in a.inputs.split(",")]
    out = {"what": "compute_svd_embeddings k=64: host scipy svds vs gdd.svd (fp64 block subspace iteration, "
                   "oversample 64, tol 1e-10, check every 8 steps), one process per record",
           "device": torch.cuda.get_device_name(0), "records": recs}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
