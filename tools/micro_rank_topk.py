"""One RankingEvaluator call (gdd_score_topk + gdd_rank_metrics + one small copy) against one
RecallEvaluator call (score GEMM + gdd_recall_at_k: mask, k sweeps, hit count) on the same inputs,
at the Ali-Display sizes: I = 10,036 items, d = 64, B = 17,730 (every user, as train_teacher
validates) and B = 5,000 (distill_recsys's --eval_max_users), K = 20 and 100.

    python tools/micro_rank_topk.py --out profiles/rank_topk.json

Synthetic inputs from a seed (normal embeddings x 0.1, 115,882 distinct training pairs, 2 to 5
evaluation lines per user). Both paths are warmed up, then timed with device events around a whole
call (each call ends in its own device-to-host read), alternating the two paths in one loop;
median, min and max over --reps are recorded. The fused kernel alone is timed the same way around
the launch. Peak device memory of one call is torch.cuda.max_memory_allocated above the resident
inputs. FLOPs (2 B I d) and bytes are computed from the shapes: the item table once per workgroup
of 16 users is what the kernel reads through L2. Shares of peak use 157.3 TFLOP/s (vector fp32)
and, for the table traffic, the 8.6 TB/s measured for cache-resident gathers (MI355X figures of the
project's DESIGN.md).
"""
import argparse
import json
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-distillation-for-recommendation_amd"))

PEAK_FP32 = 157.3e12
PEAK_CACHE_BW = 8.6e12
USERS_PER_WG = 16


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": len(ms)}


def peak_mem(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_topk.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--users", type=int, default=17730)
    ap.add_argument("--items", type=int, default=10036)
    ap.add_argument("--dim", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_rank_topk: no HIP device visible; nothing is measured without one")
    from gdd.rankeval import RankingEvaluator
    from gdd.recsys import RecallEvaluator

    rng = np.random.RandomState(0)
    n, m, d = a.users, a.items, a.dim
    key = np.unique(rng.randint(0, n * m, 125000))[:115882]
    train = sp.coo_matrix((np.ones(key.shape[0], np.float32), (key // m, key % m)), shape=(n, m)).tocsr()
    eu = np.repeat(np.arange(n), rng.randint(2, 6, n))
    ei = rng.randint(0, m, eu.shape[0])
    dev = torch.device("cuda")
    U = (torch.randn(n, d, generator=torch.Generator().manual_seed(1)) * 0.1).to(dev)
    V = (torch.randn(m, d, generator=torch.Generator().manual_seed(2)) * 0.1).to(dev)
    result = {"device": torch.cuda.get_device_name(0), "users": n, "items": m, "dim": d,
              "train_pairs": int(key.shape[0]), "eval_lines": int(eu.shape[0]), "cases": []}
    for B in (n, min(5000, n)):
        for K in (20, 100):
            new = RankingEvaluator(train, eu, ei, (K,), dev, mask_value=-1e9, max_users=B)
            old = RecallEvaluator(train, eu, ei, K, dev, max_users=B)
            for _ in range(3):
                new(U, V), old(U, V), new._lists(U, V)
            torch.cuda.synchronize()
            t_new, t_old, t_kern = [], [], []
            for _ in range(a.reps):
                t_old.append(timed(lambda: old(U, V))[0])
                t_new.append(timed(lambda: new(U, V))[0])
                t_kern.append(timed(lambda: new._lists(U, V))[0])
            # the same lists give the same hits: hits@K over the users / total pairs is the old path's
            # number (the GEMM's scores and the fma chain's can order a near-tie differently)
            m_new, r_old = new(U, V), old(U, V)
            total = int(new._dev["te_col"].numel())
            hits = int(np.rint(m_new["precision"][0] * K * m_new["users"]))
            flops = 2.0 * B * m * d
            table = m * d * 4
            l2_bytes = float(-(-B // USERS_PER_WG)) * table
            k_s = stats(t_kern)["median_ms"] * 1e-3
            case = {"B": B, "K": K, "ranking_evaluator": stats(t_new), "recall_evaluator": stats(t_old),
                    "score_topk_launch": stats(t_kern),
                    "speedup_median": stats(t_old)["median_ms"] / stats(t_new)["median_ms"],
                    "peak_bytes_ranking_evaluator": peak_mem(lambda: new(U, V)),
                    "peak_bytes_recall_evaluator": peak_mem(lambda: old(U, V)),
                    "flops": flops, "item_table_bytes": table, "table_bytes_through_l2": l2_bytes,
                    "kernel_tflops": flops / k_s / 1e12, "kernel_share_of_fp32_peak": flops / k_s / PEAK_FP32,
                    "kernel_table_tb_per_s": l2_bytes / k_s / 1e12,
                    "kernel_share_of_cache_bw": l2_bytes / k_s / PEAK_CACHE_BW,
                    "least_time_ms": max(flops / PEAK_FP32, l2_bytes / PEAK_CACHE_BW) * 1e3,
                    "bound": "fp32 FMA rate" if flops / PEAK_FP32 > l2_bytes / PEAK_CACHE_BW else "L2 table traffic",
                    "recall_old_path": r_old, "ndcg_new_path": float(m_new["ndcg"][0]),
                    "hits_new_path": hits, "total_pairs": total,
                    "recall_from_new_hits": hits / max(1, total)}
            print(json.dumps(case))
            result["cases"].append(case)
            del new, old
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
