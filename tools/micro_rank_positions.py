"""Full-ranking positions at the synthetic Ali-Display shape of tools/micro_rank_topk.py (17,730 users,
10,036 items, d = 64, 115,882 training pairs as the mask, 2 to 5 evaluation lines per user) for a
condensed model of 1,773 x 1,004 clusters, by four routes that answer the same question:

* dense    — gdd_score_positions on the expanded tables cu_z[u2cu], ci_z[i2ci];
* cluster  — gdd_cluster_positions on the cluster tables (a whole call: the distinct clusters of the
             request are found on the host and uploaded, the workspace is allocated);
* matmul   — what a user could do before: chunks of U[users] @ V.T, the mask written into the chunk,
             each target's score gathered and compared against its row, summed (ties by item id);
* ranking_evaluator — one RankingEvaluator call (a 20-item list and its metrics), for scale only.

Three target sets: every user's distinct held-out items, T = 20 targets per user (the fidelity case:
a teacher's top 20) and T = 100.

    python tools/micro_rank_positions.py --out profiles/rank_positions.json

Every route is warmed up, then the routes are timed in turn inside one loop with device events
around a whole call that ends in the copy of its positions to the host; median, min and max over
--reps are recorded. Peak device memory of one call is torch.cuda.max_memory_allocated above the
resident inputs (tables, mask and targets on the device). The dense and the cluster route must give
the same integers; the matmul route's GEMM rounds scores differently from the fma chain, so its share
of equal positions is recorded instead.
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


def matmul_positions(U, V, mask_ptr, mask_col, mask_value, tg_ptr, tg_col, chunk):
    """Positions by score chunks: [chunk, I] scores, the mask scattered in, one pass per target slot."""
    B, n_items = U.shape[0], V.shape[0]
    lens = tg_ptr[1:] - tg_ptr[:-1]
    width = int(lens.max().item()) if B else 0
    ids = torch.arange(n_items, device=U.device, dtype=torch.int32)[None, :]
    out = torch.zeros(int(tg_col.numel()), dtype=torch.int32, device=U.device)
    mrow = torch.repeat_interleave(torch.arange(B, device=U.device), (mask_ptr[1:] - mask_ptr[:-1]).long())
    for b0 in range(0, B, chunk):
        b1 = min(B, b0 + chunk)
        S = U[b0:b1] @ V.T
        lo, hi = int(mask_ptr[b0].item()), int(mask_ptr[b1].item())
        S[mrow[lo:hi] - b0, mask_col[lo:hi].long()] = mask_value
        ln = lens[b0:b1]
        for j in range(width):
            has = ln > j
            e = (tg_ptr[b0:b1] + j).long().clamp_(max=max(int(tg_col.numel()) - 1, 0))
            t = torch.where(has, tg_col[e], torch.zeros_like(tg_col[e]))
            ts = S.gather(1, t.long()[:, None])
            cnt = ((S > ts) | ((S == ts) & (ids < t[:, None]))).sum(1, dtype=torch.int32)
            out[e[has]] = cnt[has]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rank_positions.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--users", type=int, default=17730)
    ap.add_argument("--items", type=int, default=10036)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--reduction", type=float, default=0.1)
    ap.add_argument("--chunk", type=int, default=2048, help="users per score chunk of the matmul route")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_rank_positions: no HIP device visible; nothing is measured without one")
    from gdd.condrank import CondensedRecommender, mask_rows
    from gdd.rankeval import RankingEvaluator
    from gdd.rankpos import PositionEvaluator, _cluster_positions, _score_positions

    rng = np.random.RandomState(0)
    n, m, d = a.users, a.items, a.dim
    key = np.unique(rng.randint(0, n * m, 125000))[:115882]
    train = sp.coo_matrix((np.ones(key.shape[0], np.float32), (key // m, key % m)), shape=(n, m)).tocsr()
    eu = np.repeat(np.arange(n), rng.randint(2, 6, n))
    ei = rng.randint(0, m, eu.shape[0])
    num_cu, num_ci = int(np.ceil(n * a.reduction)), int(np.ceil(m * a.reduction))
    u2cu, i2ci = rng.randint(0, num_cu, n), rng.randint(0, num_ci, m)
    dev = torch.device("cuda")
    cu_z = (torch.randn(num_cu, d, generator=torch.Generator().manual_seed(1)) * 0.1).to(dev)
    ci_z = (torch.randn(num_ci, d, generator=torch.Generator().manual_seed(2)) * 0.1).to(dev)
    U = cu_z[torch.from_numpy(u2cu).to(dev)].contiguous()
    V = ci_z[torch.from_numpy(i2ci).to(dev)].contiguous()
    rec = CondensedRecommender(cu_z, ci_z, u2cu, i2ci)
    mask_value = -1e9
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)  # noqa: E731
    mask = tuple(t(x) for x in mask_rows(train, None, n, m))
    ev = PositionEvaluator(train, eu, ei, (20,), dev, mask_value=mask_value)
    g = ev._prep._prepare()
    lists_ev = RankingEvaluator(train, eu, ei, (20,), dev, mask_value=mask_value)
    G = int(np.unique(u2cu).shape[0])
    result = {"device": torch.cuda.get_device_name(0), "users": n, "items": m, "dim": d, "num_cu": num_cu,
              "num_ci": num_ci, "train_pairs": int(key.shape[0]), "eval_lines": int(eu.shape[0]),
              "score_matrix_bytes": 4 * n * m, "cluster_workspace_bytes": 4 * G * num_ci,
              "matmul_chunk_users": a.chunk, "cases": []}
    sets = [("held_out", g["te_ptr"], g["te_col"])]
    for T in (20, 100):
        sets.append((f"T={T}", t((np.arange(n + 1) * T).astype(np.int32)),
                     t(rng.randint(0, m, n * T).astype(np.int32))))
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    for name, tg_ptr, tg_col in sets:
        routes = {
            "dense": lambda: _score_positions(U, V, None, mask, mask_value, tg_ptr, tg_col, bad).cpu(),
            "cluster": lambda: _cluster_positions(rec, None, mask, mask_value, tg_ptr, tg_col).cpu(),
            "matmul": lambda: matmul_positions(U, V, mask[0], mask[1], mask_value, tg_ptr, tg_col, a.chunk).cpu(),
            "ranking_evaluator": lambda: lists_ev(U, V),
        }
        for fn in routes.values():
            fn(), fn()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, fn in routes.items():
                times[k].append(timed(fn)[0])
        dense, cluster, mm = routes["dense"](), routes["cluster"](), routes["matmul"]()
        case = {"targets": name, "n_targets": int(tg_col.numel()),
                "cluster_equals_dense": bool(torch.equal(dense, cluster)),
                "matmul_share_equal_to_dense": float((dense == mm).float().mean()),
                "matmul_largest_difference": int((dense - mm).abs().max()),
                "mean_position": float(dense.float().mean())}
        for k, fn in routes.items():
            case[k] = stats(times[k])
            case[k]["peak_bytes"] = peak_mem(fn)
        case["dense_over_cluster"] = case["dense"]["median_ms"] / case["cluster"]["median_ms"]
        case["matmul_over_dense"] = case["matmul"]["median_ms"] / case["dense"]["median_ms"]
        print(json.dumps(case))
        result["cases"].append(case)
    assert int(bad.item()) == 0
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
