"""Top-K lists of a condensed recommender two ways, at the Ali-Display sizes with synthetic data:
17,730 users and 10,036 items, d = 64, reduction 0.1 (1,773 x 1,004 clusters), K = 20, every user,
and an exclude matrix with the training set's density (115,882 distinct pairs).

    python tools/micro_condensed_topk.py --out profiles/condensed_recommend.json

* ``expanded``: what ranking a condensed model took before gdd.condrank: the two gathers
  ``cu_z[u2cu]``, ``ci_z[i2ci]`` and ``gdd.recommend`` on them (B I d fmas);
* ``condensed``: ``gdd.recommend_condensed`` (the membership CSR and the device copies of the maps
  built inside the call) and ``CondensedRecommender.recommend`` on an object prepared once
  (G num_ci d fmas and one expansion pass).

Both are warmed up, then timed with device events around a whole call (each ends in its own
device-to-host read of the counters), alternating the paths in one loop; median, min and max over
--reps are recorded. The two launches of the condensed path (gdd_score_topk over the clusters,
gdd_cluster_expand_topk) are timed the same way around each launch on prepared device inputs, and
so is the expanded path's device work alone (two gathers and its launch). gdd.recommend's host
preparation of the exclude rows (a gather and a sort per call, gdd.rankeval._rows_of; the condensed
path slices a canonical scipy CSR instead) is timed with the host clock, and whole calls without an
exclude matrix, where neither path prepares rows, are timed as a second pair. The
lists of the two paths are compared (they must be equal) before anything is written. Workspace
bytes are the condensed path's allocations besides its outputs and mask; peak bytes are
torch.cuda.max_memory_allocated above the resident inputs for one call of each path.
"""
import argparse
import json
import os
import sys
import time

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


def cover(rng, n, k):
    """n labels over k clusters, every cluster used."""
    return rng.permutation(np.concatenate([np.arange(k), rng.randint(0, k, n - k)])).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "condensed_recommend.json"))
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--users", type=int, default=17730)
    ap.add_argument("--items", type=int, default=10036)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--rate", type=float, default=0.1)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=115882)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("micro_condensed_topk: no HIP device visible; nothing is measured without one")
    import gdd
    from gdd import _lib
    from gdd.rankeval import _rows_of, _score_topk

    rng = np.random.RandomState(0)
    n, m, d, K = a.users, a.items, a.dim, a.k
    num_cu, num_ci = int(np.ceil(n * a.rate)), int(np.ceil(m * a.rate))
    key = np.unique(rng.randint(0, n * m, int(a.pairs * 1.08)))[:a.pairs]
    train = sp.coo_matrix((np.ones(key.shape[0], np.float32), (key // m, key % m)), shape=(n, m)).tocsr()
    u2cu, i2ci = cover(rng, n, num_cu), cover(rng, m, num_ci)
    dev = torch.device("cuda")
    cu_z = (torch.randn(num_cu, d, generator=torch.Generator().manual_seed(1)) * 0.1).to(dev)
    ci_z = (torch.randn(num_ci, d, generator=torch.Generator().manual_seed(2)) * 0.1).to(dev)
    u2cu_t, i2ci_t = torch.from_numpy(u2cu).to(dev), torch.from_numpy(i2ci).to(dev)
    rec = gdd.CondensedRecommender(cu_z, ci_z, u2cu, i2ci)

    def expanded():
        return gdd.recommend(cu_z[u2cu_t], ci_z[i2ci_t], K, exclude=train, mask_value=-1e9, return_scores=True)

    def one_call():
        return gdd.recommend_condensed(cu_z, ci_z, u2cu, i2ci, K, exclude=train, mask_value=-1e9,
                                       return_scores=True)

    def prepared():
        return rec.recommend(K, exclude=train, mask_value=-1e9, return_scores=True)

    # the two launches on prepared device inputs
    lib = _lib.device_lib()
    g = rec._prepare()
    groups, row = np.unique(u2cu, return_inverse=True)
    G, L = int(groups.shape[0]), min(num_ci, 256)
    t32 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).to(dev)  # noqa: E731
    groups_t, row_t = t32(groups), t32(row.ravel())
    mp, mc = (t32(x) for x in _rows_of(train, np.arange(n), m))
    counters = torch.zeros(2, dtype=torch.int32, device=dev)
    items = torch.empty(n, K, dtype=torch.int32, device=dev)
    scores = torch.empty(n, K, dtype=torch.float32, device=dev)
    incomplete = torch.empty(n, dtype=torch.int32, device=dev)

    def stage_a():
        return _score_topk(g["cu_z"], g["ci_z"], L, groups_t, None, 0.0, True, counters[:1])

    cl_item, cl_score = stage_a()

    def stage_b():
        _lib.check(lib.gdd_cluster_expand_topk(
            n, m, num_ci, L, K, None, n, row_t.data_ptr(), G, cl_item.data_ptr(), cl_score.data_ptr(),
            g["mem_ptr"].data_ptr(), g["mem_item"].data_ptr(), mp.data_ptr(), mc.data_ptr(), -1e9,
            items.data_ptr(), scores.data_ptr(), incomplete.data_ptr(), counters[1:].data_ptr(),
            counters[:1].data_ptr(), _lib.stream_ptr(dev)))

    def expanded_launches():  # the parent path's device work alone: two gathers and one launch
        return _score_topk(cu_z[u2cu_t], ci_z[i2ci_t], K, None, (mp, mc), -1e9, True, counters[:1])

    def expanded_unmasked():  # whole calls without an exclude matrix: no host preparation of rows
        return gdd.recommend(cu_z[u2cu_t], ci_z[i2ci_t], K, return_scores=True)

    def prepared_unmasked():
        return rec.recommend(K, return_scores=True)

    def host_mask():  # recommend's host preparation of the exclude rows (the condensed path slices the CSR)
        t0 = time.perf_counter()
        _rows_of(train, np.arange(n), m)
        return (time.perf_counter() - t0) * 1e3

    for _ in range(3):
        expanded(), one_call(), prepared(), stage_a(), stage_b(), expanded_launches()
        expanded_unmasked(), prepared_unmasked()
    torch.cuda.synchronize()
    want, got = expanded(), prepared()
    same = bool(torch.equal(want[0], got[0]) and torch.equal(want[1].view(torch.int32), got[1].view(torch.int32)))
    if not same:
        raise SystemExit("micro_condensed_topk: the two paths disagree; nothing is recorded")
    t = {k: [] for k in ("expanded", "one_call", "prepared", "stage_a", "stage_b", "expanded_launches", "host_mask",
                         "expanded_unmasked", "prepared_unmasked")}
    for _ in range(a.reps):
        t["expanded_unmasked"].append(timed(expanded_unmasked)[0])
        t["prepared_unmasked"].append(timed(prepared_unmasked)[0])
        t["expanded_launches"].append(timed(expanded_launches)[0])
        t["host_mask"].append(host_mask())
        t["expanded"].append(timed(expanded)[0])
        t["one_call"].append(timed(one_call)[0])
        t["prepared"].append(timed(prepared)[0])
        t["stage_a"].append(timed(stage_a)[0])
        t["stage_b"].append(timed(stage_b)[0])
    s = {k: stats(v) for k, v in t.items()}
    result = {
        "device": torch.cuda.get_device_name(0), "users": n, "items": m, "dim": d, "num_cu": num_cu,
        "num_ci": num_ci, "K": K, "train_pairs": int(key.shape[0]), "lists_equal": same,
        "last_info": rec.last_info,
        "expanded_gathers_plus_recommend": s["expanded"],
        "recommend_condensed_one_call": s["one_call"],
        "condensed_recommender_prepared": s["prepared"],
        "launch_score_topk_clusters": s["stage_a"],
        "launch_cluster_expand_topk": s["stage_b"],
        "expanded_gathers_plus_launch_alone": s["expanded_launches"],
        "host_mask_rows_of_exclude": s["host_mask"],
        "expanded_without_exclude": s["expanded_unmasked"],
        "condensed_recommender_without_exclude": s["prepared_unmasked"],
        "speedup_median_without_exclude": s["expanded_unmasked"]["median_ms"] / s["prepared_unmasked"]["median_ms"],
        "device_work_ratio_median": s["expanded_launches"]["median_ms"] / (s["stage_a"]["median_ms"]
                                                                        + s["stage_b"]["median_ms"]),
        "speedup_median_one_call": s["expanded"]["median_ms"] / s["one_call"]["median_ms"],
        "speedup_median_prepared": s["expanded"]["median_ms"] / s["prepared"]["median_ms"],
        "fma_expanded": float(n) * m * d, "fma_condensed": float(G) * num_ci * d,
        "workspace_bytes_condensed": rec.workspace_bytes(n, G),
        "peak_bytes_expanded": peak_mem(expanded), "peak_bytes_condensed": peak_mem(prepared),
    }
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
