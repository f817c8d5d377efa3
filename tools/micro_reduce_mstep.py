#!/usr/bin/env python3
"""The order-free fixed-point M-step (ShardedKMeans(mstep="reduce")) at the products k-means shape
(2,449,029 x 47 Gaussian logits, k = 196, labels of a nearest-centre pass): one rank's local phase
(gdd_lloyd_reduce_local: bucketing + int64 sums + counts + changed count) over n, n/2, n/4 and n/8
rows and the update from the reduced buffer (gdd_lloyd_reduce_update), against the ordered M-step
(gdd_lloyd_mstep: grouping + ordered fold + empty check) and update (gdd_lloyd_update) on the same
inputs in the same run. Prints one JSON object (and writes it to --out): times in ms, the ratio to the
ordered M-step, the 64-bit integer atomics the sum kernel issues at most, and an N = 8 iteration
MODELLED from the measured pieces (RCCL is not run here)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "graph-distillation-for-recommendation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gdd import _lib  # noqa: E402
from gdd.kmeans import _Ops  # noqa: E402

def tile_of(m):
    """k_reduce_sum's bucketed rows per block: the largest of 1024, 512, 256 that gives 4096 blocks."""
    t = 1024
    while t > 256 and -(-m // t) < 4096:
        t >>= 1
    return t


def timed(run, reps=20):
    for _ in range(3):
        run()
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    e[0].record()
    for _ in range(reps):
        run()
    e[1].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]) / reps


def atomics_bound(labels, k, dim):
    """One atomic per (tile, column) for the tile's first cluster, one per (worker, further cluster
    run, column) — an upper bound: zero sums are not sent."""
    cid = np.repeat(np.arange(k), np.bincount(labels, minlength=k))
    pos = np.arange(cid.shape[0])
    tile = tile_of(cid.shape[0])
    worker = tile // 4  # four 64-lane workers per block at dim > 32
    first = cid[(pos // tile) * tile]
    other = cid != first
    runs = np.unique((pos[other] // worker) * k + cid[other]).shape[0]
    tiles = -(-cid.shape[0] // tile)
    return int((tiles + runs) * dim), int(tiles)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--ranks", default="1,2,4,8", help="row counts n / R to time (the last one feeds the model)")
    ap.add_argument("--tiles", default="", help="also time the local phase with these rows per block pinned "
                    "(GDD_FORCE=reduce_tile=N), e.g. 256,512,1024,2048")
    args = ap.parse_args()
    lib = _lib.device_lib()
    n, dim, k = 2449029, 47, 196
    g = torch.Generator(device="cuda").manual_seed(5)
    X = torch.randn(n, dim, device="cuda", generator=g)
    C = X[torch.randperm(n, device="cuda", generator=g)[:k]].contiguous()
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    _Ops("cuda", n, k, dim).assign(X, C, labels=labels)
    lab_h = labels.cpu().numpy()
    s = _lib.stream_ptr()
    state = torch.zeros(lib.gdd_lloyd_state_bytes(), dtype=torch.uint8, device="cuda")
    res = {"shape": [n, dim, k], "message_bytes": 8 * (k * (dim + 1) + 1), "labels_gather_bytes": 4 * n}

    # the ordered M-step and update (unchanged by the reduce mode)
    ws = _lib.workspace(lib.gdd_kmeans_lloyd_ws_bytes(n, dim, k), X.device)
    sums = torch.empty(k, dim, dtype=torch.float32, device="cuda")
    wsum = torch.empty(k, dtype=torch.float32, device="cuda")
    shift = torch.zeros(k, dtype=torch.float32, device="cuda")
    labels_old = torch.full_like(labels, -1)
    res["ordered_mstep_ms"] = timed(lambda: _lib.check(lib.gdd_lloyd_mstep(
        n, dim, X.data_ptr(), labels.data_ptr(), k, 0, dim, sums.data_ptr(), wsum.data_ptr(),
        state.data_ptr(), 0, ws.data_ptr(), ws.numel(), s)))

    def ordered_update():  # re-averages the averaged sums: the same kernels and bytes
        _lib.check(lib.gdd_lloyd_update(n, dim, k, None, dim, sums.data_ptr(), wsum.data_ptr(), C.data_ptr(),
                                        shift.data_ptr(), labels.data_ptr(), labels_old.data_ptr(), 0.0,
                                        state.data_ptr(), 0, s))
    res["ordered_update_ms"] = timed(ordered_update)
    state.zero_()

    # the reduce mode's phases
    exps = torch.zeros(dim, dtype=torch.int32, device="cuda")
    res["exponents_ms"] = timed(lambda: _lib.check(lib.gdd_lloyd_reduce_exponents(
        n, dim, X.data_ptr(), exps.data_ptr(), s)), reps=5)
    buf = torch.zeros(lib.gdd_lloyd_reduce_words(dim, k), dtype=torch.int64, device="cuda")
    rws = _lib.workspace(lib.gdd_lloyd_reduce_ws_bytes(n, dim, k), X.device)
    res["local"] = []
    for world in [int(r) for r in args.ranks.split(",")]:
        m = -(-n // world)
        ms = timed(lambda: _lib.check(lib.gdd_lloyd_reduce_local(
            n, 0, m, dim, X.data_ptr(), labels.data_ptr(), labels_old.data_ptr(), k, exps.data_ptr(),
            buf.data_ptr(), state.data_ptr(), 0, rws.data_ptr(), rws.numel(), s)))
        atomics, tiles = atomics_bound(lab_h[:m], k, dim)
        res["local"].append({"ranks": world, "rows": m, "ms": ms, "ratio_to_ordered_mstep": ms / res["ordered_mstep_ms"],
                             "tile": tile_of(m), "tiles": tiles, "int64_atomics_at_most": atomics})
        print(f"ranks {world}: rows {m}: local {ms:.3f} ms, <= {atomics} 8-byte atomics", flush=True)
        for t in [int(t) for t in args.tiles.split(",") if t]:
            os.environ["GDD_FORCE"] = f"reduce_tile={t}"
            ms_t = timed(lambda: _lib.check(lib.gdd_lloyd_reduce_local(
                n, 0, m, dim, X.data_ptr(), labels.data_ptr(), labels_old.data_ptr(), k, exps.data_ptr(),
                buf.data_ptr(), state.data_ptr(), 0, rws.data_ptr(), rws.numel(), s)))
            del os.environ["GDD_FORCE"]
            res["local"][-1].setdefault("pinned_tile_ms", {})[str(t)] = ms_t
            print(f"  tile {t}: local {ms_t:.3f} ms ({-(-m // t)} blocks)", flush=True)
    _lib.check(lib.gdd_lloyd_reduce_local(n, 0, n, dim, X.data_ptr(), labels.data_ptr(), labels_old.data_ptr(),
                                          k, exps.data_ptr(), buf.data_ptr(), state.data_ptr(), 0,
                                          rws.data_ptr(), rws.numel(), s))
    buf[-1] = 1  # labels changed: the update runs to the convergence test and goes on (tol 0)
    res["reduce_update_ms"] = timed(lambda: _lib.check(lib.gdd_lloyd_reduce_update(
        dim, k, buf.data_ptr(), exps.data_ptr(), 0, sums.data_ptr(), wsum.data_ptr(), C.data_ptr(),
        shift.data_ptr(), 0.0, state.data_ptr(), 0, s)))
    # MODELLED, not measured: the bounded E-step's 233 us per iteration (r06 trace, row-proportional),
    # ~25 us for a small RCCL collective (the planning figure of DESIGN §6), the rest measured above
    l8 = res["local"][-1]["ms"]
    res["modelled_n8_iteration_ms"] = {
        "estep": 0.233 / 8, "local": l8, "all_reduce": 0.025, "update": res["reduce_update_ms"],
        "total": 0.233 / 8 + l8 + 0.025 + res["reduce_update_ms"],
        "ordered_rows_mode_total": 0.233 / 8 + 0.025 + 4.0 * n * (7 / 8) / 300e9 * 1e3
        + res["ordered_mstep_ms"] + res["ordered_update_ms"]}
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
