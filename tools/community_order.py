#!/usr/bin/env python3
"""What the on-device community order (gdd.graph.locality_order(adj, "community")) costs and
gains: gdd.propagate with the intermediate hops in that order against the original ids, "rcm" (scipy,
host) and the true community order, device events, same process, every configuration checked
bit-identical to the original order. Modelled on tools/relabel_products.py (default hop schedule only).

Graphs: the products-shape stochastic block model (2,449,029 nodes, ~126M entries, communities of
2,048 nodes, 90% of the edges inside) with shuffled ids (all four orders) and with contiguous blocks,
the bench's products Chung-Lu graph, and the arxiv-shape SBM of tools/micro_relabel.py with shuffled
ids (the new order only on these three: what it costs where no gain is expected).

For the new order it records the build time (a whole locality_order call, host clock around the
call, which ends in a stream synchronise), the same with 0 sweeps (labels, sort and scatter alone), the
time per sweep from the difference, and the changed counts. "pays per call" at a shape means build +
(T - 1) relabelled hops < (T - 1) original hops; break_even_hops = build / (original - relabelled) per
hop. Prints one JSON line per record; --out FILE also writes them all as one JSON document.
COMMUNITY_REPS (default 3) timed calls per configuration."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                "graph-distillation-for-recommendation_amd"))
import torch  # noqa: E402

import gdd  # noqa: E402
from gdd import synth  # noqa: E402

REPS = int(os.environ.get("COMMUNITY_REPS", "3"))
SWEEPS = 12


def timed(gn, X, T, alpha, relabel):
    out = gdd.propagate(gn, X, T, alpha, relabel=relabel)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        gdd.propagate(gn, X, T, alpha, relabel=relabel)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS, out


def build_seconds(fn):
    """best of REPS host-clock timings of fn() (each ends synchronised) after one warm-up call"""
    out = fn()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, out


def community(gn):
    full_s, rho = build_seconds(lambda: gdd.graph.locality_order(gn, "community", sweeps=SWEEPS))
    base_s, _ = build_seconds(lambda: gdd.graph.locality_order(gn, "community", sweeps=0))
    labels, changed = gdd.graph.community_labels(gn, sweeps=SWEEPS)
    changed = changed.cpu().tolist()
    ran = sum(1 for i, c in enumerate(changed) if i == 0 or changed[i - 1] > 0)
    extra = {"sweeps": SWEEPS, "sweeps_run": ran, "changed": changed,
             "build_s_0_sweeps": base_s, "ms_per_sweep": (full_s - base_s) * 1e3 / max(ran, 1),
             "labels_distinct": int(torch.unique(labels).numel())}
    return rho, full_s, extra


def run(name, g, d, T, alpha, orders, res):
    gn = gdd.normalize_adj(g)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    X = torch.randn(g.n, d, device="cuda", generator=gen)
    hops = T - 1
    ref = None
    base_ms = None
    for kind, rho_fn in orders:
        extra = {}
        if kind == "community":
            rho, order_s, extra = community(gn)
        else:
            t0 = time.perf_counter()
            rho = rho_fn(gn) if rho_fn else None
            torch.cuda.synchronize()
            order_s = time.perf_counter() - t0
        ms, (t, p) = timed(gn, X, T, alpha, rho)
        if ref is None:
            ref, base_ms = (t, p), ms
        same = torch.equal(t.view(torch.int32), ref[0].view(torch.int32)) and \
            torch.equal(p.view(torch.int32), ref[1].view(torch.int32))
        rec = {"graph": name, "order": kind, "n": g.n, "nnz": int(gn.nnz), "d": d, "hops": hops,
               "ms_per_call": ms, "us_per_hop": ms * 1e3 / hops, "order_build_s": order_s,
               "bit_identical_to_original_order": bool(same), "calls": 1 + REPS}
        if rho is not None:
            gain_ms_per_hop = (base_ms - ms) / hops
            rec["call_plus_build_ms"] = ms + order_s * 1e3
            rec["pays_per_call"] = bool(ms + order_s * 1e3 < base_ms)
            rec["break_even_hops"] = order_s * 1e3 / gain_ms_per_hop if gain_ms_per_hop > 0 else None
        rec.update(extra)
        res.append(rec)
        print(json.dumps(rec), flush=True)
    del gn, X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    pc = synth.CONFIGS["products"]
    ac = synth.CONFIGS["arxiv"]
    res = []
    new = ("community", None)
    rcm = ("rcm", lambda gn: gdd.graph.locality_order(gn, "rcm"))
    for shuffle in (True, False):
        g, perm = synth.sbm_device(pc.n, pc.avg_degree, 11, block=2048, p_in=0.9, shuffle=shuffle,
                                   return_perm=True)
        orders = [("original", None), new]
        if shuffle:  # node perm[i] sits in block i // 2048: the true community order puts it at row i
            def true_order(gn, perm=perm):
                rho = torch.empty(gn.n, dtype=torch.int32, device="cuda")
                rho[perm] = torch.arange(gn.n, dtype=torch.int32, device="cuda")
                return rho
            orders += [("true community order", true_order), rcm]
        run(f"products-shape SBM ({'shuffled ids' if shuffle else 'contiguous blocks'})", g, pc.d, pc.T,
            pc.alpha, orders, res)
        del g, perm
        torch.cuda.empty_cache()
    g = synth.chung_lu_device(pc.n, pc.avg_degree, pc.seed)
    run("products chung-lu (bench graph)", g, pc.d, pc.T, pc.alpha, [("original", None), new], res)
    del g
    torch.cuda.empty_cache()
    g = synth.sbm_device(ac.n, ac.avg_degree, 7, block=1024, p_in=0.9, shuffle=True)
    run("arxiv-shape SBM (shuffled ids)", g, ac.d, ac.T, ac.alpha, [("original", None), new], res)
    doc = {"tool": "tools/community_order.py", "reps": REPS, "device": torch.cuda.get_device_name(0),
           "records": res}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
    print(json.dumps({"summary": [(r["graph"], r["order"], round(r["us_per_hop"], 1),
                                  round(r["order_build_s"], 4)) for r in res]}), flush=True)


if __name__ == "__main__":
    main()
