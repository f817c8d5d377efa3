"""Record tests/golden/rankformer_layer.npz from the reference Rankformer code (CPU, data only).

    python tools/make_golden_rankformer.py --reference <checkout>/Rankformer/code

Imports the reference's ``rec.py`` (its ``parse.py`` reads ``sys.argv`` at import, so argv is set
first) and runs its ``Rankformer`` and ``GCN`` layers on two small cases:

* ``small``: 37 users x 29 items, d = 8;  * ``wide``: 61 users x 45 items, d = 64;

both at density about 0.15 with the edge cases forced in: user 0 has no positives and user 1 holds
every item it can. An item without users cannot coexist with a user that holds every item, so the
two are split: ``small`` has the user with all 29 items (d⁻ clamped at 1), ``wide`` has item 2 with
no user and user 1 holding the 44 others.

Per case (keys prefixed ``<case>_``): ``n``, ``m``, ``u``, ``i`` (the distinct pairs), ``x`` and
``W`` (fp64 arrays whose values are exactly representable in fp32), the reference layer's output
``z64`` / ``z32`` (run in fp64 / fp32), the GCN layer's ``gcn64`` / ``gcn32`` (left 1, right 0) and
``gcnb64`` / ``gcnb32`` (left 0.5, right 0.5), and for the loss ``sum(z * W)`` the reference's
gradient with respect to x, ``g64`` / ``g32``. alpha = 2, clamp = 0 (parse.py's defaults).
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_pairs(n, m, density, rng, empty_item):
    M = rng.random_sample((n, m)) < density
    M[0, :] = False
    M[1, :] = True
    if empty_item is not None:
        M[:, empty_item] = False
    M[2:, 0] |= ~M[2:].any(axis=1)  # every other user keeps at least one item
    u, i = np.nonzero(M)
    return u.astype(np.int64), i.astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's Rankformer/code directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rankformer_layer.npz"))
    a = ap.parse_args()
    sys.argv = ["main.py", "--device", "-1"]
    sys.path.insert(0, a.reference)
    import rec  # noqa: E402  (the reference layer)

    out = {}
    for name, n, m, d, empty_item, seed in (("small", 37, 29, 8, None, 11), ("wide", 61, 45, 64, 2, 12)):
        rng = np.random.RandomState(seed)
        u, i = make_pairs(n, m, 0.15, rng, empty_item)
        x = (0.1 * rng.standard_normal((n + m, d))).astype(np.float32).astype(np.float64)
        W = rng.standard_normal((n + m, d)).astype(np.float32).astype(np.float64)
        ds = types.SimpleNamespace(num_users=n, num_items=m)
        ut, it = torch.from_numpy(u), torch.from_numpy(i)
        out.update({f"{name}_n": np.int64(n), f"{name}_m": np.int64(m), f"{name}_u": u.astype(np.int32),
                    f"{name}_i": i.astype(np.int32), f"{name}_x": x, f"{name}_W": W})
        for tag, dt in (("64", torch.float64), ("32", torch.float32)):
            # the GCN layer builds its weights from integer degrees in the default dtype
            torch.set_default_dtype(dt)
            xt = torch.from_numpy(x).to(dt).requires_grad_(True)
            z = rec.Rankformer(ds, rec.args.rankformer_alpha)(xt, ut, it)
            (z * torch.from_numpy(W).to(dt)).sum().backward()
            out[f"{name}_z{tag}"] = z.detach().numpy()
            out[f"{name}_g{tag}"] = xt.grad.numpy()
            with torch.no_grad():
                out[f"{name}_gcn{tag}"] = rec.GCN(ds, 1.0, 0.0)(xt.detach(), ut, it).numpy()
                out[f"{name}_gcnb{tag}"] = rec.GCN(ds, 0.5, 0.5)(xt.detach(), ut, it).numpy()
    torch.set_default_dtype(torch.float32)
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
