"""Record tests/golden/rankformer_layer.npz and rankformer_layer_more.npz from the reference
Rankformer code (CPU, data only).

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
gradient with respect to x, ``g64`` / ``g32``. alpha = 2, clamp = 0 (parse.py's defaults). A file
that already holds exactly these arrays is left as it is (an .npz carries the time it was written).

The second file (``--more-out``, keys ``<case>.<field>``; the cases are tests/rankformer_ref.py's
``MORE_CASES``) holds the settings the first does not reach, as ``alpha``, ``clamp``, ``layers``,
``z64``, ``g64`` (fp64) and the reference's own fp32 error on the same input as two scalars,
``z32_err = max|z32 − z64|`` and ``g32_err``; a case stores ``n, m, u, i`` and ``x``, ``W`` (fp32)
only where they are not those of the case it runs on:

* ``small_c05``, ``small_c025``, ``wide_c05``, ``wide_c025``: the first file's pairs, ``x`` and ``W``
  at (alpha, clamp) = (0.5, 0.6) and (0.25, 0.3) (``args.rankformer_clamp_value`` set before the
  call), where the clamp is active on some and inactive on other rows of all three denominators;
* ``cut``, ``cut_c05``: 100 users x 80 items, d = 65, density 0.15, item 0 held by every user but
  the empty user 0, user 1 holding every item but the empty item 5: rows of both orientations are
  cut by the kernels' 32-entry chunks; at (2, 0) and (0.5, 0.6). The seed is the first from 0 for
  which the clamp conditions of ``rankformer_ref.clamp_conditions`` hold (``cut.seed``);
* ``small193``: the ``small`` pairs with a new ``x``, ``W`` of width 193, at (2, 0);
* ``stack2``: ``small`` at (2, 0), two applications blended as x <- (1 − tau) x + tau layer(x),
  tau = 0.5 (model.py:234); output and gradient with respect to the initial x.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rankformer_ref as R  # noqa: E402  (the dense definition: the cut case's seed search)


def make_pairs(n, m, density, rng, empty_item):
    M = rng.random_sample((n, m)) < density
    M[0, :] = False
    M[1, :] = True
    if empty_item is not None:
        M[:, empty_item] = False
    M[2:, 0] |= ~M[2:].any(axis=1)  # every other user keeps at least one item
    u, i = np.nonzero(M)
    return u.astype(np.int64), i.astype(np.int64)


def make_cut(seed, n=100, m=80, d=65):
    rng = np.random.RandomState(seed)
    M = rng.random_sample((n, m)) < 0.15
    M[:, 0] = True
    M[1, :] = True
    M[:, 5] = False
    M[0, :] = False
    u, i = np.nonzero(M)
    x = (0.1 * rng.standard_normal((n + m, d))).astype(np.float32)
    W = rng.standard_normal((n + m, d)).astype(np.float32)
    return u.astype(np.int64), i.astype(np.int64), n, m, x, W


def conditions_hold(u, i, n, m, x, alpha, clamp):
    counts, gap = R.clamp_conditions(torch.from_numpy(x.astype(np.float64)), R.mask_of(u, i, n, m), alpha, clamp)
    return all(0 < k < total for k, total in counts) and gap >= 1e-4


def run_reference(rec, u, i, n, m, x, W, alpha, clamp, layers):
    """(z64, g64, z32_err, g32_err) of the reference layer (``layers`` > 1: the model's blend)."""
    ds = types.SimpleNamespace(num_users=n, num_items=m)
    ut, it = torch.from_numpy(u), torch.from_numpy(i)
    rec.args.rankformer_clamp_value = clamp
    res = {}
    for dt in (torch.float64, torch.float32):
        torch.set_default_dtype(dt)
        x0 = torch.from_numpy(x).to(dt).requires_grad_(True)
        layer = rec.Rankformer(ds, alpha)
        z = x0
        if layers == 1:
            z = layer(z, ut, it)
        else:
            for _ in range(layers):
                z = (1 - R.TAU) * z + R.TAU * layer(z, ut, it)
        (z * torch.from_numpy(W).to(dt)).sum().backward()
        res[dt] = (z.detach().numpy().astype(np.float64), x0.grad.numpy().astype(np.float64))
    torch.set_default_dtype(torch.float32)
    rec.args.rankformer_clamp_value = 0
    (z64, g64), (z32, g32) = res[torch.float64], res[torch.float32]
    return z64, g64, np.float64(np.abs(z32 - z64).max()), np.float64(np.abs(g32 - g64).max())


def same_arrays(path, out):
    if not os.path.exists(path):
        return False
    old = np.load(path)
    return sorted(old.files) == sorted(out) and all(
        old[k].dtype == np.asarray(out[k]).dtype and np.array_equal(old[k], out[k]) for k in out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's Rankformer/code directory")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rankformer_layer.npz"))
    ap.add_argument("--more-out", default=os.path.join(ROOT, "tests", "golden", "rankformer_layer_more.npz"))
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
    if same_arrays(a.out, out):
        print(f"{a.out}: holds these arrays already, left as it is")
    else:
        np.savez_compressed(a.out, **out)
        print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")

    # ---- the second file -------------------------------------------------------------------------
    data = {}  # pairs case -> (u, i, n, m, x, W) with x, W fp32
    for name in R.CASES:
        data[name] = (out[f"{name}_u"].astype(np.int64), out[f"{name}_i"].astype(np.int64), int(out[f"{name}_n"]),
                      int(out[f"{name}_m"]), out[f"{name}_x"].astype(np.float32), out[f"{name}_W"].astype(np.float32))
    seed = next(s for s in range(10000) if conditions_hold(*make_cut(s)[:5], 0.5, 0.6))
    data["cut"] = make_cut(seed)
    rng = np.random.RandomState(13)
    su, si, sn, sm = data["small"][:4]
    data["small193"] = (su, si, sn, sm, (0.1 * rng.standard_normal((sn + sm, 193))).astype(np.float32),
                        rng.standard_normal((sn + sm, 193)).astype(np.float32))
    more = {"cut.seed": np.int64(seed)}
    for name, (base, alpha, clamp, layers) in R.MORE_CASES.items():
        u, i, n, m, x, W = data[name if name in data else base]
        if name in data:  # the case brings its own pairs or inputs
            more.update({f"{name}.x": x, f"{name}.W": W})
            if base == name:
                more.update({f"{name}.n": np.int64(n), f"{name}.m": np.int64(m), f"{name}.u": u.astype(np.int32),
                             f"{name}.i": i.astype(np.int32)})
        if clamp > 0:
            assert conditions_hold(u, i, n, m, x, alpha, clamp), name
        z64, g64, z32_err, g32_err = run_reference(rec, u, i, n, m, x, W, alpha, clamp, layers)
        more.update({f"{name}.alpha": np.float64(alpha), f"{name}.clamp": np.float64(clamp),
                     f"{name}.layers": np.int64(layers), f"{name}.z64": z64, f"{name}.g64": g64,
                     f"{name}.z32_err": z32_err, f"{name}.g32_err": g32_err})
        print(f"{name}: reference fp32 error {z32_err:.3e} (output), {g32_err:.3e} (gradient)")
    if same_arrays(a.more_out, more):
        print(f"{a.more_out}: holds these arrays already, left as it is (cut seed {seed})")
    else:
        np.savez_compressed(a.more_out, **more)
        print(f"wrote {a.more_out}: {os.path.getsize(a.more_out)} bytes (cut seed {seed})")


if __name__ == "__main__":
    main()
