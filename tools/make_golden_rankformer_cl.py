"""Record tests/golden/rankformer_cl.npz from the reference Rankformer code (CPU, data only): the
contrastive loss and the layer's three ablation switches.

    python tools/make_golden_rankformer_cl.py --reference <checkout>/Rankformer/code

Imports the reference's ``model.py`` and ``rec.py`` (``parse.py`` reads ``sys.argv`` at import, so argv
is set first; the switches are ``args`` attributes set before each call). Keys are ``<case>.<field>``.

* ``nce65`` (B, d, tau) = (65, 63, 0.15) and ``nce300`` = (300, 64, 0.15): the reference ``InfoNCE``
  (model.py:10-24) on ``x = 0.1 randn``, ``y = x + 0.01 randn`` (stored as fp32). ``loss64``, and for
  the gradients of the loss ``gx64``, ``gy64`` and of the row losses ``rows64`` (fp64 runs); the
  reference's own fp32 errors on the same input as scalars ``loss32_err``, ``gx32_err``, ``gy32_err``,
  ``rows32_err`` (max |fp32 run − fp64 run| over all elements).
* ``<pairs>_<switch>`` for pairs in ``small``, ``wide`` (the pairs, ``x`` and ``W`` of
  rankformer_layer.npz) and switch in ``neg``, ``bench``, ``norm``, ``all``: the reference layer
  (rec.py:143-274) with ``del_neg`` / ``del_benchmark`` / ``del_omega_norm`` / all three set, alpha = 2,
  clamp = 0: ``z64``, the gradient ``g64`` of ``sum(z * W)`` with respect to x, and the reference's
  fp32 errors ``z32_err``, ``g32_err`` over all elements. ``wide`` has an item without users: with
  ``del_neg`` at clamp 0 its row is 0/0 in the reference, in fp64 and fp32 alike. Those NaN are
  stored as they are and the errors are over the other elements.

To keep the file small, an fp64 array of more than 70 rows is stored for every 8th row only
(``<case>.rows`` lists them; the errors are over all rows). tests/test_infonce_host.py checks that the
dense definitions of tests/infonce_ref.py reproduce the stored rows to fp64 rounding, so the device
tests compare every row against those definitions. A file that already holds exactly these arrays is
left as it is.
"""
import argparse
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCE_CASES = {"nce65": (65, 63, 0.15, 31), "nce300": (300, 64, 0.15, 32)}  # B, d, tau, seed
SWITCHES = {"neg": (True, False, False), "bench": (False, True, False), "norm": (False, False, True),
            "all": (True, True, True)}  # del_neg, del_benchmark, del_omega_norm


def stored_rows(n):
    return np.arange(n, dtype=np.int64) if n <= 70 else np.arange(0, n, 8, dtype=np.int64)


def run_infonce(model, x, y, tau):
    res = {}
    for dt in (torch.float64, torch.float32):
        xt = torch.from_numpy(x).to(dt).requires_grad_(True)
        yt = torch.from_numpy(y).to(dt).requires_grad_(True)
        loss = model.InfoNCE(xt, yt, tau)
        loss.backward()
        with torch.no_grad():  # the row losses: the same expression without the mean
            xn, yn = torch.nn.functional.normalize(xt), torch.nn.functional.normalize(yt)
            rows = -torch.diag(torch.nn.functional.log_softmax((xn @ yn.T) / tau, dim=1))
        res[dt] = [np.float64(loss.item()), xt.grad.numpy().astype(np.float64),
                   yt.grad.numpy().astype(np.float64), rows.numpy().astype(np.float64)]
    return res[torch.float64], res[torch.float32]


def run_layer(rec, u, i, n, m, x, W, switches):
    ds = types.SimpleNamespace(num_users=n, num_items=m)
    ut, it = torch.from_numpy(u), torch.from_numpy(i)
    rec.args.del_neg, rec.args.del_benchmark, rec.args.del_omega_norm = switches
    res = {}
    for dt in (torch.float64, torch.float32):
        torch.set_default_dtype(dt)
        x0 = torch.from_numpy(x).to(dt).requires_grad_(True)
        z = rec.Rankformer(ds, 2.0)(x0, ut, it)
        (z * torch.from_numpy(W).to(dt)).sum().backward()
        res[dt] = (z.detach().numpy().astype(np.float64), x0.grad.numpy().astype(np.float64))
    torch.set_default_dtype(torch.float32)
    rec.args.del_neg = rec.args.del_benchmark = rec.args.del_omega_norm = False
    return res[torch.float64], res[torch.float32]


def same_arrays(path, out):
    if not os.path.exists(path):
        return False
    old = np.load(path)
    return sorted(old.files) == sorted(out) and all(
        old[k].dtype == np.asarray(out[k]).dtype and np.array_equal(old[k], out[k]) for k in out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's Rankformer/code directory")
    ap.add_argument("--layer", default=os.path.join(ROOT, "tests", "golden", "rankformer_layer.npz"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "rankformer_cl.npz"))
    a = ap.parse_args()
    sys.argv = ["main.py", "--device", "-1"]
    sys.path.insert(0, a.reference)
    import model  # noqa: E402  (the reference InfoNCE)
    import rec  # noqa: E402  (the reference layer)

    out = {}
    for name, (B, d, tau, seed) in NCE_CASES.items():
        rng = np.random.RandomState(seed)
        x = (0.1 * rng.standard_normal((B, d))).astype(np.float32)
        y = (x + 0.01 * rng.standard_normal((B, d))).astype(np.float32)
        (l64, gx64, gy64, r64), (l32, gx32, gy32, r32) = run_infonce(model, x, y, tau)
        rows = stored_rows(B)
        errs = {"loss32_err": abs(l32 - l64), "gx32_err": np.abs(gx32 - gx64).max(),
                "gy32_err": np.abs(gy32 - gy64).max(), "rows32_err": np.abs(r32 - r64).max()}
        out.update({f"{name}.x": x, f"{name}.y": y, f"{name}.tau": np.float64(tau), f"{name}.rows": rows,
                    f"{name}.loss64": l64, f"{name}.gx64": gx64[rows], f"{name}.gy64": gy64[rows],
                    f"{name}.rows64": r64[rows]})
        out.update({f"{name}.{k}": np.float64(v) for k, v in errs.items()})
        print(name, " ".join(f"{k}={v:.3e}" for k, v in errs.items()))
        assert all(v > 0 for v in errs.values()), "a zero reference error would make a zero bound"

    layer = np.load(a.layer)
    for base in ("small", "wide"):
        n, m = int(layer[f"{base}_n"]), int(layer[f"{base}_m"])
        u, i = layer[f"{base}_u"].astype(np.int64), layer[f"{base}_i"].astype(np.int64)
        x, W = layer[f"{base}_x"], layer[f"{base}_W"]
        rows = stored_rows(n + m)
        for tag, sw in SWITCHES.items():
            (z64, g64), (z32, g32) = run_layer(rec, u, i, n, m, x, W, sw)
            name = f"{base}_{tag}"
            # wide's item without users is 0/0 under del_neg at clamp 0, in the reference too
            assert np.array_equal(np.isnan(z32), np.isnan(z64)) and np.array_equal(np.isnan(g32), np.isnan(g64))
            print(f"{name}: {int(np.isnan(z64).sum())} NaN outputs, {int(np.isnan(g64).sum())} NaN gradients")
            ze, ge = np.nanmax(np.abs(z32 - z64)), np.nanmax(np.abs(g32 - g64))
            out.update({f"{name}.switches": np.asarray(sw, np.int64), f"{name}.rows": rows,
                        f"{name}.z64": z64[rows], f"{name}.g64": g64[rows], f"{name}.z32_err": np.float64(ze),
                        f"{name}.g32_err": np.float64(ge)})
            print(f"{name}: reference fp32 error {ze:.3e} (output), {ge:.3e} (gradient)")
            assert ze > 0 and ge > 0
    if same_arrays(a.out, out):
        print(f"{a.out}: holds these arrays already, left as it is")
    else:
        np.savez_compressed(a.out, **out)
        print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
