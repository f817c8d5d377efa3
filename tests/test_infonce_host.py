"""CPU checks for the contrastive loss and the ablation switches: the dense fp64 definitions of
tests/infonce_ref.py reproduce the fixture recorded from the reference (tests/golden/rankformer_cl.npz)
to fp64 rounding, which anchors the yardstick of the device tests in the reference; the command line
takes every new flag with the reference's defaults; the host-side validation of the new entry points."""
import numpy as np
import pytest
import torch

import infonce_ref as N
import rankformer_ref as R


def _close64(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    scale = max(1.0, float(np.nanmax(np.abs(want)))) if want.size else 1.0
    err = float(np.nanmax(np.abs(got - want))) if np.isfinite(want).any() else 0.0
    assert err <= 1e-12 * scale, (what, err)


@pytest.mark.parametrize("name", N.NCE_CASES)
def test_dense_infonce_reproduces_reference_fp64(name):
    c = N.load_cl_case(name)
    tau = float(c["tau"])
    x = torch.from_numpy(c["x"]).double().requires_grad_(True)
    y = torch.from_numpy(c["y"]).double().requires_grad_(True)
    assert tuple(x.shape) == {"nce65": (65, 63), "nce300": (300, 64)}[name] and tau == 0.15
    loss = N.dense_infonce(x, y, tau)
    loss.backward()
    rows = c["rows"]
    _close64(loss.item(), c["loss64"], "loss")
    _close64(x.grad.numpy()[rows], c["gx64"], "gx")
    _close64(y.grad.numpy()[rows], c["gy64"], "gy")
    with torch.no_grad():
        xn, yn = torch.nn.functional.normalize(x), torch.nn.functional.normalize(y)
        _close64(N.dense_rows(xn, yn, tau).numpy()[rows], c["rows64"], "row losses")
    # the bound the device test takes from these is not vacuous
    assert all(float(c[k]) > 0 for k in ("loss32_err", "gx32_err", "gy32_err", "rows32_err"))


@pytest.mark.parametrize("name", N.LAYER_CASES)
def test_dense_switches_reproduce_reference_fp64(name):
    c = N.load_cl_case(name)
    base = R.load_case(name.split("_")[0])
    sw = [bool(v) for v in c["switches"]]
    M = R.mask_of(base["u"], base["i"], int(base["n"]), int(base["m"]))
    x = torch.from_numpy(base["x"]).double().requires_grad_(True)
    with torch.no_grad():
        z = N.dense_rankformer(x, M, 2.0, 0.0, *sw)
    W = torch.from_numpy(base["W"]).double()
    rows = c["rows"]
    _close64(z.numpy()[rows], c["z64"], "z")
    # a 0/0 row (wide's item without users under del_neg) is NaN in the reference too: it stays out of
    # the dense loss, and the reference's NaN gradients (that item's own row) are not compared
    good = ~torch.isnan(z).any(1)
    assert int((~good).sum()) == (1 if name == "wide_neg" else 0)
    (N.dense_rankformer(x, M, 2.0, 0.0, *sw, rows=good) * W[good]).sum().backward()
    g = x.grad.numpy()[rows]
    ok = ~np.isnan(c["g64"])
    _close64(np.where(ok, g, np.nan), c["g64"], "g")
    assert float(c["z32_err"]) > 0 and float(c["g32_err"]) > 0


@pytest.mark.parametrize("case", R.CASES)
def test_switches_off_is_the_layer(case):
    c = R.load_case(case)
    M = R.mask_of(c["u"], c["i"], int(c["n"]), int(c["m"]))
    x = torch.from_numpy(c["x"]).double()
    for alpha, clamp in ((2.0, 0.0), (0.5, 0.6)):
        a, b = N.dense_rankformer(x, M, alpha, clamp), R.dense_rankformer(x, M, alpha, clamp)
        assert float((a - b).abs().max()) <= 1e-13 * max(1.0, float(b.abs().max()))


def test_parse_args_takes_the_reference_flags_and_defaults():
    from gdd import train_teacher as T
    a = T.parse_args([])
    assert (a.use_cl, a.cl_layer, a.cl_lambda, a.cl_eps, a.cl_tau) == (False, 1, 0.05, 0.1, 0.15)
    assert (a.del_neg, a.del_benchmark, a.del_omega_norm) == (False, False, False)
    a = T.parse_args(["--use_gcn", "--use_cl", "--cl_layer", "2", "--cl_lambda", "0.1", "--cl_eps", "0.2",
                      "--cl_tau", "0.3", "--del_neg", "--del_benchmark", "--del_omega_norm"])
    assert (a.use_cl, a.cl_layer, a.cl_lambda, a.cl_eps, a.cl_tau) == (True, 2, 0.1, 0.2, 0.3)
    assert a.del_neg and a.del_benchmark and a.del_omega_norm and a.use_gcn


def test_planted_case_overflows_without_the_maximum():
    """What the running-maximum test rests on: exp(ℓ) overflows fp32 in the planted rows, the fp64
    losses are finite and large."""
    for late in (False, True):
        A, Y = N.planted(late=late)
        L = N.logits(A, Y, 0.01)
        assert int(torch.isinf(torch.exp(L).sum(1)).sum()) >= 30
        rows = N.dense_rows(A.double(), Y.double(), 0.01)
        assert bool(torch.isfinite(rows).all()) and float(rows.max()) > 50


def test_entry_points_validate_on_the_host():
    """Bad sizes, d, inv_tau and null pointers are refused before any device work; B = 0 succeeds."""
    from gdd import _lib
    lib = _lib.load()
    assert lib.gdd_infonce_ws_bytes(17730, 64) == 0
    nulls = (None,) * 5  # rows: lse, diag, pd, R, ws; cols: lse, pd, G, C, ws

    def rows(B, d, inv_tau):
        return lib.gdd_infonce_rows(B, d, None, None, inv_tau, *nulls, 0, None)

    def cols(B, d, inv_tau):
        return lib.gdd_infonce_cols(B, d, None, None, inv_tau, *nulls, 0, None)

    assert rows(0, 64, 1.0) == 0 and cols(0, 64, 1.0) == 0
    for B, d, inv_tau in ((-1, 64, 1.0), (4, 0, 1.0), (4, 257, 1.0), (2 ** 31, 8, 1.0), (4, 8, 0.0),
                          (4, 8, float("nan"))):
        assert rows(B, d, inv_tau) != 0
        assert b"infonce_rows" in lib.gdd_last_error()
        assert cols(B, d, inv_tau) != 0
        assert b"infonce_cols" in lib.gdd_last_error()
    assert rows(4, 8, 1.0) != 0
    assert b"null pointer" in lib.gdd_last_error()
    assert cols(4, 8, 1.0) != 0
    assert b"null pointer" in lib.gdd_last_error()
