"""The contrastive loss on the MI355X (csrc/gdd_infonce.hip, gdd.rankformer.infonce_rows / infonce):
the two passes against the dense fp64 definitions of tests/infonce_ref.py under the forward bounds
derived in that module's docstring (u = 2^-24, no fitted constant), the running maximum on planted
logits of 100, autograd with a mixed-sign upstream gradient, the fixture recorded from the
reference (within 4 x the reference's own fp32 error, this project's margin for "the same sums in
another order"), determinism, peak memory (no B x B object), no_grad and B = 0.

Every output buffer of the kernel tests is pre-filled with NaN, so an unwritten element shows. Each
test prints its largest error / bound ratio."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infonce_ref as N  # noqa: E402

pytestmark = pytest.mark.gpu

TAU = 0.15
# every B of {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 300} and every d of
# {1, 8, 63, 64, 65, 128, 129, 193, 256}: tile edges of the 32-row tiles and the 128-row workgroups,
# and every feature instantiation (32, 64, 128, 192, 256) at and beside its edge
SHAPES = [(1, 1), (1, 256), (2, 8), (2, 129), (31, 63), (32, 64), (33, 65), (33, 8), (63, 128), (64, 129),
          (65, 193), (127, 256), (128, 1), (128, 64), (129, 193), (129, 63), (300, 64), (300, 65), (300, 256)]


def nan_buf(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")


def raw_passes(A, Y, tau, G):
    """Both entry points through the C ABI into NaN-filled buffers: (lse, diag, pd, R, C)."""
    from gdd import _lib
    lib = _lib.device_lib()
    B, d = A.shape
    a, y, g = A.cuda().contiguous(), Y.cuda().contiguous(), G.cuda().contiguous()
    lse, diag, pd, R, C = nan_buf(B), nan_buf(B), nan_buf(B), nan_buf(B, d), nan_buf(B, d)
    ws = _lib.workspace(lib.gdd_infonce_ws_bytes(B, d), "cuda")
    s = _lib.stream_ptr("cuda")
    _lib.check(lib.gdd_infonce_rows(B, d, a.data_ptr(), y.data_ptr(), 1.0 / tau, lse.data_ptr(), diag.data_ptr(),
                                    pd.data_ptr(), R.data_ptr(), ws.data_ptr(), ws.numel(), s))
    _lib.check(lib.gdd_infonce_cols(B, d, a.data_ptr(), y.data_ptr(), 1.0 / tau, lse.data_ptr(), pd.data_ptr(),
                                    g.data_ptr(), C.data_ptr(), ws.data_ptr(), ws.numel(), s))
    torch.cuda.synchronize()
    return lse.cpu(), diag.cpu(), pd.cpu(), R.cpu(), C.cpu()


def within(name, got, exact, bound):
    got, exact, bound = (torch.as_tensor(t, dtype=torch.float64) for t in (got, exact, bound))
    assert bool(torch.isfinite(got).all()), f"{name}: an element is not finite (unwritten?)"
    err = (got - exact).abs()
    ratio = float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0
    print(f"{name}: max err/bound = {ratio:.3f}")
    assert bool((err <= bound).all()), (name, ratio)
    return ratio


def mixed_G(B, seed):
    g = torch.Generator().manual_seed(seed)
    G = torch.randn(B, generator=g)
    G[::5] = 0.0
    return G


def check_passes(tag, A, Y, tau, G):
    lse, diag, pd, R, C = raw_passes(A, Y, tau, G)
    A64, Y64, G64 = A.double(), Y.double(), G.double()
    within(f"{tag} loss", lse.double() - diag.double(), N.dense_rows(A64, Y64, tau), N.bound_rows(A64, Y64, tau))
    P_rr = torch.diagonal(N.dense_P(A64, Y64, tau))
    within(f"{tag} pd", pd, P_rr, N.rel_factor(A64, Y64, tau) * P_rr + N.U)
    within(f"{tag} R", R, N.dense_R(A64, Y64, tau), N.bound_R(A64, Y64, tau))
    within(f"{tag} C", C, N.dense_C(A64, Y64, tau, G64), N.bound_C(A64, Y64, tau, G64))


@pytest.mark.parametrize("B,d", SHAPES)
def test_passes_vs_fp64(B, d):
    A, Y = N.unit_rows(B, d, 1000 * B + d)
    check_passes(f"B={B} d={d}", A, Y, TAU, mixed_G(B, B + d))


@pytest.mark.parametrize("late", [False, True], ids=["early", "late"])
def test_running_maximum(late):
    """Logits of 100 off the diagonal at tau = 0.01: a sum of exp(l) without the maximum overflows
    (tests/test_infonce_host.py); the kernel's losses, R and C are finite and within the bounds."""
    A, Y = N.planted(130, 64, late)
    assert float(N.dense_rows(A.double(), Y.double(), 0.01).max()) > 50
    check_passes(f"planted late={late}", A, Y, 0.01, mixed_G(130, 7))


@pytest.mark.parametrize("B,d", [(65, 63), (129, 193), (300, 64)])
def test_autograd_rows(B, d):
    from gdd import rankformer as RF
    A, Y = N.unit_rows(B, d, 77 + B)
    G = mixed_G(B, 3 * B)
    a, y = A.cuda().requires_grad_(True), Y.cuda().requires_grad_(True)
    rows = RF.infonce_rows(a, y, TAU)
    rows.backward(G.cuda())
    A64, Y64 = A.double().requires_grad_(True), Y.double().requires_grad_(True)
    ref = N.dense_rows(A64, Y64, TAU)
    ref.backward(G.double())
    Ad, Yd, Gd = A.double(), Y.double(), G.double()
    tag = f"autograd B={B} d={d}"
    within(f"{tag} rows", rows.detach().cpu(), ref.detach(), N.bound_rows(Ad, Yd, TAU))
    within(f"{tag} dA", a.grad.cpu(), A64.grad, N.bound_dA(Ad, Yd, TAU, Gd))
    within(f"{tag} dY", y.grad.cpu(), Y64.grad, N.bound_dY(Ad, Yd, TAU, Gd))
    assert not a.grad.cpu()[G == 0].any()  # a zero upstream gradient gives a zero row of dA


@pytest.mark.parametrize("B,d", [(65, 63), (300, 64)])
def test_autograd_infonce(B, d):
    """The model-level function (fp32 normalisation in torch, then the passes, then the mean) against
    fp64 autograd of the dense definition, un-normalised inputs of mixed row lengths."""
    from gdd import rankformer as RF
    g = torch.Generator().manual_seed(B)
    x = (torch.randn(B, d, generator=g) * (0.05 + torch.rand(B, 1, generator=g))).float()
    y = (x + 0.05 * torch.randn(B, d, generator=g)).float()
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    loss = RF.infonce(xd, yd, TAU)
    loss.backward()
    x64, y64 = x.double().requires_grad_(True), y.double().requires_grad_(True)
    ref = N.dense_infonce(x64, y64, TAU)
    ref.backward()
    lb, bx, by = N.bounds_infonce(x.double(), y.double(), TAU)
    tag = f"infonce B={B} d={d}"
    within(f"{tag} loss", loss.detach().cpu(), ref.detach(), torch.tensor(lb))
    within(f"{tag} dx", xd.grad.cpu(), x64.grad, bx)
    within(f"{tag} dy", yd.grad.cpu(), y64.grad, by)
    # b_cos=False is the rows' mean as it stands
    assert torch.equal(RF.infonce(xd.detach(), yd.detach(), TAU, b_cos=False),
                       RF.infonce_rows(xd.detach(), yd.detach(), TAU).mean())


@pytest.mark.parametrize("name", N.NCE_CASES)
def test_fixture(name):
    """The reference's two recorded cases through infonce: loss and both gradients within 4 x the
    reference's own fp32 error of the fp64 values. The fixture stores every 8th row of the larger
    case; the dense definition reproduces the stored rows to fp64 rounding (test_infonce_host.py) and
    stands in for the others."""
    from gdd import rankformer as RF
    c = N.load_cl_case(name)
    tau = float(c["tau"])
    x = torch.from_numpy(c["x"]).cuda().requires_grad_(True)
    y = torch.from_numpy(c["y"]).cuda().requires_grad_(True)
    loss = RF.infonce(x, y, tau)
    loss.backward()
    x64 = torch.from_numpy(c["x"]).double().requires_grad_(True)
    y64 = torch.from_numpy(c["y"]).double().requires_grad_(True)
    N.dense_infonce(x64, y64, tau).backward()
    rows = c["rows"]
    assert np.allclose(x64.grad.numpy()[rows], c["gx64"], rtol=0, atol=1e-14)
    for what, got, want, err in (("loss", loss.item(), float(c["loss64"]), float(c["loss32_err"])),
                                 ("gx", x.grad.cpu().double().numpy(), x64.grad.numpy(), float(c["gx32_err"])),
                                 ("gy", y.grad.cpu().double().numpy(), y64.grad.numpy(), float(c["gy32_err"]))):
        ratio = float(np.max(np.abs(np.asarray(got) - np.asarray(want)))) / err
        print(f"{name} {what}: max err / reference fp32 err = {ratio:.3f}")
        assert ratio <= 4.0, (name, what, ratio)


@pytest.mark.parametrize("B,d", [(300, 64), (129, 193)])
def test_two_runs_same_bits(B, d):
    A, Y = N.unit_rows(B, d, 9)
    G = mixed_G(B, 1)
    one, two = raw_passes(A, Y, TAU, G), raw_passes(A, Y, TAU, G)
    for name, p, q in zip(("lse", "diag", "pd", "R", "C"), one, two):
        assert torch.equal(p.view(torch.int32), q.view(torch.int32)), name


def test_no_bxb_object():
    """Forward and backward at B = 4096, d = 16 allocate less than 8 MB above the level before the
    call: the logits alone would be 67 MB; A, Y, R, C and the gradients together are under 2 MB."""
    from gdd import rankformer as RF
    B, d = 4096, 16
    A, Y = N.unit_rows(B, d, 2)
    a, y = A.cuda().requires_grad_(True), Y.cuda().requires_grad_(True)
    RF.infonce_rows(a[:8], y[:8], TAU).sum().backward()  # the library is loaded, the allocator warm
    a.grad = y.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    RF.infonce_rows(a, y, TAU).mean().backward()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - before
    print(f"peak above the level before the call: {extra / 1e6:.2f} MB")
    assert extra < 8e6
    assert bool(torch.isfinite(a.grad).all()) and bool(torch.isfinite(y.grad).all())


def test_no_grad_skips_R(monkeypatch):
    from gdd import rankformer as RF
    A, Y = N.unit_rows(65, 63, 4)
    a, y = A.cuda(), Y.cuda()
    seen = []
    real = RF.infonce_row_pass

    def spy(a_, y_, tau, want_R=True):
        out = real(a_, y_, tau, want_R)
        seen.append((want_R, out[2] is None and out[3] is None))
        return out

    monkeypatch.setattr(RF, "infonce_row_pass", spy)
    with_grad = RF.infonce_rows(a.clone().requires_grad_(True), y, TAU)
    with torch.no_grad():
        without = RF.infonce_rows(a.clone().requires_grad_(True), y, TAU)
    plain = RF.infonce_rows(a, y, TAU)  # neither input needs a gradient
    assert seen == [(True, False), (False, True), (False, True)]
    assert torch.equal(with_grad.detach(), without) and torch.equal(without, plain)
    assert not without.requires_grad


def test_empty_batch():
    from gdd import _lib, rankformer as RF
    lib = _lib.device_lib()
    e = torch.zeros(0, 8, device="cuda", requires_grad=True)
    rows = RF.infonce_rows(e, e.detach(), TAU)
    assert rows.shape == (0,)
    rows.sum().backward()
    assert e.grad.shape == (0, 8)
    assert lib.gdd_infonce_rows(0, 8, None, None, 1.0, None, None, None, None, None, 0, None) == 0
    with pytest.raises(ValueError):
        RF.infonce_rows(torch.zeros(4, 257, device="cuda"), torch.zeros(4, 257, device="cuda"), TAU)
    with pytest.raises(ValueError):
        RF.infonce_rows(torch.zeros(4, 8, device="cuda"), torch.zeros(5, 8, device="cuda"), TAU)
