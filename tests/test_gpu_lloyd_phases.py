"""The Lloyd loop's phase entry points (gdd_lloyd_estep / _mstep / _update) on one GPU.

* The convergence test's numpy pairwise sum of the squared centre shifts, evaluated by the workgroup
  (leaves in parallel, r04): with tol set to numpy's own float32 sum S, the loop stops (reason 2);
  with tol one ulp below S it does not — for k across the leaf-layout cases (fewer than 8 values, one
  leaf, leaf boundaries, many leaves).
* The M-step over a feature-column range equals the corresponding columns of the full fold, for the
  small-cluster (8 KiB chunk) and the regular fold buffers.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O

pytestmark = pytest.mark.gpu

from gdd import _lib  # noqa: E402


@pytest.mark.parametrize("k", [1, 5, 7, 8, 9, 100, 128, 129, 135, 604, 1000, 1773, 5000, 8192])
def test_update_convergence_sum_is_numpys(k):
    lib = _lib.device_lib()
    dim, n = 3, 16
    rng = np.random.default_rng(k)
    C_old = rng.standard_normal((k, dim)).astype(np.float32)
    C_new = (C_old + rng.standard_normal((k, dim)).astype(np.float32) * np.float32(1e-3)
             * rng.random((k, 1)).astype(np.float32) ** 4).astype(np.float32)
    wsum = np.ones(k, np.float32)  # averaging by 1/1 leaves C_new as it is
    dev = "cuda"
    shift = torch.empty(k, dtype=torch.float32, device=dev)
    labels = torch.zeros(n, dtype=torch.int32, device=dev)
    res = []
    for pick in ("at", "below"):
        Cn = torch.from_numpy(C_new.copy()).to(dev)
        Co = torch.from_numpy(C_old).to(dev)
        w = torch.from_numpy(wsum).to(dev)
        labels_old = torch.full((n,), -1, dtype=torch.int32, device=dev)  # changed: the tol test decides
        state = torch.zeros(lib.gdd_lloyd_state_bytes(), dtype=torch.uint8, device=dev)
        # first pass with tol = -1 (never stops) to read the shifts the device computes
        _lib.check(lib.gdd_lloyd_update(n, dim, k, None, 1, Cn.data_ptr(), w.data_ptr(), Co.data_ptr(),
                                        shift.data_ptr(), labels.data_ptr(), labels_old.data_ptr(), -1.0,
                                        state.data_ptr(), 0, _lib.stream_ptr()))
        sh = shift.cpu().numpy()
        S = float(np.sum(sh * sh, dtype=np.float32))  # numpy's pairwise float32 sum
        tol = S if pick == "at" else float(np.nextafter(np.float32(S), np.float32(0)))
        Cn = torch.from_numpy(C_new.copy()).to(dev)
        labels_old = torch.full((n,), -1, dtype=torch.int32, device=dev)
        state = torch.zeros(lib.gdd_lloyd_state_bytes(), dtype=torch.uint8, device=dev)
        _lib.check(lib.gdd_lloyd_update(n, dim, k, None, 1, Cn.data_ptr(), w.data_ptr(), Co.data_ptr(),
                                        shift.data_ptr(), labels.data_ptr(), labels_old.data_ptr(), tol,
                                        state.data_ptr(), 0, _lib.stream_ptr()))
        st = state[:20].view(torch.int32).cpu().numpy()
        res.append((int(st[0]), int(st[1])))
    assert res[0] == (2, 2), res  # stop_at = step 1 + 1, reason 2 (tol)
    assert res[1] == (0, 0), res


W, MEAN, X_UNALIGNED = 1, 2, 4  # gdd.h GDD_FOLD_*


def _fold_case(n, dim, k, seed, sizes=None):
    """X (device rows start one float past a 16-byte boundary when asked), labels with no empty cluster
    (sizes: the clusters' shares, else uniform), weights."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    lab = (rng.choice(k, n, p=np.asarray(sizes) / np.sum(sizes)) if sizes else rng.integers(0, k, n)).astype(np.int32)
    lab[:k] = np.arange(k)
    w = (rng.random(n) + 0.5).astype(np.float32)
    return X, lab, w


# one shape per kernel form of the ordered fold that gdd_segment_sum_f32 / gdd_cluster_mean reach
# (tests/test_lloyd_plan_host.py pins the names on the host): the smallest that take the form
@pytest.mark.parametrize("n,dim,k,flags,path", [
    (3000, 8, 5, 0, "cm/8x1024"),
    (3000, 64, 5, 0, "cm/64x256"),
    (2000, 68, 4, 0, "seg/f32/vec/1x240"),
    (2000, 7, 4, 0, "seg/f32/scalar/1x1024"),
    (3000, 64, 5, X_UNALIGNED, "seg/f32/scalar/1x256"),
    (3000, 64, 5, W, "seg/f32/vec/w/1x256"),
    (1500, 192, 3, W, "seg/f32/vec/w/1x80"),
    (1500, 193, 3, W, "seg/f32/scalar/w/2x80"),
    (1500, 196, 3, W, "seg/f32/vec/w/2x80"),
    (1200, 256, 3, 0, "seg/f32/vec/1x64"),
    (1200, 257, 3, 0, "seg/f32/scalar/2x64"),
    (1200, 260, 3, 0, "seg/f32/vec/2x64"),
    (600, 12, 60, 0, "seg/f32/vec/small/1x160"),
    (600, 13, 60, 0, "seg/f32/scalar/small/1x144"),
    (600, 12, 60, W, "seg/f32/vec/w/small/1x160"),
    (600, 13, 60, W, "seg/f32/scalar/w/small/1x144"),
    (600, 132, 60, 0, "seg/f32/vec/1x112"),
    (2000, 128, 40, MEAN, "seg/mean/vec/1x64"),
    (2000, 47, 40, MEAN, "seg/mean/scalar/1x160"),
    (2000, 128, 40, MEAN | X_UNALIGNED, "seg/mean/scalar/1x64"),
    (2000, 300, 40, MEAN, "seg/mean/vec/2x32"),
])
def test_fold_forms_match_oracle(n, dim, k, flags, path):
    import gdd
    lib = _lib.device_lib()
    assert lib.gdd_fold_path(n, dim, 0, k, flags, 0).decode() == path
    X, lab, w = _fold_case(n, dim, k, n + dim + flags)
    off = 1 if flags & X_UNALIGNED else 0
    Xd = torch.empty(n * dim + 4, dtype=torch.float32, device="cuda")[off:off + n * dim].view(n, dim)
    Xd.copy_(torch.from_numpy(X))
    assert Xd.data_ptr() % 16 == (4 if off else 0)
    ld = torch.from_numpy(lab).cuda()
    perm, offs = gdd.group_by_label(ld, k)
    out = torch.empty(k, dim, dtype=torch.float32, device="cuda")
    if flags & MEAN:
        counts = torch.empty(k, dtype=torch.int64, device="cuda")
        _lib.check(lib.gdd_cluster_mean(n, dim, Xd.data_ptr(), perm.data_ptr(), offs.data_ptr(), k, 0,
                                        out.data_ptr(), counts.data_ptr(), _lib.stream_ptr()))
        ref, cref = O.cluster_mean(X, lab, k)
        assert np.array_equal(counts.cpu().numpy(), cref)
    else:
        wd = torch.from_numpy(w).cuda() if flags & W else None
        wsum = torch.empty(k, dtype=torch.float32, device="cuda")
        _lib.check(lib.gdd_segment_sum_f32(n, dim, Xd.data_ptr(), _lib.ptr(wd), perm.data_ptr(), offs.data_ptr(), k,
                                           out.data_ptr(), wsum.data_ptr(), _lib.stream_ptr()))
        ref, wref = np.empty((k, dim), np.float32), np.empty(k, np.float32)
        O.lib().oracle_segment_sum_f32(n, dim, X, w.ctypes.data if flags & W else None, lab, k, ref, wref)
        assert np.array_equal(wsum.cpu().numpy().view(np.uint32), wref.view(np.uint32))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), ref.view(np.uint32))


# the M-step of the phase driver: a column range (dim = f1 - f0 of rows of the full dim) and, from 4096
# members and 1.5 x the mean size, a cluster folded in 16-column slices
@pytest.mark.parametrize("n,dim,k,f0,f1,sizes,path", [
    (6040, 64, 604, 32, 64, None, "seg/f32/vec/small/2x64/sliced128"),
    (3000, 41, 40, 0, 20, None, "seg/f32/scalar/2x816/sliced1024"),
    (3000, 41, 40, 38, 41, None, "seg/f32/scalar/1x1024"),
    (3000, 64, 5, 0, 32, None, "cm/32x512/sliced1024"),
    (12000, 48, 3, 0, 48, (10, 1, 1), "cm/48x336/sliced1024"),
    (12000, 47, 3, 0, 47, (10, 1, 1), "seg/f32/scalar/3x336/sliced1024"),
    (12000, 136, 3, 0, 136, (10, 1, 1), "seg/f32/vec/9x112/sliced1024"),
])
def test_mstep_fold_forms_match_oracle(n, dim, k, f0, f1, sizes, path):
    lib = _lib.device_lib()
    X, lab, _ = _fold_case(n, dim, k, n + dim + f0, sizes)
    if sizes:
        assert np.bincount(lab).max() >= max(1.5 * n / k, 4096)  # a sliced cluster
    Xd, ld = torch.from_numpy(X).cuda(), torch.from_numpy(lab).cuda()
    unaligned = X_UNALIGNED if (Xd.data_ptr() + 4 * f0) % 16 else 0
    assert lib.gdd_fold_path(n, f1 - f0, dim, k, unaligned, -1).decode() == path
    ref, wref = np.empty((k, dim), np.float32), np.empty(k, np.float32)
    O.lib().oracle_segment_sum_f32(n, dim, X, None, lab, k, ref, wref)
    ws = _lib.workspace(lib.gdd_kmeans_lloyd_ws_bytes(n, dim, k), Xd.device)
    state = torch.zeros(lib.gdd_lloyd_state_bytes(), dtype=torch.uint8, device="cuda")
    out = torch.empty(k, f1 - f0, dtype=torch.float32, device="cuda")
    wsum = torch.empty(k, dtype=torch.float32, device="cuda")
    _lib.check(lib.gdd_lloyd_mstep(n, dim, Xd.data_ptr(), ld.data_ptr(), k, f0, f1, out.data_ptr(), wsum.data_ptr(),
                                   state.data_ptr(), 0, ws.data_ptr(), ws.numel(), _lib.stream_ptr()))
    assert np.array_equal(out.cpu().numpy().view(np.uint32), np.ascontiguousarray(ref[:, f0:f1]).view(np.uint32))
    assert np.array_equal(wsum.cpu().numpy().view(np.uint32), wref.view(np.uint32))
    assert state[:4].view(torch.int32).item() == 0  # no empty cluster: the loop goes on


@pytest.mark.parametrize("n,dim,k", [(6040, 64, 604), (20000, 47, 196), (3000, 41, 40)])
def test_mstep_column_range_equals_full_fold(n, dim, k):
    """Each rank's column slice (gdd_lloyd_mstep over [f0, f1)) is exactly those columns of the full
    ordered fold and of the oracle's segment sums."""
    lib = _lib.device_lib()
    rng = np.random.default_rng(n)
    X = rng.standard_normal((n, dim)).astype(np.float32)
    lab = rng.integers(0, k, n).astype(np.int32)
    lab[: k] = np.arange(k)  # no empty cluster
    ref = np.empty((k, dim), np.float32)
    wref = np.empty(k, np.float32)
    O.lib().oracle_segment_sum_f32(n, dim, X, None, lab, k, ref, wref)
    Xd, ld = torch.from_numpy(X).cuda(), torch.from_numpy(lab).cuda()
    ws = _lib.workspace(lib.gdd_kmeans_lloyd_ws_bytes(n, dim, k), Xd.device)
    for f0, f1 in [(0, dim), (0, (dim + 1) // 2), ((dim + 1) // 2, dim), (dim - 3, dim)]:
        state = torch.zeros(lib.gdd_lloyd_state_bytes(), dtype=torch.uint8, device="cuda")
        out = torch.empty(k * (f1 - f0), dtype=torch.float32, device="cuda")
        wsum = torch.empty(k, dtype=torch.float32, device="cuda")
        _lib.check(lib.gdd_lloyd_mstep(n, dim, Xd.data_ptr(), ld.data_ptr(), k, f0, f1, out.data_ptr(),
                                       wsum.data_ptr(), state.data_ptr(), 0, ws.data_ptr(), ws.numel(),
                                       _lib.stream_ptr()))
        got = out.cpu().numpy().reshape(k, f1 - f0)
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(ref[:, f0:f1]).view(np.uint32))
        assert np.array_equal(wsum.cpu().numpy(), wref)
