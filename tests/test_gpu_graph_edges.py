"""Every form of the propagation hop, and the row-length, block and alignment edges of the graph
kernels (gdd_propagate.hip, gdd_normalize.hip), against the oracle bit for bit and against
references that share no code with either (graph_ref) — needs a gfx950 GPU.

A hop test names its kernel form first (gdd_hop_path, the function the launchers switch on), so a
moved threshold cannot silently take a test off the form it is there for."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import graph_ref as R
from oracle import oracle as O

pytestmark = pytest.mark.gpu

import gdd  # noqa: E402
from gdd import _lib  # noqa: E402
from gdd.graph import CSRGraph, SpMMPlan  # noqa: E402

bits = R.bits
HOP_FORMS = R.HOP_FORMS


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host_bits(t):
    return bits(t.cpu().numpy())


def dev_graph(rp, col, val):
    """The CSR arrays as they are on the device (no re-canonicalisation on the way)."""
    return CSRGraph(_dev(rp.astype(np.int32)), _dev(col.astype(np.int32)),
                    _dev(val.astype(np.float32)), len(rp) - 1)


def offset_view(a, off_bytes):
    """A contiguous device copy of `a` that starts off_bytes into a larger (256-byte aligned)
    allocation."""
    t = torch.from_numpy(np.ascontiguousarray(a, np.float32))
    buf = torch.empty(t.numel() + 8, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 16 == 0 and off_bytes % 4 == 0
    v = buf[off_bytes // 4: off_bytes // 4 + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == off_bytes % 16
    return v


def common_align(*tensors):
    ptrs = [t.data_ptr() for t in tensors]
    return 16 if all(p % 16 == 0 for p in ptrs) else 8 if all(p % 8 == 0 for p in ptrs) else 4


def hop_path(d, align):
    return _lib.load().gdd_hop_path(d, align).decode()


def w32(alpha):
    """The target's weight as the library forms it: alpha arrives as fp32, 1 - alpha is taken in
    fp64 and rounded to fp32 (the reference's Python double meeting an fp32 tensor)."""
    return np.float32(1.0 - np.float64(np.float32(alpha)))


def feats(n, d, seed):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


# ---- shared graphs and references (computed once, never modified) ---------------------------------
@functools.lru_cache(maxsize=None)
def signed_ladder():
    A = R.ladder_graph(weighted=True, signed=True)
    return A, R.csr_arrays(A), dev_graph(*R.csr_arrays(A))


@functools.lru_cache(maxsize=None)
def normalized_ladder():
    """The unsigned ladder graph normalised by the oracle (the hop tests do not depend on the
    normalisation kernels)."""
    rp, col, _ = R.csr_arrays(R.ladder_graph())
    ro, co, vo = O.normalize_csr(rp, col, None, -1)
    return (ro, co, vo), dev_graph(ro, co, vo)


def check_propagate(g_host, g_dev, X, T, alpha, Xd=None, **kw):
    t_ref, p_ref = O.propagate(*g_host, X, T, alpha)
    t, p = gdd.propagate(g_dev, _dev(X) if Xd is None else Xd, T, alpha, **kw)
    assert np.array_equal(_host_bits(t), bits(t_ref))
    assert np.array_equal(_host_bits(p), bits(p_ref))


# ---- one test per hop form ------------------------------------------------------------------------
ALIGNED_FORMS = [(d, a, f) for d, a, f in HOP_FORMS if a == 16]


def test_every_reachable_form_is_named():
    """Every k_hop<V, G, S> that run_hop can launch appears in the per-form or the misaligned test."""
    forms = {f for _, _, f in HOP_FORMS} | {f for _, _, f in MISALIGNED}
    for V in (4, 2, 1):
        for S in (8, 4, 2, 1, 0):
            assert f"v{V}/g64/s{S}" in forms
        assert f"v{V}/g16/s1" in forms and f"v{V}/g32/s1" in forms
    assert "v4/g16/s2" in forms


@pytest.mark.parametrize("d,align,form", ALIGNED_FORMS, ids=[f"{d}-{f}" for d, _, f in ALIGNED_FORMS])
def test_hop_form_bitexact(d, align, form):
    assert hop_path(d, align) == form
    A, (rp, col, val), g = signed_ladder()
    n = A.shape[0]
    x = feats(n, d, d)
    xd = _dev(x)
    assert common_align(xd) == align
    # a single hop: the oracle's bits, and within the derived bound of the fp64 product
    y_ref = O.spmm(rp, col, val, x, scale=0.7)
    y = gdd.spmm(g, xd, 0.7).cpu().numpy()
    y64, bound = R.spmm_ref64(A, x, 0.7)
    err = np.abs(y.astype(np.float64) - y64)
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    assert np.array_equal(bits(y), bits(y_ref))
    # a planned hop with an accumulator, twice on one plan
    acc0 = feats(n, d, d + 1)
    y_ref = O.spmm(rp, col, val, x, scale=0.91)
    acc_ref = (acc0 + np.float32(0.09) * y_ref).astype(np.float32)
    plan = SpMMPlan(g, d)
    for _ in range(2):
        yd = torch.empty_like(xd)
        acc = _dev(acc0)
        assert common_align(xd, yd, acc) == align
        plan.hop(xd, yd, 0.91, acc, 0.09)
        assert np.array_equal(_host_bits(yd), bits(y_ref))
        assert np.array_equal(_host_bits(acc), bits(acc_ref))
    # the propagation loop: first hop with the initial target, paired and unpaired tails
    gn_host, gn = normalized_ladder()
    for T in (4, 5):
        check_propagate(gn_host, gn, x, T, 0.8)


# ---- buffers that are not 16-byte aligned ---------------------------------------------------------
MISALIGNED = [(128, 8, "v2/g64/s1"), (128, 4, "v1/g64/s2"), (64, 8, "v2/g32/s1"), (64, 4, "v1/g64/s1")]


@pytest.mark.parametrize("which", ["x", "y", "acc"])
@pytest.mark.parametrize("d,align,form", MISALIGNED, ids=[f"{d}-a{a}" for d, a, _ in MISALIGNED])
def test_misaligned_buffers(d, align, form, which):
    off = align  # 8 or 4 bytes into a 16-byte aligned allocation
    assert hop_path(d, align) == form
    A, (rp, col, val), g = signed_ladder()
    n = A.shape[0]
    x, acc0 = feats(n, d, 3), feats(n, d, 4)
    y_ref = O.spmm(rp, col, val, x, scale=0.91)
    acc_ref = (acc0 + np.float32(0.09) * y_ref).astype(np.float32)
    plan = SpMMPlan(g, d)
    # the aligned run
    xa, ya, acca = _dev(x), torch.empty(n, d, device="cuda"), _dev(acc0)
    assert common_align(xa, ya, acca) == 16
    plan.hop(xa, ya, 0.91, acca, 0.09)
    # one buffer moved off alignment
    xm = offset_view(x, off) if which == "x" else _dev(x)
    ym = offset_view(np.zeros((n, d), np.float32), off) if which == "y" else torch.empty(n, d, device="cuda")
    accm = offset_view(acc0, off) if which == "acc" else _dev(acc0)
    assert common_align(xm, ym, accm) == align
    plan.hop(xm, ym, 0.91, accm, 0.09)
    assert torch.equal(ym.view(torch.int32), ya.view(torch.int32))
    assert torch.equal(accm.view(torch.int32), acca.view(torch.int32))
    assert np.array_equal(_host_bits(ym), bits(y_ref))
    assert np.array_equal(_host_bits(accm), bits(acc_ref))


@pytest.mark.parametrize("d", [128, 64])
def test_propagate_misaligned_features(d):
    """X 4 bytes off: the first hop (x and the initial target both read X) runs the scalar form, the
    later hops the aligned one."""
    assert hop_path(d, 4).startswith("v1/") and hop_path(d, 16).startswith("v4/")
    gn_host, gn = normalized_ladder()
    X = feats(gn.n, d, 11)
    Xd = offset_view(X, 4)
    assert common_align(Xd) == 4
    for T in (2, 4, 5):
        check_propagate(gn_host, gn, X, T, 0.8, Xd=Xd)


# ---- relabelled propagation on the sliced and float2 forms ----------------------------------------
@pytest.mark.parametrize("d,form", [(1024, "v4/g64/s4"), (450, "v2/g64/s4"), (62, "v2/g32/s1")])
def test_propagate_relabeled_forms(d, form):
    assert hop_path(d, 16) == form
    gn_host, gn = normalized_ladder()
    check_propagate(gn_host, gn, feats(gn.n, d, 5), 5, 0.8, relabel="degree")


# ---- the fix-up pass ------------------------------------------------------------------------------
def _rows_graph(n, lengths, seed):
    rng = np.random.default_rng(seed)
    cols = np.concatenate([np.sort(rng.choice(n, size=L, replace=False)) for L in lengths])
    nnz = int(np.sum(lengths))
    vals = (rng.uniform(0.1, 3.0, nnz) * rng.choice([-1.0, 1.0], nnz)).astype(np.float32)
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(lengths, out=rowptr[1:])
    return rowptr, cols.astype(np.int32), vals


def _check_hop_with_acc(rp, col, val, d, seed):
    n = len(rp) - 1
    g = dev_graph(rp, col, val)
    x, acc0 = feats(n, d, seed), feats(n, d, seed + 1)
    y_ref = O.spmm(rp, col, val, x, scale=0.91)
    acc_ref = (acc0 + np.float32(0.09) * y_ref).astype(np.float32)
    xd = _dev(x)
    assert np.array_equal(_host_bits(gdd.spmm(g, xd, 0.91)), bits(y_ref))
    yd, acc = torch.empty_like(xd), _dev(acc0)
    SpMMPlan(g, d).hop(xd, yd, 0.91, acc, 0.09)
    assert np.array_equal(_host_bits(yd), bits(y_ref))
    assert np.array_equal(_host_bits(acc), bits(acc_ref))


@pytest.mark.parametrize("d", [8, 7])
def test_fixup_grid_stride(d):
    """1100 split rows (257 entries each): more than k_fixup's 1024 blocks, so its loop iterates."""
    n = 1100
    rp, col, val = _rows_graph(n, [257] * n, 6)
    assert n > 1024 and min(n * 257 // 256 + 1, 1024) == 1024
    _check_hop_with_acc(rp, col, val, d, 7)


def test_fixup_partial_counts():
    """Rows of 256 s + 1 entries, s = 1..17: 2..18 partials, every remainder of the fold's
    eight-at-a-time loop, zero to two rounds of it."""
    n = 4400
    lengths = np.random.default_rng(8).integers(0, 4, n)
    for s in range(1, 18):
        lengths[100 + 250 * (s - 1)] = 256 * s + 1
    rp, col, val = _rows_graph(n, lengths, 9)
    assert sorted({-(-int(L) // 256) for L in lengths if L > 256}) == list(range(2, 19))
    _check_hop_with_acc(rp, col, val, 4, 10)


# ---- T = 1 ----------------------------------------------------------------------------------------
def test_propagate_t1_stride_loop():
    """n * d above k_scale_copy's 8192 * 256 threads: its stride loop takes a second round."""
    n, d = 2100, 1024
    assert n * d > 8192 * 256
    rp, col, val = _rows_graph(n, np.ones(n, np.int64), 12)
    X = feats(n, d, 13)
    t, p = gdd.propagate(dev_graph(rp, col, val), _dev(X), 1, 0.8)
    assert np.array_equal(_host_bits(t), bits(w32(0.8) * X))
    assert np.array_equal(_host_bits(p), bits(X))
    t_ref, p_ref = O.propagate(rp, col, val, X, 1, 0.8)
    assert np.array_equal(_host_bits(t), bits(t_ref)) and np.array_equal(_host_bits(p), bits(p_ref))


# ---- degenerate graphs ----------------------------------------------------------------------------
def _identity_closed_form(X, T, alpha):
    """Â = I: every hop is one rounded product fp32(alpha) * p (the fma chain of a single entry of
    value fp32(alpha) * 1 from +0), the target accumulates fp32(1 - alpha) * p hop by hop."""
    a, w = np.float32(alpha), w32(alpha)
    p = X.copy()
    t = w * X
    for _ in range(T - 1):
        p = a * p
        t = t + w * p
    return t, p


@pytest.mark.parametrize("stored", [False, True])
@pytest.mark.parametrize("self_loops", [-1, 0, 1])
def test_single_node(stored, self_loops):
    A = sp.csr_matrix(np.array([[1.0 if stored else 0.0]], np.float32))
    A.eliminate_zeros()
    g = gdd.normalize_adj(gdd.to_csr(A), self_loops=self_loops)
    ro, co, vo = O.normalize_csr(*R.csr_arrays(A)[:2], None, self_loops)
    assert np.array_equal(g.rowptr.cpu().numpy(), ro) and np.array_equal(g.col.cpu().numpy(), co)
    assert np.array_equal(_host_bits(g.val), bits(vo))
    # [[1]] whenever anything is stored or added (1/1, or 2/(sqrt 2 sqrt 2)); empty otherwise
    empty = not stored and self_loops == 0
    assert g.val.cpu().tolist() == ([] if empty else [1.0])
    X = feats(1, 5, 14)
    for T in (1, 2, 4):
        t, p = gdd.propagate(g, _dev(X), T, 0.8)
        if empty and T > 1:
            t_exp, p_exp = w32(0.8) * X, np.zeros_like(X)
        else:
            t_exp, p_exp = _identity_closed_form(X, T, 0.8)
        assert np.array_equal(_host_bits(t), bits(t_exp))
        assert np.array_equal(_host_bits(p), bits(p_exp))
    y = gdd.spmm(g, _dev(X), 0.7)
    assert np.array_equal(_host_bits(y), bits(np.zeros_like(X) if empty else np.float32(0.7) * X))


@pytest.mark.parametrize("d", [40, 7])
def test_empty_graph(d):
    n = 768
    A = sp.csr_matrix((n, n), dtype=np.float32)
    g0 = gdd.to_csr(A)
    assert g0.nnz == 0
    X = feats(n, d, 15)
    Xd = _dev(X)
    # with self-loops Â = I
    for self_loops in (-1, 1):
        gi = gdd.normalize_adj(g0, self_loops=self_loops)
        assert np.array_equal(gi.rowptr.cpu().numpy(), np.arange(n + 1))
        assert np.array_equal(gi.col.cpu().numpy(), np.arange(n))
        assert np.array_equal(_host_bits(gi.val), bits(np.ones(n, np.float32)))
    for T in (1, 2, 4, 5):
        t, p = gdd.propagate(gi, Xd, T, 0.8)
        t_exp, p_exp = _identity_closed_form(X, T, 0.8)
        assert np.array_equal(_host_bits(t), bits(t_exp))
        assert np.array_equal(_host_bits(p), bits(p_exp))
    # without them Â is empty: every hop is exact +0, the target keeps its first term
    ge = gdd.normalize_adj(g0, self_loops=0)
    assert ge.nnz == 0 and not ge.rowptr.cpu().numpy().any()
    for T in (2, 4):
        t, p = gdd.propagate(ge, Xd, T, 0.8)
        assert np.array_equal(_host_bits(t), bits(w32(0.8) * X))
        assert not _host_bits(p).any()
    assert not _host_bits(gdd.spmm(ge, Xd, 0.7)).any()
    yd, acc = torch.empty_like(Xd), Xd.clone()
    SpMMPlan(ge, d).hop(Xd, yd, 0.91, acc, 0.09)
    assert not _host_bits(yd).any() and np.array_equal(_host_bits(acc), bits(X))


# ---- normalisation --------------------------------------------------------------------------------
NORM_GRAPHS = {
    "ladder_binary": lambda: R.ladder_graph(),
    "ladder_weighted": lambda: R.ladder_graph(weighted=True),
    "diag_cases": lambda: R.diag_cases_graph(),
    "sparse_runs_exact": lambda: R.sparse_runs_graph(True),
    "sparse_runs_inexact": lambda: R.sparse_runs_graph(False),
}


@pytest.mark.parametrize("self_loops", [-1, 0, 1])
@pytest.mark.parametrize("name", sorted(NORM_GRAPHS))
def test_normalize_edges(name, self_loops):
    A = NORM_GRAPHS[name]()
    rp, col, val = R.csr_arrays(A)
    binary = bool((val == 1).all())
    assert binary == (name in ("ladder_binary", "sparse_runs_exact", "sparse_runs_inexact"))
    if name.startswith("sparse_runs"):
        # the layouts this graph is for, as k_fast_fill's blocks see them
        first, last, span = R.fill_block_ranges(rp)
        assert span.max() > 512  # a block whose row range is searched in global memory
        assert np.any((first == R.SPARSE_HUB_ROW) & (last == R.SPARSE_HUB_ROW))  # a block inside the hub
    g = gdd.normalize_adj(gdd.to_csr(A, binary=binary), self_loops=self_loops)
    got = (g.rowptr.cpu().numpy(), g.col.cpu().numpy(), g.val.cpu().numpy())
    for ref in (O.normalize_csr(rp, col, None if binary else val, self_loops),
                R.normalize_ref(A, R.adds_identity(A, self_loops))):
        assert np.array_equal(got[0], ref[0])
        assert np.array_equal(got[1], ref[1])
        assert np.array_equal(bits(got[2]), bits(ref[2]))
