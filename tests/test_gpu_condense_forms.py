"""HIP condensation kernels (csrc/gdd_condense.hip) at the forms test_gpu_condense.py never selects,
bit for bit against oracle/condense.py — needs a gfx950 GPU.

* class counts that are multiples of four (the float4 branches of k_edge_cos and k_class_keys, the
  32-wide block of the former and its float4 tail) next to their neighbours;
* rows of 511..12291 entries (k_row_sums_long's chunk loop and buffer flip);
* top-k ties that straddle 4096-edge blocks, under one set and several, and more than 256 blocks
  (two blocks per lane in k_tk_scan); negatives, infinities, denormals and both zeros at the cut;
* graphs without values (every kernel's `val == nullptr` branch), the `sel` argument of
  gdd_graph_compress, empty selections, softmax edges and the label checks.

That the inputs have these properties is asserted on the host, from the oracle alone, in
test_condense_cases_host.py. Values are compared as bits; where the oracle gives NaN (an ER of 0/0)
the device must give NaN at the same place, the payload being nobody's definition."""
import functools

import numpy as np
import pytest
import torch

import condense_cases as CC
from oracle import condense as O

pytestmark = pytest.mark.gpu

from gdd import _lib  # noqa: E402
from gdd import condense as GC  # noqa: E402
from gdd.graph import CSRGraph  # noqa: E402


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _assert_same(dev, ref, what=""):
    a = np.ascontiguousarray(_np(dev), dtype=np.float32)
    b = np.ascontiguousarray(_np(ref), dtype=np.float32)
    assert a.shape == b.shape, what
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), what
    assert np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]), what


def _graph(rowptr, col, val, n):
    return CSRGraph(torch.tensor(rowptr, dtype=torch.int32).cuda(), torch.tensor(col, dtype=torch.int32).cuda(),
                    None if val is None else torch.tensor(val, dtype=torch.float32).cuda(), int(n))


def _ones_if_none(val, nnz):
    return np.ones(nnz, np.float32) if val is None else val


def _case_graph(name, binary):
    rowptr, col, val, n = CC.small_graph() if name == "small" else CC.long_row_graph()
    return rowptr, col, (None if binary else val), n


# ---- cosine forms ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _attaw_ref(name, binary, C):
    rowptr, col, val, n = _case_graph(name, binary)
    return O.attaw_er(rowptr, col, _ones_if_none(val, len(col)), CC.embeddings(n, C))


def _check_attaw(name, binary, C):
    rowptr, col, val, n = _case_graph(name, binary)
    ebd = CC.embeddings(n, C)
    er_ref, rew_ref = _attaw_ref(name, binary, C)
    er, g = GC.attaw_ER_estimator(_graph(rowptr, col, val, n), torch.tensor(ebd).cuda())
    _assert_same(g.val, rew_ref, "reweighted values")
    _assert_same(er, er_ref, "er")
    return ebd


@pytest.mark.parametrize("C", [1, 3, 4, 8, 28, 32, 33, 36, 40, 64, 68])
def test_cosine_forms(C):
    ebd = _check_attaw("small", False, C)
    assert np.isnan(_attaw_ref("small", False, C)[0]).any()  # the zero rows' 0/0
    _assert_same(GC.softmax_rows(torch.tensor(ebd).cuda()), O.softmax_rows(ebd), "softmax")


@pytest.mark.parametrize("C", [4, 33, 40])
def test_cosine_forms_binary(C):
    _check_attaw("small", True, C)


# ---- class-key forms ---------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [4, 8, 40])
def test_class_key_forms(C):
    rowptr, col, val, n = CC.small_graph()
    ebd = CC.embeddings(n, C)
    sels, vals = O.graph_sparse(rowptr, col, val, 0.3, ebd, "attaw")
    out = GC.graph_sparse(_graph(rowptr, col, val, n), 0.3, torch.tensor(ebd).cuda(), "attaw")
    assert len(out) == len(sels) == C
    rows = O.coo_rows(rowptr)
    for i, (g, s) in enumerate(zip(out, sels)):
        assert np.array_equal(O.coo_rows(_np(g.rowptr)), rows[s]), i
        assert np.array_equal(_np(g.col), col[s]), i
        _assert_same(g.val, vals[s], f"class {i}")


# ---- long rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("binary", [False, True], ids=["valued", "binary"])
def test_long_rows_vanilla(binary):
    rowptr, col, val, n = _case_graph("long", binary)
    ref = O.vanilla_er(rowptr, col, _ones_if_none(val, len(col)))
    assert not np.isnan(ref).any()
    _assert_same(GC.ER_estimator(_graph(rowptr, col, val, n)), ref)


@pytest.mark.parametrize("C", [4, 7])
def test_long_rows_attaw(C):
    _check_attaw("long", False, C)


def test_long_row_degrees_one_at_a_time():
    """col = the row's own index: er = 2 v / deg[row], so an entry depends on one degree only and a
    failure names the row. (test_long_rows_vanilla pins every long degree already, through the 511+
    quotients v / deg[row] of its own entries; this case is kept for the plain reading.)"""
    rowptr, col, val, n = CC.long_row_graph()
    rows = O.coo_rows(rowptr)
    ref = O.vanilla_er(rowptr, rows, val)
    lib = _lib.device_lib()
    g = _graph(rowptr, rows, val, n)
    er = torch.empty(g.nnz, dtype=torch.float32, device="cuda")
    ws = _lib.workspace(lib.gdd_er_ws_bytes(n, 1), g.device)
    _lib.check(lib.gdd_vanilla_er(n, g.nnz, g.rowptr.data_ptr(), g.col.data_ptr(), g.col.data_ptr(),
                                  g.val.data_ptr(), er.data_ptr(), ws.data_ptr(), ws.numel(),
                                  _lib.stream_ptr(g.device)))
    got = _np(er)
    bad = sorted(set(rows[got.view(np.uint32) != ref.view(np.uint32)].tolist()))
    assert not bad, f"rows with a wrong degree: {bad[:10]} (lengths {np.diff(rowptr)[bad[:10]]})"


# ---- top-k across blocks, one set --------------------------------------------------------------------
def _edge_list(nnz):
    """A graph object for topk_edges when probs is None: rows and col are passed and never read."""
    z = torch.zeros(nnz, dtype=torch.int32, device="cuda")
    g = CSRGraph(torch.tensor([0, nnz], dtype=torch.int32).cuda(), z, None, 1)
    g._rows = z
    return g


def _check_topk(w, ms):
    g = _edge_list(len(w))
    wd = torch.tensor(w).cuda()
    for m in ms:
        sel = _np(GC.topk_edges(g, wd, m))
        assert sel.shape == (1, m)
        assert np.array_equal(sel[0], O.topk_edges(w, m)), m


@pytest.mark.parametrize("kind", ["ints", "equal", "mixed"])
def test_topk_ties_across_blocks(kind):
    _check_topk(CC.tie_weights(CC.TOPK_NNZ, kind), CC.topk_ms(CC.TOPK_NNZ))


def test_topk_two_blocks_per_scan_lane():
    _check_topk(CC.tie_weights(CC.TOPK_NNZ_BIG, "ints1000"), CC.topk_ms_big(CC.TOPK_NNZ_BIG))


# ---- top-k with several sets -------------------------------------------------------------------------
def _check_class_topk(n, nsets, ms):
    rowptr, rows, col = CC.complete_graph(n)
    probs, er = CC.complete_weights(n, nsets)
    g = _graph(rowptr, col, None, n)
    pd, ed = torch.tensor(probs).cuda(), torch.tensor(er).cuda()
    ws = [O.class_weights(probs, er, rows, col, i) for i in range(nsets)]
    for m in ms:
        sel = _np(GC.topk_edges(g, ed, m, pd))
        assert sel.shape == (nsets, m)
        for i in range(nsets):
            assert np.array_equal(sel[i], O.topk_edges(ws[i], m)), (m, i)


@pytest.mark.parametrize("nsets", [3, 4])
def test_class_topk_ties(nsets):
    _check_class_topk(130, nsets, (1, 5000, 16899))


def test_class_topk_two_sets_two_blocks_per_scan_lane():
    _check_class_topk(1040, 2, (1040 * 1040 // 3,))


# ---- compress, select --------------------------------------------------------------------------------
def _labels(n, k, seed=5):
    lab = np.random.default_rng(seed).integers(0, k, n).astype(np.int32)
    lab[:k] = np.arange(k)
    return lab


def test_compress_binary():
    rowptr, col, _, n = CC.small_graph()
    lab = _labels(n, 7)
    ref = O.compress(lab, O.coo_rows(rowptr), col, np.ones(len(col), np.float32))
    _assert_same(GC.compress_dense(torch.tensor(lab).cuda(), _graph(rowptr, col, None, n), 7), ref)


@pytest.mark.parametrize("e", [60, -60])
def test_compress_scales_exactly(e):
    rowptr, col, val, n = CC.small_graph()
    lab = _labels(n, 7)
    labd = torch.tensor(lab).cuda()
    rows = O.coo_rows(rowptr)
    base = _np(GC.compress_dense(labd, _graph(rowptr, col, val, n), 7))
    _assert_same(base, O.compress(lab, rows, col, val))
    scaled = np.ldexp(val, e).astype(np.float32)
    assert np.array_equal(np.ldexp(scaled.astype(np.float64), -e), val.astype(np.float64))  # exact
    got = GC.compress_dense(labd, _graph(rowptr, col, scaled, n), 7)
    _assert_same(got, O.compress(lab, rows, col, scaled))
    want = np.ldexp(base.astype(np.float64), e).astype(np.float32)
    assert np.all(np.isfinite(want)) and np.all((want != 0) == (base != 0))
    _assert_same(got, want)


def test_compress_one_cluster():
    rowptr, col, val, n = CC.small_graph()
    lab = np.zeros(n, np.int32)
    got = GC.compress_dense(torch.tensor(lab).cuda(), _graph(rowptr, col, val, n), 1)
    _assert_same(got, O.compress(lab, O.coo_rows(rowptr), col, val, k=1))
    assert _np(got).tolist() == [[0.0]]


@pytest.mark.parametrize("binary", [False, True], ids=["valued", "binary"])
def test_compress_sel_argument(binary):
    """gdd_graph_compress over the edge ids in `sel` = compress of the selected sub-graph."""
    rowptr, col, val, n = _case_graph("small", binary)
    nnz, kk = len(col), 9
    lab = _labels(n, kk)
    s = np.sort(np.random.default_rng(8).choice(nnz, nnz // 3, replace=False)).astype(np.int32)
    g = _graph(rowptr, col, val, n)
    labd, seld = torch.tensor(lab).cuda(), torch.tensor(s).cuda()
    lib = _lib.device_lib()
    out = torch.empty((kk, kk), dtype=torch.float32, device="cuda")
    ws = _lib.workspace(lib.gdd_compress_ws_bytes(kk), g.device)
    _lib.check(lib.gdd_graph_compress(n, labd.data_ptr(), kk, len(s), _lib.ptr(GC.coo_rows(g)),
                                      _lib.ptr(g.col), _lib.ptr(g.val), seld.data_ptr(), out.data_ptr(),
                                      ws.data_ptr(), ws.numel(), _lib.stream_ptr(g.device)))
    sub = GC.select_graph(g, seld, g.val)  # binary: no values, the selection carries ones
    assert sub.nnz == len(s)
    _assert_same(out, GC.compress_dense(labd, sub, kk))
    rows = O.coo_rows(rowptr)
    _assert_same(out, O.compress(lab, rows[s], col[s], _ones_if_none(val, nnz)[s], k=kk))


def test_select_graph_of_nothing():
    rowptr, col, val, n = CC.small_graph()
    g = _graph(rowptr, col, val, n)
    sub = GC.select_graph(g, torch.empty(0, dtype=torch.int32, device="cuda"), g.val)
    assert sub.n == n and sub.nnz == 0
    assert np.array_equal(_np(sub.rowptr), np.zeros(n + 1, np.int32))


# ---- softmax -----------------------------------------------------------------------------------------
def test_softmax_one_class():
    x = np.random.default_rng(2).standard_normal((300, 1)).astype(np.float32) * 50
    p = GC.softmax_rows(torch.tensor(x).cuda())
    _assert_same(p, O.softmax_rows(x))
    assert np.all(_np(p) == 1.0)


def test_softmax_underflow_and_minus_inf():
    x = np.random.default_rng(3).standard_normal((257, 6)).astype(np.float32)
    x[0] = [80, -80, 0, 79.5, -79.5, 80]     # exp(-160) is 0 in fp32, and the maximum twice
    x[1] = [-80, -80, -80, -80, -80, 80]
    x[2] = [0, -np.inf, 1, 2, 3, 4]          # one -inf: a zero, not a NaN
    x[3] = [-np.inf, 5, 5, 5, 5, 5]
    x[256] = [-103.9, 0, -104.0, -87.3, -87.4, 0]  # either side of fp32's smallest denormal and normal
    ref = O.softmax_rows(x)
    assert not np.isnan(ref).any() and ref[0, 1] == 0 and ref[2, 1] == 0
    _assert_same(GC.softmax_rows(torch.tensor(x).cuda()), ref)


# ---- labels ------------------------------------------------------------------------------------------
def test_labels_outside_the_clusters_are_refused():
    """Refused on the host, before any launch (F.one_hot in the reference rejects negatives too)."""
    rowptr, col, val, n = CC.small_graph()
    g = _graph(rowptr, col, val, n)
    lab = _labels(n, 7)
    lab[11] = -1  # sklearn-style "unassigned"
    with pytest.raises(ValueError):
        GC.graph_compress(torch.tensor(lab), g, [g])
    with pytest.raises(ValueError):
        GC.graph_compress(lab, g, [])
    with pytest.raises(ValueError):
        GC.compress_dense(torch.tensor(lab).cuda(), g, 7)
    lab[11] = 7
    with pytest.raises(ValueError):
        GC.compress_dense(torch.tensor(lab).cuda(), g, 7)
    with pytest.raises(ValueError):
        GC.compress_dense(torch.tensor(lab[:-1]).cuda(), g, 8)
