"""The community node order on the device (gdd_community_order: gdd.graph.locality_order(adj,
"community"), gdd.graph.community_labels, gdd.propagate(relabel="community")) against the host model
of tests/community_util.py. Integer work: rho, labels and the per-sweep changed counts are equal
exactly. The relabelled propagation is bitwise the plain one."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import community_util as cu

pytestmark = pytest.mark.gpu

import gdd  # noqa: E402
from gdd import _lib  # noqa: E402
from gdd.graph import _community_order  # noqa: E402


def _graph(rowptr, col):
    n = rowptr.shape[0] - 1
    return gdd.CSRGraph(torch.from_numpy(np.asarray(rowptr, np.int32)).cuda(),
                        torch.from_numpy(np.asarray(col, np.int32)).cuda(), None, n)


def _check(rowptr, col, sweeps, ref=None):
    rho_m, lab_m, chg_m = ref if ref is not None else cu.community_order(rowptr, col, sweeps)
    g = _graph(rowptr, col)
    rho, lab, chg = _community_order(g, sweeps)
    assert rho.dtype == torch.int32 and rho.device.type == "cuda"
    assert np.array_equal(chg.cpu().numpy(), chg_m), (chg.cpu().numpy(), chg_m)
    assert np.array_equal(lab.cpu().numpy(), lab_m)
    assert np.array_equal(rho.cpu().numpy(), rho_m)
    # the public entry points are the same call
    assert torch.equal(gdd.graph.locality_order(g, "community", sweeps=sweeps), rho)
    lab2, chg2 = gdd.graph.community_labels(g, sweeps=sweeps)
    assert torch.equal(lab2, lab) and torch.equal(chg2, chg)
    return chg_m


@pytest.mark.parametrize("diag", [False, True])
@pytest.mark.parametrize("sweeps", [0, 1, 8, 16])
def test_sbm_matches_model(sweeps, diag):
    rowptr, col = cu.sbm(0, diag=diag)
    chg = _check(rowptr, col, sweeps, cu.model("sbm", 0, sweeps, diag=diag))
    if sweeps == 16:  # the early exit ran: the last sweeps follow a zero-change sweep
        assert chg[-1] == 0 and chg[-2] == 0 and chg[0] > 0


def test_normalized_graph_matches_model():
    """The shape propagate sees: a raw binary graph through gdd.normalize_adj (stored diagonal, values)."""
    rowptr, col = cu.sbm(1)
    A = sp.csr_matrix((np.ones(col.shape[0], np.float32), col, rowptr), shape=(8192, 8192))
    g = gdd.normalize_adj(gdd.to_csr(A))
    rp, c = g.rowptr.cpu().numpy().astype(np.int64), g.col.cpu().numpy().astype(np.int64)
    assert g.nnz == col.shape[0] + 8192
    rho_m, lab_m, chg_m = cu.community_order(rp, c, 8)
    rho = gdd.graph.locality_order(g, "community", sweeps=8)
    lab, chg = gdd.graph.community_labels(g, sweeps=8)
    assert np.array_equal(rho.cpu().numpy(), rho_m)
    assert np.array_equal(lab.cpu().numpy(), lab_m)
    assert np.array_equal(chg.cpu().numpy(), chg_m)


def test_hub_graph_matches_model():
    """Rows above CAP: only their first 256 entries vote, and entries that point at them cast none."""
    rowptr, col = cu.sbm(0, hubs=3)
    assert (np.diff(rowptr) > cu.CAP).sum() == 3
    _check(rowptr, col, 8, cu.model("sbm", 0, 8, hubs=3))


# every row length at which the sweep kernel takes another path (16 and 32 lanes per row, the whole
# wave, the 128- and 256-slot sorts, the cap), one below and one above each
LENS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600]


@pytest.mark.parametrize("n", [701, 702, 704])  # ragged last quad of rows, ragged last block of waves
def test_row_length_thresholds(n):
    rowptr, col = cu.rows_graph(LENS, n)
    assert np.diff(rowptr)[:len(LENS)].tolist() == LENS
    chg = _check(rowptr, col, 6)
    assert chg[0] > 0 and chg[2] > 0
    # the same long rows where every quad holds one: rows 0, 4, 8, ... (the others short)
    lens = np.zeros(4 * len(LENS), np.int64)
    lens[::4] = LENS
    lens[1::4] = 3
    rowptr, col = cu.rows_graph(lens.tolist(), n)
    _check(rowptr, col, 4)


@pytest.mark.parametrize("name", ["empty", "one", "path", "ring", "grid"])
def test_small_and_tie_heavy_graphs(name):
    rowptr, col = {"empty": lambda: (np.zeros(301, np.int64), np.zeros(0, np.int64)),
                   "one": lambda: (np.zeros(2, np.int64), np.zeros(0, np.int64)),
                   "path": lambda: cu.path(5), "ring": lambda: cu.ring(1000),
                   "grid": lambda: cu.grid(32, 32)}[name]()
    chg = _check(rowptr, col, 5)
    if name in ("empty", "one"):
        g = _graph(rowptr, col)
        assert gdd.graph.locality_order(g, "community").cpu().tolist() == list(range(g.n))
        assert chg.tolist() == [0] * 5
    else:
        assert chg[0] > 0


def test_poisoned_buffers_give_equal_results():
    """Nothing is read before it is written: two calls into differently poisoned outputs and a
    workspace of exactly gdd_community_order_ws_bytes are bit-equal (and equal the model)."""
    rowptr, col = cu.sbm(0, hubs=3)
    g = _graph(rowptr, col)
    lib = _lib.device_lib()
    nbytes = lib.gdd_community_order_ws_bytes(g.n, g.nnz)
    assert nbytes % 4 == 0
    outs = []
    for fill in (0x7FC00000, -1):  # a NaN pattern, all ones
        ws = torch.full((nbytes // 4,), fill, dtype=torch.int32, device="cuda")
        rho, lab = (torch.full((g.n,), fill, dtype=torch.int32, device="cuda") for _ in range(2))
        chg = torch.full((8,), fill, dtype=torch.int32, device="cuda")
        _lib.check(lib.gdd_community_order(g.n, g.nnz, g.rowptr.data_ptr(), g.col.data_ptr(), 8,
                                           rho.data_ptr(), lab.data_ptr(), chg.data_ptr(), ws.data_ptr(),
                                           nbytes, _lib.stream_ptr(g.device)))
        outs.append((rho.cpu().numpy(), lab.cpu().numpy(), chg.cpu().numpy()))
    for a, b, m in zip(outs[0], outs[1], cu.model("sbm", 0, 8, hubs=3)):
        assert np.array_equal(a, b) and np.array_equal(a, m)
    # rho alone (labels and changed are optional)
    rho = torch.empty(g.n, dtype=torch.int32, device="cuda")
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    _lib.check(lib.gdd_community_order(g.n, g.nnz, g.rowptr.data_ptr(), g.col.data_ptr(), 8,
                                       rho.data_ptr(), None, None, ws.data_ptr(), nbytes,
                                       _lib.stream_ptr(g.device)))
    assert np.array_equal(rho.cpu().numpy(), outs[0][0])


@pytest.mark.parametrize("T", [2, 5])
@pytest.mark.parametrize("d", [40, 100, 128])
def test_propagate_community_bitexact(d, T):
    n = 4096
    rowptr, col = cu.sbm(2, n=n)
    A = sp.csr_matrix((np.ones(col.shape[0], np.float32), col, rowptr), shape=(n, n))
    g = gdd.normalize_adj(gdd.to_csr(A))
    X = torch.from_numpy(np.random.default_rng(d + T).standard_normal((n, d)).astype(np.float32)).cuda()
    t0, p0 = gdd.propagate(g, X, T, 0.8)
    t1, p1 = gdd.propagate(g, X, T, 0.8, relabel="community")
    assert torch.equal(t0.view(torch.int32), t1.view(torch.int32))
    assert torch.equal(p0.view(torch.int32), p1.view(torch.int32))
    rho = gdd.graph.locality_order(g, "community")
    assert not torch.equal(rho, torch.arange(n, dtype=torch.int32, device="cuda"))  # a real reorder


def test_rejects_bad_input():
    rowptr, col = cu.ring(100)
    g = _graph(rowptr, col)
    with pytest.raises(ValueError):
        gdd.graph.locality_order(g, "community", sweeps=-1)
    with pytest.raises(ValueError):
        gdd.graph.community_labels(g, sweeps=-1)
    lib = _lib.device_lib()
    rho = torch.empty(100, dtype=torch.int32, device="cuda")
    nbytes = lib.gdd_community_order_ws_bytes(100, 200)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    args = (g.rowptr.data_ptr(), g.col.data_ptr())
    st = _lib.stream_ptr(g.device)
    assert lib.gdd_community_order(-1, 200, *args, 3, rho.data_ptr(), None, None, ws.data_ptr(), nbytes, st) != 0
    assert b"community_order" in lib.gdd_last_error()
    assert lib.gdd_community_order(100, 200, *args, -1, rho.data_ptr(), None, None, ws.data_ptr(), nbytes, st) != 0
    assert b"sweeps" in lib.gdd_last_error()
    assert lib.gdd_community_order(100, 200, *args, 3, rho.data_ptr(), None, None, ws.data_ptr(), 64, st) == 0x10002
    assert b"workspace" in lib.gdd_last_error()
    # an out-of-range column is not dereferenced: it casts no vote, sets the flag, and the call reports it
    for badcol in (100, -1, 2**31 - 1):
        c = col.copy()
        c[17] = badcol
        with pytest.raises(RuntimeError, match="column index out of range"):
            gdd.graph.locality_order(_graph(rowptr, c), "community", sweeps=2)
    # the sweeps keyword is accepted and ignored by the other kinds
    assert torch.equal(gdd.graph.locality_order(g, "degree", sweeps=3), gdd.graph.locality_order(g, "degree"))
    with pytest.raises(ValueError, match="unknown locality order"):
        gdd.graph.locality_order(g, "nope")
