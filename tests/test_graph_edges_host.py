"""Host-side checks of the graph front end (no GPU): the hop's form selection (gdd_hop_path), the
oracle's normalisation and SpMM against references that share no code with it (graph_ref), and the
worst cases of the propagation workspace's size formulas."""
import os
import subprocess

import numpy as np
import pytest

import graph_ref as R
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

HOP_FORMS = R.HOP_FORMS


@pytest.fixture(scope="module")
def lib():
    from gdd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "graph-distillation-for-recommendation_amd",
                                                   "csrc")], check=True)
    return _lib.load()


def hop_form_py(d, align):
    """The dispatch restated: floats per lane from divisibility and alignment, lanes per item from
    the lane count (with the two-slice exception for 29..32 float4 lanes), slices from the number of
    G*V feature chunks."""
    if d % 4 == 0 and align == 16:
        V = 4
    elif d % 2 == 0 and align >= 8:
        V = 2
    else:
        V = 1
    lanes = -(-d // V)
    if lanes <= 16 or (V == 4 and 28 < lanes <= 32):
        G = 16
    elif lanes <= 32:
        G = 32
    else:
        G = 64
    chunks = -(-d // (G * V))
    S = chunks if chunks in (1, 2, 4, 8) else 0
    return f"v{V}/g{G}/s{S}"


def test_hop_path_table(lib):
    for d, align, form in HOP_FORMS:
        assert lib.gdd_hop_path(d, align) == form.encode(), (d, align)
        assert hop_form_py(d, align) == form, (d, align)


def test_hop_path_matches_restated_dispatch(lib):
    seen = set()
    for align in (16, 8, 4):
        for d in range(1, 2305):
            got = lib.gdd_hop_path(d, align).decode()
            assert got == hop_form_py(d, align), (d, align)
            seen.add(got)
    # every instantiated (V, G, S) that a width up to 2304 can reach was named at least once
    for V in (4, 2, 1):
        for S in (8, 4, 2, 1, 0):
            assert f"v{V}/g64/s{S}" in seen
        assert f"v{V}/g16/s1" in seen and f"v{V}/g32/s1" in seen
    assert "v4/g16/s2" in seen


@pytest.mark.parametrize("d,align", [(0, 16), (-4, 16), (128, 0), (128, 2), (128, 32), (128, 12),
                                     (128, -16), (0, 0)])
def test_hop_path_invalid(lib, d, align):
    assert lib.gdd_hop_path(d, align) == b"invalid"


# ---- oracle vs the independent references ---------------------------------------------------------
GRAPHS = {
    "ladder_binary": lambda: R.ladder_graph(),
    "ladder_weighted": lambda: R.ladder_graph(weighted=True),
    "diag_cases": lambda: R.diag_cases_graph(),
    "sparse_runs_exact": lambda: R.sparse_runs_graph(True),
    "sparse_runs_inexact": lambda: R.sparse_runs_graph(False),
}


@pytest.mark.parametrize("self_loops", [-1, 0, 1])
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_oracle_normalize_matches_ref(name, self_loops):
    A = GRAPHS[name]()
    rp, col, val = R.csr_arrays(A)
    binary = bool((val == 1).all())
    ro, co, vo = O.normalize_csr(rp, col, None if binary else val, self_loops)
    rr, cr, vr = R.normalize_ref(A, R.adds_identity(A, self_loops))
    assert np.array_equal(ro, rr)
    assert np.array_equal(co, cr)
    assert np.array_equal(R.bits(vo), R.bits(vr))


def test_graphs_hold_their_edges():
    """The builders deliver the row lengths and block layouts the GPU tests rely on."""
    A = R.ladder_graph()
    lens = np.diff(A.indptr)
    assert [int(lens[r]) for r in R.ladder_rows()] == list(R.LADDER_LENGTHS)
    assert lens.max() == 768 and np.delete(lens, R.ladder_rows()).max() <= 11
    D = R.diag_cases_graph()
    for i, (below, above, stored) in R.diag_case_rows():
        c = D.indices[D.indptr[i]:D.indptr[i + 1]]
        assert (c < i).sum() == below and (c > i).sum() == above
        assert ((c == i).sum() == 1) == (stored is not None)
        if stored is not None:
            assert c[stored - 1] == i
    assert sorted({i % 4 for i, _ in R.diag_case_rows()}) == [0, 1, 2, 3]
    for exact in (True, False):
        S = R.sparse_runs_graph(exact)
        rp = S.indptr
        assert rp[1] == 0 and np.all(np.diff(rp)[-R.SPARSE_TAIL:] == 0)
        first, last, span = R.fill_block_ranges(rp)
        assert span.max() > 512                                # the global-search branch
        assert (span <= 512).any()                             # and the staged one
        assert np.any((first == R.SPARSE_HUB_ROW) & (last == R.SPARSE_HUB_ROW))  # inside the hub
        assert S[R.SPARSE_HUB_ROW, R.SPARSE_HUB_ROW] == 1 and S[R.SPARSE_HUB_ROW + 1, R.SPARSE_HUB_ROW + 1] == 1


SPMM_WIDTHS = [1, 31, 255, 450, 511, 1022, 1024, 2048]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("d", SPMM_WIDTHS)
def test_oracle_spmm_within_ref64_bound(d, weighted):
    A = R.ladder_graph(weighted=weighted, signed=True)
    rp, col, val = R.csr_arrays(A)
    x = np.random.default_rng(d).standard_normal((A.shape[0], d)).astype(np.float32)
    y = O.spmm(rp, col, val, x, scale=0.7)
    y64, bound = R.spmm_ref64(A, x, 0.7)
    err = np.abs(y.astype(np.float64) - y64)
    assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    assert np.all(y[np.diff(rp) == 0] == 0)  # empty rows: bound 0, exact zeros


# ---- workspace formulas ---------------------------------------------------------------------------
def _plan_counts(lengths):
    """k_seg_counts / k_make_items restated: a row of up to 256 entries is one work item, a longer
    one ceil(len / 256) items with one partial slot each, and is listed as a split row."""
    lengths = np.asarray(lengths, np.int64)
    nseg = np.where(lengths <= R.SEG, 1, -(-lengths // R.SEG))
    return int(nseg.sum()), int(nseg[nseg > 1].sum()), int((nseg > 1).sum())


@pytest.mark.parametrize("case", ["rows_of_257", "ladder", "one_full_segment_each", "single_hub"])
def test_workspace_formulas_cover_worst_cases(case):
    lengths = {
        "rows_of_257": [257] * 1100,  # the most split rows and slots per entry
        "ladder": np.diff(R.ladder_graph().indptr),
        "one_full_segment_each": [256] * 300,
        "single_hub": [0] * 10 + [256 * 40 + 1],
    }[case]
    n, nnz = len(lengths), int(np.sum(lengths))
    items, slots, split = _plan_counts(lengths)
    assert items <= n + nnz // R.SEG + 1   # max_items_for (gdd_propagate.hip)
    assert slots <= 2 * (nnz // R.SEG) + 2  # max_parts_for
    assert split <= nnz // R.SEG + 1        # carve_plan's max_long
    if case == "rows_of_257":
        assert split == 1100 and slots == 2200 and split > 1024  # more split rows than k_fixup has blocks
