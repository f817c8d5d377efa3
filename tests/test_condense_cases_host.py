"""CPU: the conditions that keep tests/test_gpu_condense_forms.py honest, asserted from the oracle
(oracle/condense.py) and the inputs of tests/condense_cases.py alone.

* the oracle's row sums and cosines equal an independent statement of the same order;
* on the long rows that order differs from the two orders a parallel kernel would most easily
  produce instead, so a wrong order cannot pass by coincidence;
* at every (weights, m) of the device's tie cases the threshold value is tied, some of the ties are
  taken and some left, and the ties taken and the ties left do not lie in one 4096-edge block — so
  the cap on the ties (`min(pe, rem)` in k_tk_emit) acts across blocks. m = nnz takes everything:
  there the condition cannot hold and the test states so."""
import numpy as np
import pytest

import condense_cases as CC
from oracle import condense as O


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_long_row_graph_shape():
    rowptr, col, val, n = CC.long_row_graph()
    cnt = np.diff(rowptr)
    assert n == 12300 and len(rowptr) == n + 1 and rowptr[-1] == len(col) == len(val)
    for r, L in CC.LONG_ROWS.items():
        assert cnt[r] == L
    rest = np.delete(cnt, list(CC.LONG_ROWS))
    assert rest.min() >= 1 and rest.max() <= 11
    assert 100_000 < len(col) < 125_000
    assert col.min() >= 0 and col.max() < n
    inner = np.ones(len(col), bool)
    inner[rowptr[:-1]] = False  # first entry of each row
    assert np.all(np.diff(col.astype(np.int64))[inner[1:]] > 0)  # distinct and ascending per row
    # not symmetric: row 200 holds nearly every column, few rows hold column 200
    rows = O.coo_rows(rowptr)
    assert set(col[rows == 200].tolist()) != set(rows[col == 200].tolist())
    # every long row is also some edge's column, so `er` reads its degree on both sides
    assert set(CC.LONG_ROWS) <= set(col.tolist())


def test_oracle_row_sums_are_the_sequential_sum():
    rowptr, col, val, n = CC.long_row_graph()
    got = O.row_sums(rowptr, val)
    want = np.array([np.cumsum(val[rowptr[r]:rowptr[r + 1]], dtype=np.float32)[-1] for r in range(n)],
                    np.float32)
    assert np.array_equal(_bits(got), _bits(want))


def test_order_shows_on_every_row_of_4096_or_more():
    rowptr, col, val, n = CC.long_row_graph()
    checked = 0
    for r, L in CC.LONG_ROWS.items():
        if L < 4096:
            continue
        v = val[rowptr[r]:rowptr[r + 1]]
        seq = np.cumsum(v, dtype=np.float32)[-1]
        assert seq != np.float32(np.sum(v)), r                      # numpy's pairwise order
        assert seq != np.float32(np.sum(v.astype(np.float64))), r  # the exact sum, rounded
        checked += 1
    assert checked == 5


def test_oracle_cosine_is_the_plain_loop_at_40_classes():
    rowptr, col, val, n = CC.small_graph()
    rows = O.coo_rows(rowptr)
    xu = O.row_unit(CC.embeddings(n, 40))
    cos = O.edge_cosine(xu, rows, col)
    pick = np.random.default_rng(3).choice(len(col), 200, replace=False)
    for e in pick:
        s = np.float32(0)
        for j in range(40):
            s = np.float32(s + np.float32(xu[rows[e], j] * xu[col[e], j]))
        assert s.view(np.uint32) == cos[e].view(np.uint32)


def test_zero_embedding_rows_give_nan_er():
    rowptr, col, val, n = CC.small_graph()
    er, rew = O.attaw_er(rowptr, col, val, CC.embeddings(n, 4))
    for r in CC.ZERO_ROWS:
        assert np.all(rew[rowptr[r]:rowptr[r + 1]] == 0) and np.isnan(er[rowptr[r]:rowptr[r + 1]]).all()


def _assert_straddling_ties(w, m, nnz):
    thr, taken, left = CC.tie_split(w, m)
    if m == nnz:  # everything is taken: nothing can be left
        assert len(left) == 0 and len(taken) >= 2
        return thr
    assert len(taken) + len(left) >= 2
    assert len(taken) > 0 and len(left) > 0
    # a tie taken and a tie left in different blocks (the taken ones are the lower ids)
    assert taken.min() // CC.BLK < left.max() // CC.BLK
    return thr


@pytest.mark.parametrize("kind", ["ints", "equal", "mixed"])
def test_ties_straddle_blocks(kind):
    nnz = CC.TOPK_NNZ
    w = CC.tie_weights(nnz, kind)
    assert len(w) == nnz
    thrs = {m: _assert_straddling_ties(w, m, nnz) for m in CC.topk_ms(nnz)}
    if kind == "mixed":
        assert np.isnan(thrs[1])  # NaN is the largest
        assert thrs[nnz // 2] == 0.0  # +0 and -0 tie at the cut
        assert np.isfinite(thrs[3 * nnz // 4]) and thrs[3 * nnz // 4] < 0  # the ~u key branch
        assert thrs[nnz - 1] == -np.inf
        for s in (np.inf, -np.inf, np.float32(1e-40), np.float32(-1e-40)):
            assert np.count_nonzero(w == s) >= 2
        assert np.count_nonzero(np.isnan(w)) >= 2
        z = w == 0
        assert np.count_nonzero(z & np.signbit(w)) >= 2 and np.count_nonzero(z & ~np.signbit(w)) >= 2


def test_ties_straddle_blocks_in_the_two_pass_scan():
    nnz = CC.TOPK_NNZ_BIG
    assert (nnz + CC.BLK - 1) // CC.BLK == 258  # more blocks than scan lanes: two blocks per lane
    w = CC.tie_weights(nnz, "ints1000")
    for m in CC.topk_ms_big(nnz):
        thr, taken, left = CC.tie_split(w, m)
        _assert_straddling_ties(w, m, nnz)
        assert len(taken) + len(left) > 900  # about nnz / 1000 ties at any threshold


@pytest.mark.parametrize("n,nsets,ms", [(130, 3, (1, 5000, 16899)), (130, 4, (1, 5000, 16899)),
                                        (1040, 2, (1040 * 1040 // 3,))])
def test_class_products_tie_across_blocks(n, nsets, ms):
    rowptr, rows, col = CC.complete_graph(n)
    probs, er = CC.complete_weights(n, nsets)
    nnz = n * n
    assert (nnz + CC.BLK - 1) // CC.BLK == (5 if n == 130 else 265)
    for i in range(nsets):
        w = O.class_weights(probs, er, rows, col, i)
        for m in ms:
            _assert_straddling_ties(w, m, nnz)
