"""gdd.rankeval on the device: the fused score + top-K kernel, the metrics kernel, the evaluator
and the teacher's NDCG selection, against tests/rankeval_ref.py (fp64 numpy) and the reference's
recorded metrics.

Bounds (none measured on the device first).

* Grid inputs (entries in {-2..2}/2, d <= 256): every product is a multiple of 1/4 and every partial
  sum is below 2^10, so the fp32 chain is exact whatever its order; lists must equal the stable
  sort of the fp64 scores and the scores must match bit for bit.
* Random normal inputs: the score is a chain of d fmas, so it lies within gamma sum_f |u_f v_f| of the
  exact dot product, gamma = d 2^-24 / (1 - d 2^-24) (the standard bound for a recursive sum of d
  products, each fma rounding once). The fp64 reference's own error (d 2^-53) is far below. A list
  is then judged on three properties that hold for any correct selection: each score within its
  bound, the list strictly ordered by (returned score descending, item ascending), and no omitted
  item's exact score above the list's smallest exact score by more than the two items' bounds.
* Metrics: the kernel and the definition do the same fp64 operations in the same rank order except
  for the final sum over users (a fixed tree against numpy's pairwise sum): rel 1e-12.
* Against the reference's fp32 metrics: rel 5e-5 (test_rankeval_host.py).
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rankeval_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32) + np.float32(0.0)).view(np.uint32)


def random_mask(rng, nu, I, frac=0.05):
    M = rng.random_sample((nu, I)) < frac
    r, c = np.nonzero(M)
    return R.csr_of(r, c, nu)


def dev_off4(a):
    """``a`` on the device, contiguous, its first element 4 bytes past a 16-byte boundary."""
    flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = flat[1:1 + a.size].view(*a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


def device_lists(U, V, k, users=None, mask=None, mask_value=-1024.0, vdev=dev):
    import gdd
    Vt = vdev(V)
    items, scores = gdd.recommend(dev(U), Vt, k, users=users, exclude=mask, mask_value=mask_value,
                                  return_scores=True)
    assert items.dtype == torch.int32 and scores.dtype == torch.float32 and items.is_cuda
    return items.cpu().numpy(), scores.cpu().numpy()


def reference_lists(U, V, k, users=None, mask=None, mask_value=-1024.0):
    sel = np.arange(U.shape[0]) if users is None else np.asarray(users)
    m = None if mask is None else R.take_rows(mask[0], mask[1], sel)
    return R.ranked(R.scores64(U, V, sel, m, mask_value), k)


# (I, K, d, B): every I, K, d and B of the issue's cross at least once; K = I where I <= 256. The
# last three select the prefetch depths on both sides of their edges: d = 68 and 128 stage a tile in
# eight float4 per thread, d = 132 in sixteen (d = 64 in four, d = 256 in sixteen, above).
GRID_CASES = [(1, 1, 1, 1), (63, 5, 3, 7), (63, 63, 64, 7), (64, 64, 65, 7), (64, 20, 200, 1), (65, 65, 256, 7),
              (65, 1, 64, 300), (257, 256, 3, 7), (257, 20, 65, 300), (1000, 256, 64, 7), (1000, 5, 200, 300),
              (1000, 64, 256, 7), (1000, 20, 1, 300), (1000, 1, 3, 1),
              (65, 65, 68, 7), (257, 20, 128, 17), (257, 5, 132, 7)]


@pytest.mark.parametrize("I,K,d,B", GRID_CASES)
def test_grid_inputs_lists_and_scores_are_exact(I, K, d, B):
    check_grid_case(I, K, d, B, dev)


def test_grid_inputs_item_table_off_16_byte_alignment():
    """d = 64 with the item table 4 bytes past a 16-byte boundary: d % 4 == 0, yet the tile is staged
    float by float."""
    check_grid_case(257, 65, 64, 17, dev_off4)


def check_grid_case(I, K, d, B, vdev):
    rng = np.random.RandomState(I * 7 + K * 3 + d + B)
    nu = B + 5
    U, V = R.grid(rng, nu, d), R.grid(rng, I, d)
    users = rng.permutation(nu)[:B]
    if B > 1:
        users[-1] = users[0]  # a repeated id
    mask = random_mask(rng, nu, I)
    got_i, got_s = device_lists(U, V, K, users, mask, vdev=vdev)
    ref_i, ref_s = reference_lists(U, V, K, users, mask)
    assert np.array_equal(got_i, ref_i)
    assert np.array_equal(bits(got_s), bits(ref_s))
    if B > 1:
        assert np.array_equal(got_i[-1], got_i[0])


def test_all_users_in_table_order_is_the_default():
    rng = np.random.RandomState(3)
    U, V = R.grid(rng, 37, 5), R.grid(rng, 130, 5)
    got_i, got_s = device_lists(U, V, 9)
    ref_i, ref_s = reference_lists(U, V, 9)
    assert np.array_equal(got_i, ref_i) and np.array_equal(bits(got_s), bits(ref_s))


def test_threshold_scheme_adversaries():
    """I = 5000, K = 256, d = 1: scores strictly ascending in the item id (every item beats the running
    threshold), strictly descending, and all zero (only the tie rule orders the list)."""
    I, K = 5000, 256
    V = (np.arange(I, dtype=np.float32) / 8.0).reshape(I, 1)
    U = np.array([[1.0], [-1.0], [0.0]], np.float32)
    got_i, got_s = device_lists(U, V, K)
    assert np.array_equal(got_i[0], np.arange(I - 1, I - 1 - K, -1))
    assert np.array_equal(got_i[1], np.arange(K)) and np.array_equal(got_i[2], np.arange(K))
    assert np.array_equal(bits(got_s[0]), bits(V[got_i[0], 0]))
    assert np.array_equal(bits(got_s[1]), bits(-V[:K, 0])) and np.array_equal(bits(got_s[2]), bits(np.zeros(K)))


@pytest.mark.parametrize("mask_value", [-1024.0, -1e9])
def test_masked_items_fill_the_tail(mask_value):
    """A user with all but 3 of 200 items masked (a mask row longer than one 64-item tile) and K = 10:
    the three unmasked items, then masked items in ascending id, scored mask_value."""
    rng = np.random.RandomState(5)
    I, K = 200, 10
    U, V = R.grid(rng, 4, 8), R.grid(rng, I, 8)
    keep = np.array([7, 64, 199])
    r1 = np.setdiff1d(np.arange(I), keep)
    rows = np.concatenate([np.full(r1.shape[0], 1), [3, 3]])
    mask = R.csr_of(rows, np.concatenate([r1, [0, 150]]), 4)  # users 0 and 2: empty rows
    got_i, got_s = device_lists(U, V, K, None, mask, mask_value)
    ref_i, ref_s = reference_lists(U, V, K, None, mask, mask_value)
    assert np.array_equal(got_i, ref_i) and np.array_equal(bits(got_s), bits(ref_s))
    assert sorted(got_i[1, :3]) == list(keep) and np.array_equal(got_i[1, 3:], r1[:7])
    assert np.array_equal(bits(got_s[1, 3:]), bits(np.full(7, mask_value)))
    # an empty mask is no mask
    empty = (np.zeros(5, np.int32), np.zeros(0, np.int32))
    a = device_lists(U, V, K, None, empty, mask_value)
    b = device_lists(U, V, K, None, None, mask_value)
    assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))


def test_a_row_is_a_function_of_its_user_alone():
    """Random floats: the full call, per-user calls (B = 1), another order of the users and a second
    run give the same items and the same score bits per user."""
    rng = np.random.RandomState(11)
    nu, I, d, K = 21, 300, 65, 20
    U, V = rng.randn(nu, d).astype(np.float32), rng.randn(I, d).astype(np.float32)
    mask = random_mask(rng, nu, I)
    full_i, full_s = device_lists(U, V, K, None, mask)
    again_i, again_s = device_lists(U, V, K, None, mask)
    assert np.array_equal(full_i, again_i) and np.array_equal(bits(full_s), bits(again_s))
    order = rng.permutation(nu)
    perm_i, perm_s = device_lists(U, V, K, order, mask)
    assert np.array_equal(perm_i, full_i[order]) and np.array_equal(bits(perm_s), bits(full_s[order]))
    wide_i, wide_s = device_lists(U, V, 2 * K, None, mask)  # another K: a prefix
    assert np.array_equal(wide_i[:, :K], full_i) and np.array_equal(bits(wide_s[:, :K]), bits(full_s))
    for u in (0, 7, 20):
        one_i, one_s = device_lists(U, V, K, [u], mask)
        assert np.array_equal(one_i[0], full_i[u]) and np.array_equal(bits(one_s[0]), bits(full_s[u]))


@pytest.mark.parametrize("d", [64, 200])
def test_random_floats_within_the_chain_bound(d):
    rng = np.random.RandomState(d)
    B, I, K = 64, 3000, 50
    U, V = rng.randn(B, d).astype(np.float32), rng.randn(I, d).astype(np.float32)
    got_i, got_s = device_lists(U, V, K)
    S = R.scores64(U, V)
    mag = np.abs(U.astype(np.float64)) @ np.abs(V.astype(np.float64)).T
    gamma = d * 2.0 ** -24 / (1.0 - d * 2.0 ** -24)
    bound = gamma * mag
    rows = np.arange(B)[:, None]
    err = np.abs(got_s.astype(np.float64) - S[rows, got_i])
    print(f"d={d}: largest err/bound {float((err / bound[rows, got_i]).max()):.3f}")
    assert (err <= bound[rows, got_i]).all()
    for b in range(B):
        assert len(set(got_i[b])) == K and got_i[b].min() >= 0 and got_i[b].max() < I
        s, it = got_s[b], got_i[b]
        assert all(s[r] > s[r + 1] or (s[r] == s[r + 1] and it[r] < it[r + 1]) for r in range(K - 1))
        low = it[np.argmin(S[b, it])]
        out = np.setdiff1d(np.arange(I), it)
        assert (S[b, out] - S[b, low] <= bound[b, out] + bound[b, low]).all()


def test_metrics_kernel_equals_the_definition():
    """gdd_rank_metrics on the kernel's own lists: a hit exactly at rank k - 1 and one at rank k,
    n > k, n = 0 (not counted), te_deg above the row length, topks [1, 5, 20]."""
    import gdd
    rng = np.random.RandomState(9)
    B, I, K, topks = 40, 300, 20, (1, 5, 20)
    U, V = R.grid(rng, B, 6), R.grid(rng, I, 6)
    lists = gdd.recommend(dev(U), dev(V), K)
    L = lists.cpu().numpy()
    rows, cols = [], []
    deg = np.zeros(B, np.int64)

    def give(b, items, n=None):
        rows.extend([b] * len(items))
        cols.extend(int(i) for i in items)
        deg[b] = len(set(int(i) for i in items)) if n is None else n

    give(0, [L[0, 4], L[0, 5]])  # rank k - 1 and rank k of k = 5
    give(1, list(L[1, [0, 19]]) + list(np.setdiff1d(np.arange(I), L[1])[:28]))  # n = 30 > 20
    give(3, [L[3, 0], L[3, 2]], n=5)  # repeated lines: n above the row length
    give(4, np.setdiff1d(np.arange(I), L[4])[:3])  # no hit
    for b in range(5, B):
        give(b, rng.permutation(I)[:rng.randint(1, 40)])
    te_ptr, te_col = R.csr_of(rows, cols, B)  # user 2: no items, n = 0
    per, sums, count = gdd.rank_metrics(lists, dev(te_ptr), dev(te_col), dev(deg.astype(np.int32)), topks)
    ref_per, ref_sums, ref_count = R.metrics(L, te_ptr, te_col, deg, topks)
    per, sums = per.cpu().numpy(), sums.cpu().numpy()
    assert int(count.item()) == ref_count == B - 1
    assert per.shape == (B, 3, 3) and np.array_equal(per[2], np.zeros((3, 3)))
    assert np.array_equal(per[0, 0], [0.0, 1 / 5, 2 / 20]) and np.array_equal(per[0, 1], [0.0, 1 / 2, 2 / 2])
    assert np.array_equal(per[1, 1], [1 / 1, 1 / 5, 2 / 20]) and np.array_equal(per[3, 1], [1 / 1, 2 / 5, 2 / 5])
    assert np.array_equal(per[4], np.zeros((3, 3)))
    assert np.allclose(per, ref_per, rtol=1e-12, atol=0) and np.allclose(sums, ref_sums, rtol=1e-12, atol=0)
    # te_deg omitted: the row length
    per2, _, _ = gdd.rank_metrics(lists, dev(te_ptr), dev(te_col), None, topks)
    ref2, _, _ = R.metrics(L, te_ptr, te_col, None, topks)
    assert np.allclose(per2.cpu().numpy(), ref2, rtol=1e-12, atol=0)


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def fixture_evaluator(fx, **kw):
    import gdd
    n, m = int(fx["n"]), int(fx["m"])
    train = sp.coo_matrix((np.ones(fx["train_u"].shape[0], np.float32), (fx["train_u"], fx["train_i"])),
                          shape=(n, m)).tocsr()
    topks = tuple(int(k) for k in fx["topks"])
    return gdd.RankingEvaluator(train, fx["valid_u"], fx["valid_i"], topks, "cuda", **kw)


def test_fixture_on_the_device_equals_the_reference(fx):
    ev = fixture_evaluator(fx)
    m = ev(dev(fx["U"]), dev(fx["V"]))
    assert m["users"] == int(fx["ref_count"])
    ref = R.fixture_reference_run(fx, ev.topks)
    assert np.array_equal(ev.ranked(dev(fx["U"]), dev(fx["V"])).cpu().numpy(), ref["lists"])
    for j, name in enumerate(("precision", "recall", "ndcg")):
        assert m[name].dtype == np.float64 and m[name].shape == (4,)
        rel = np.abs(m[name] - fx["ref_" + name]) / np.abs(fx["ref_" + name])
        print(f"{name}: rel to the reference {rel}")
        assert (rel <= 5e-5).all()
        assert np.allclose(m[name], ref["means"][j], rtol=1e-12, atol=0)
    again = ev(dev(fx["U"]), dev(fx["V"]))
    assert all(np.array_equal(m[k], again[k]) for k in ("precision", "recall", "ndcg"))


def test_hits_agree_with_the_recall_kernel(fx):
    """mask_value -1e9 as the driver's evaluator uses: sum of hits@20 over the users / total pairs is
    recsys.recall_at_k's number exactly."""
    import gdd
    from gdd import recsys
    n, m = int(fx["n"]), int(fx["m"])
    train = sp.coo_matrix((np.ones(fx["train_u"].shape[0], np.float32), (fx["train_u"], fx["train_i"])),
                          shape=(n, m)).tocsr()
    U, V = dev(fx["U"]), dev(fx["V"])
    ev = gdd.RankingEvaluator(train, fx["valid_u"], fx["valid_i"], (20,), "cuda", mask_value=-1e9,
                              count_repeats=False)
    lists = ev.ranked(U, V)
    g = ev._dev
    per, _, _ = gdd.rank_metrics(lists, g["te_ptr"], g["te_col"], None, (20,))
    hits = int(np.rint(per[:, 0, 0].cpu().numpy() * 20).sum())
    total = int(g["te_col"].numel())
    old = recsys.recall_at_k(U, V, train, fx["valid_u"], fx["valid_i"], 20, "cuda")
    assert hits > 0 and float(hits / max(1, total)) == old


def test_bad_ids_are_reported_and_not_read():
    """A user id outside [0, nu) and a mask column outside [0, I): the guard counts the rows and
    fills them with -1 without reading through the id; the other rows are right."""
    import gdd
    from gdd import rankeval
    rng = np.random.RandomState(13)
    nu, I, K = 9, 150, 12
    U, V = R.grid(rng, nu, 7), R.grid(rng, I, 7)
    users = np.array([3, nu + 4, 0, -1, 8, 3], np.int32)
    mask = random_mask(rng, nu, I)
    mrows = R.take_rows(mask[0], mask[1], np.clip(users, 0, nu - 1))
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    items, scores = rankeval._score_topk(dev(U), dev(V), K, dev(users), (dev(mrows[0]), dev(mrows[1])), -1024.0,
                                         True, bad)
    good = [0, 2, 4, 5]
    ref_i, ref_s = reference_lists(U, V, K, users[good], mask)
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    assert int(bad.item()) == 2
    assert (items[[1, 3]] == -1).all() and np.isnan(scores[[1, 3]]).all()
    assert np.array_equal(items[good], ref_i) and np.array_equal(bits(scores[good]), bits(ref_s))
    # mask columns: one past the table in user 2's row, a negative one in user 5's
    ptr, col = mask
    rows = np.repeat(np.arange(nu), np.diff(ptr))
    col2 = np.concatenate([col, [I + 5, -2]]).astype(np.int64)
    rows2 = np.concatenate([rows, [2, 5]])
    order = np.lexsort((col2, rows2))
    ptr2 = np.searchsorted(rows2[order], np.arange(nu + 1)).astype(np.int32)
    col2 = col2[order].astype(np.int32)
    bad.zero_()
    items, _ = rankeval._score_topk(dev(U), dev(V), K, None, (dev(ptr2), dev(col2)), -1024.0, False, bad)
    items = items.cpu().numpy()
    ok = [u for u in range(nu) if u not in (2, 5)]
    assert int(bad.item()) == 2 and (items[[2, 5]] == -1).all()
    assert np.array_equal(items[ok], reference_lists(U, V, K, None, mask)[0][ok])
    with pytest.raises(RuntimeError, match="out of range"):
        gdd.recommend(dev(U), dev(V), K, exclude=(ptr2, col2))


def teacher_data():
    rng = np.random.RandomState(4)
    n, m = 60, 80
    key = rng.permutation(n * m)[:900]
    tr, va, te = key[:600], key[600:750], key[750:]
    return n, m, (tr // m, tr % m), (va // m, va % m), (te // m, te % m)


def run_teacher():
    from gdd.rankformer import train_teacher
    n, m, tr, va, te = teacher_data()
    lines = []
    model, hist = train_teacher(n, m, tr[0], tr[1], va[0], va[1], hidden_dim=16, max_epochs=6, valid_interval=2,
                                select_by="ndcg", topks=[5, 20], test_u=te[0], test_i=te[1], seed=7,
                                log=lines.append)
    return model, hist, lines


def test_teacher_selects_on_validation_ndcg():
    import gdd
    model, hist, lines = run_teacher()
    assert [e for e, _ in hist["valid"]] == [0, 2, 4, 6] and hist["topks"] == [5, 20]
    ndcg = [float(m["ndcg"][-1]) for _, m in hist["valid"]]
    best = max(ndcg)
    want = hist["valid"][ndcg.index(best)][0] if best > 0 else 0
    assert hist["best_epoch"] == want and hist["best_ndcg"] == (best if best > 0 else 0.0)
    n, m, tr, va, te = teacher_data()
    fresh = gdd.RankingEvaluator(model.graph.to_scipy(), te[0], te[1], (5, 20), "cuda")
    model.eval()
    with torch.no_grad():
        users, items = model.computer()
        again = fresh(users, items)
    assert best > 0 and hist["test"] is not None
    for k in ("precision", "recall", "ndcg"):
        assert np.array_equal(hist["test"][k], again[k])
    assert hist["test"]["users"] == again["users"] == np.unique(te[0]).shape[0]
    text = "\n".join(lines)
    assert "ndcg@20 = " in text and "recall@5 = " in text and "pre@20 = " in text
    _, hist2, lines2 = run_teacher()
    assert lines2 == lines and hist2["loss"] == hist["loss"] and hist2["best_epoch"] == hist["best_epoch"]
    for (_, a), (_, b) in zip(hist["valid"], hist2["valid"]):
        assert all(np.array_equal(a[k], b[k]) for k in ("precision", "recall", "ndcg"))
