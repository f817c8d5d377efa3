"""gdd.condrank on the device: lists from the condensed model's cluster tables against
gdd.recommend on the expanded tables cu_z[u2cu], ci_z[i2ci].

The contract is equality, not a bound: the score of a (user, item) pair is one fp32 fma chain over
the two rows alone, the expanded rows are copies of the cluster rows, so every score has the same
bits on both paths and the lists must agree in every item and every score bit (array_equal on ids
and on bit patterns). On grid inputs (tests/rankeval_ref.py: chains exact in any order) both must
also equal the stable sort of the fp64 scores. Which users are recomputed against the expanded item
table is compared with the numpy model of the completion rule in tests/condrank_ref.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import condrank_ref as C  # noqa: E402
import rankeval_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def labels(rng, n, k):
    """n labels over k clusters, every cluster used when n >= k, in shuffled order."""
    lab = np.concatenate([np.arange(min(n, k)), rng.randint(0, k, max(0, n - k))])
    return rng.permutation(lab).astype(np.int64)


def random_mask(rng, nu, I, frac=0.02):
    r, c = np.nonzero(rng.random_sample((nu, I)) < frac)
    return R.csr_of(r, c, nu)


def check(cu, ci, u2cu, i2ci, k, users=None, mask=None, mask_value=-1024.0, exact=True):
    """Run both device paths and assert the contract; returns (recommender, items, scores) on the host."""
    import gdd
    cu_t, ci_t = dev(cu), dev(ci)
    rec = gdd.CondensedRecommender(cu_t, ci_t, u2cu, i2ci)
    items, scores = rec.recommend(k, users=users, exclude=mask, mask_value=mask_value, return_scores=True)
    assert items.dtype == torch.int32 and scores.dtype == torch.float32 and items.is_cuda
    want_i, want_s = gdd.recommend(cu_t[dev(u2cu)], ci_t[dev(i2ci)], k, users=users, exclude=mask,
                                   mask_value=mask_value, return_scores=True)
    assert items.shape == want_i.shape
    assert np.array_equal(items.cpu().numpy(), want_i.cpu().numpy())
    assert np.array_equal(bits(scores), bits(want_s))
    if exact:
        sel = np.arange(len(u2cu)) if users is None else np.asarray(users)
        m = None if mask is None else R.take_rows(mask[0], mask[1], sel)
        ref_i, ref_s = C.expanded_reference(cu, ci, u2cu, i2ci, k, sel, m, mask_value)
        assert np.array_equal(items.cpu().numpy(), ref_i)
        assert np.array_equal(scores.cpu().numpy(), ref_s.astype(np.float32))
    return rec, items.cpu().numpy(), scores.cpu().numpy()


# K, d, B (None: users=None; "rep": 7 ids with a repeat), num_ci, num_cu: K in {1, 20, 64, 65, 256},
# d in {1, 3, 64, 65, 256}, B in {1, 7, 300}, num_ci in {1, 5, 256}, num_cu in {1, 9}, every value at
# least once; L == num_ci throughout, so no user can be recomputed and the walk itself is checked
CROSS = [(1, 1, 1, 1, 1), (20, 3, 7, 5, 9), (64, 64, 300, 256, 9), (65, 65, None, 256, 1), (256, 256, "rep", 5, 9),
         (20, 64, 300, 1, 9), (256, 1, 1, 256, 9), (65, 3, None, 5, 1), (1, 256, 300, 256, 9), (64, 65, 7, 1, 1),
         (20, 256, None, 256, 9), (256, 64, 300, 5, 9)]


@pytest.mark.parametrize("K,d,B,num_ci,num_cu", CROSS)
def test_grid_cross(K, d, B, num_ci, num_cu):
    rng = np.random.RandomState(K * 1000 + d)
    nu, I = 40, 1000
    cu, ci = R.grid(rng, num_cu, d), R.grid(rng, num_ci, d)
    u2cu, i2ci = labels(rng, nu, num_cu), labels(rng, I, num_ci)
    if B is None:
        users = None
    elif B == "rep":
        users = np.array([5, 39, 5, 0, 17, 5, 8])
    else:
        users = rng.randint(0, nu, B)
    rec, items, _ = check(cu, ci, u2cu, i2ci, K, users, random_mask(rng, nu, I))
    assert rec.last_info == {"fallback_users": 0, "ranked_clusters": len(np.unique(u2cu if users is None
                                                                                    else u2cu[users])),
                             "list_len": num_ci}
    assert all(len(set(row)) == K for row in items.tolist())


def sized_clusters(rng):
    """692 items: 200 clusters of one item, clusters of 63, 64, 65 and 300, and 6 empty clusters."""
    sizes = [1] * 100 + [0, 0, 63, 64, 0, 65, 300, 0] + [1] * 100 + [0, 0]
    lab = np.repeat(np.arange(len(sizes)), sizes)
    return rng.permutation(lab).astype(np.int64), len(sizes), sizes


@pytest.mark.parametrize("K", [20, 256])
def test_cluster_sizes(K):
    rng = np.random.RandomState(11)
    i2ci, num_ci, sizes = sized_clusters(rng)
    assert num_ci <= 256 and sorted(set(sizes)) == [0, 1, 63, 64, 65, 300]
    d, num_cu, nu = 8, 6, 30
    cu, ci = R.grid(rng, num_cu, d), R.grid(rng, num_ci, d)
    ci[sizes.index(300)] = np.sign(cu[0]) + (cu[0] == 0)  # the 300-member cluster is cluster 0's best or tied
    u2cu = labels(rng, nu, num_cu)
    rec, items, _ = check(cu, ci, u2cu, i2ci, K, None, random_mask(rng, nu, len(i2ci)))
    assert rec.last_info["fallback_users"] == 0 and rec.last_info["list_len"] == num_ci
    big = np.nonzero(i2ci == sizes.index(300))[0]
    if K == 20:  # the per-cluster quota is in play: some user's list draws on the big cluster
        assert any(np.isin(row, big).sum() > 0 for row in items)


def test_duplicate_cluster_rows_interleave_by_item_id():
    rng = np.random.RandomState(12)
    d, num_cu, num_ci, nu, I, K = 4, 3, 12, 9, 240, 30
    cu, ci = R.grid(rng, num_cu, d), R.grid(rng, num_ci, d)
    cu[0] = 1.0
    ci[3] = ci[7] = 2.0  # score 8 for user cluster 0, above every other cluster's (at most 4)
    u2cu, i2ci = labels(rng, nu, num_cu), labels(rng, I, num_ci)
    _, items, scores = check(cu, ci, u2cu, i2ci, K)
    both = np.nonzero((i2ci == 3) | (i2ci == 7))[0]
    assert both.shape[0] >= K and (np.diff(i2ci[both[:K]]) != 0).any()
    for b in np.nonzero(u2cu == 0)[0]:
        assert np.array_equal(items[b], both[:K]) and (scores[b] == 8.0).all()


@pytest.mark.parametrize("mask_value", [-1024.0, -1e9, 1e9])
def test_masks(mask_value):
    rng = np.random.RandomState(13)
    d, num_cu, num_ci, nu, I, K = 8, 3, 8, 6, 200, 10
    cu, ci = R.grid(rng, num_cu, d), R.grid(rng, num_ci, d)
    u2cu, i2ci = np.array([0, 1, 2, 0, 1, 2]), labels(rng, I, num_ci)
    best = int(np.argsort(-(cu[u2cu[2]].astype(np.float64) @ ci.T.astype(np.float64)), kind="stable")[0])
    keep = np.array([4, 77, 150])
    rows = {1: rng.permutation(I)[:100],                     # a row longer than 64
            2: np.nonzero(i2ci == best)[0],                  # every member of the user's best cluster
            3: np.setdiff1d(np.arange(I), keep),             # all but three items
            4: rng.permutation(I)[:5]}                       # users 0 and 5: empty rows
    mask = R.csr_of(np.concatenate([np.full(len(v), u) for u, v in rows.items()]),
                    np.concatenate(list(rows.values())), nu)
    rec, items, scores = check(cu, ci, u2cu, i2ci, K, None, mask, mask_value)
    assert rec.last_info["fallback_users"] == 0
    mv = np.float32(mask_value)
    if mask_value < 0:  # the three unmasked items, then the masked ones in ascending id
        assert set(items[3, :3]) == set(keep) and np.array_equal(items[3, 3:], rows[3][:K - 3])
        assert (scores[3, 3:] == mv).all() and (scores[3, :3] != mv).all()
        assert not np.isin(items[2], rows[2]).any()
    else:  # masked items come first
        assert np.array_equal(items[3], rows[3][:K]) and (scores[3] == mv).all()
        assert np.array_equal(items[1], np.sort(rows[1])[:K])
        assert np.array_equal(items[4, :5], np.sort(rows[4])) and (scores[4, 5:] != mv).all()


@pytest.mark.parametrize("num_ci", [257, 300])
def test_fallback_users_are_those_of_the_rule(num_ci):
    rng = np.random.RandomState(num_ci)
    d, num_cu, nu, I, K = 16, 9, 45, 1000, 20
    cu, ci = R.grid(rng, num_cu, d), R.grid(rng, num_ci, d)
    cu[0] = 0.0  # (a) every cluster ties for the users of cluster 0
    u2cu, i2ci = np.arange(nu) % num_cu, labels(rng, I, num_ci)
    order = np.argsort(-(cu[u2cu[1]].astype(np.float64) @ ci.T.astype(np.float64)), kind="stable")[:256]
    covered = np.nonzero(np.isin(i2ci, order))[0]  # (b) user 1: every item of its best 256 clusters
    few = random_mask(rng, nu, I)
    r = np.repeat(np.arange(nu), np.diff(few[0]))
    sel = r != 1
    mask = R.csr_of(np.concatenate([r[sel], np.full(len(covered), 1)]), np.concatenate([few[1][sel], covered]), nu)
    users = np.concatenate([np.arange(nu), [1, 0, 13]])
    m = R.take_rows(mask[0], mask[1], users)
    want = C.must_fall_back(cu, ci, u2cu, i2ci, K, users, m)
    assert want[users == 1].all() and want[u2cu[users] == 0].all()            # (a) and (b)
    assert not want[(users != 1) & (u2cu[users] != 0)].any()                  # (c) ordinary users
    rec, _, _ = check(cu, ci, u2cu, i2ci, K, users, mask)
    assert rec.last_info == {"fallback_users": int(want.sum()), "ranked_clusters": num_cu, "list_len": 256}


@pytest.fixture(scope="module")
def normal_case():
    g = torch.Generator().manual_seed(5)
    rng = np.random.RandomState(5)
    d, num_cu, num_ci, nu, I = 64, 50, 200, 500, 2000
    cu = (torch.randn(num_cu, d, generator=g) * 0.1).numpy()
    ci = (torch.randn(num_ci, d, generator=g) * 0.1).numpy()
    return cu, ci, labels(rng, nu, num_cu), labels(rng, I, num_ci), random_mask(rng, nu, I, 0.01)


def test_random_normal_inputs_match_the_expanded_tables(normal_case):
    cu, ci, u2cu, i2ci, mask = normal_case
    rec, _, _ = check(cu, ci, u2cu, i2ci, 20, None, mask, -1e9, exact=False)
    assert rec.last_info == {"fallback_users": 0, "ranked_clusters": 50, "list_len": 200}


def test_scipy_exclude_matrices(normal_case):
    """A canonical scipy CSR (sliced without a sort) and one with unsorted, repeated columns."""
    import scipy.sparse as sp
    cu, ci, u2cu, i2ci, mask = normal_case
    nu, I = len(u2cu), len(i2ci)
    canon = sp.csr_matrix((np.ones(len(mask[1]), np.float32), mask[1], mask[0]), shape=(nu, I))
    canon.sort_indices()
    canon.sum_duplicates()
    rng = np.random.RandomState(6)
    ptr, col = [0], []
    for u in range(nu):
        row = canon.indices[canon.indptr[u]:canon.indptr[u + 1]]
        col += rng.permutation(np.concatenate([row, row[:3]])).tolist()
        ptr.append(len(col))
    messy = sp.csr_matrix((np.ones(len(col), np.float32), np.array(col), np.array(ptr)), shape=(nu, I))
    assert canon.has_canonical_format and not messy.has_canonical_format
    for users in (None, np.array([7, 499, 7, 0, 123])):
        _, a_i, a_s = check(cu, ci, u2cu, i2ci, 40, users, mask, 1e9, exact=False)
        for ex in (canon, messy):
            _, b_i, b_s = check(cu, ci, u2cu, i2ci, 40, users, ex, 1e9, exact=False)
            assert np.array_equal(a_i, b_i) and np.array_equal(a_s.view(np.uint32), b_s.view(np.uint32))


def test_two_calls_give_the_same_bits_and_the_function_is_the_method(normal_case):
    import gdd
    cu, ci, u2cu, i2ci, mask = normal_case
    cu_t, ci_t = dev(cu), dev(ci)
    users = np.arange(0, 500, 3)
    rec = gdd.CondensedRecommender(cu_t, ci_t, u2cu, i2ci)
    a_i, a_s = rec.recommend(50, users=users, exclude=mask, return_scores=True)
    b_i, b_s = rec.recommend(50, users=users, exclude=mask, return_scores=True)
    c_i, c_s = gdd.recommend_condensed(cu_t, ci_t, u2cu, i2ci, 50, users=users, exclude=mask, return_scores=True)
    for i, s in ((b_i, b_s), (c_i, c_s)):
        assert torch.equal(a_i, i) and np.array_equal(bits(a_s), bits(s))
    only = gdd.recommend_condensed(cu_t, ci_t, u2cu, i2ci, 50, users=users, exclude=mask)
    assert torch.equal(only, a_i)


def test_invalid_rows():
    import gdd
    from gdd import _lib
    from gdd.rankeval import _score_topk
    rng = np.random.RandomState(14)
    d, num_cu, num_ci, nu, I, K = 8, 4, 300, 10, 600, 5
    cu, ci = R.grid(rng, num_cu, d), R.grid(rng, num_ci, d)
    u2cu, i2ci = labels(rng, nu, num_cu), labels(rng, I, num_ci)
    cu_t, ci_t = dev(cu), dev(ci)
    ptr = np.array([0, 2, 2, 4, 4, 4, 4, 4, 4, 4, 4], np.int32)
    col = np.array([3, 9, 7, I], np.int32)  # user 2: a column == I
    with pytest.raises(RuntimeError, match="out of range"):
        gdd.recommend_condensed(cu_t, ci_t, u2cu, i2ci, K, exclude=(ptr, col))
    with pytest.raises(RuntimeError, match="out of range"):
        gdd.recommend(cu_t[dev(u2cu)], ci_t[dev(i2ci)], K, exclude=(ptr, col))

    # the raw entry point: user 4's id is outside the table, user 2's mask row holds the column I
    lib = _lib.device_lib()
    rec = gdd.CondensedRecommender(cu_t, ci_t, u2cu, i2ci)
    g = rec._prepare()
    users = np.arange(nu, dtype=np.int32)
    users[4] = nu
    groups, row = np.unique(u2cu, return_inverse=True)
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    L = 256
    cl_item, cl_score = _score_topk(cu_t, ci_t, L, dev(groups.astype(np.int32)), None, 0.0, True, counters[:1])
    items = torch.zeros(nu, K, dtype=torch.int32, device="cuda")
    scores = torch.zeros(nu, K, dtype=torch.float32, device="cuda")
    inc = torch.full((nu,), 7, dtype=torch.int32, device="cuda")
    row_t, users_t, mp, mc = dev(row.astype(np.int32)), dev(users), dev(ptr), dev(col)
    _lib.check(lib.gdd_cluster_expand_topk(
        nu, I, num_ci, L, K, users_t.data_ptr(), nu, row_t.data_ptr(), len(groups), cl_item.data_ptr(),
        cl_score.data_ptr(), g["mem_ptr"].data_ptr(), g["mem_item"].data_ptr(), mp.data_ptr(), mc.data_ptr(),
        -1024.0, items.data_ptr(), scores.data_ptr(), inc.data_ptr(), counters[1:].data_ptr(),
        counters[:1].data_ptr(), _lib.stream_ptr(torch.device("cuda"))))
    assert counters.cpu().tolist() == [2, 0] and not inc.cpu().numpy().any()
    items, scores = items.cpu().numpy(), scores.cpu().numpy()
    for b in (2, 4):
        assert (items[b] == -1).all() and np.isnan(scores[b]).all()
    good = np.setdiff1d(np.arange(nu), [2, 4])
    gptr, gcol = R.take_rows(ptr, col, good)
    assert not C.must_fall_back(cu, ci, u2cu, i2ci, K, good, (gptr, gcol)).any()  # L < num_ci, yet complete
    ref_i, ref_s = C.expanded_reference(cu, ci, u2cu, i2ci, K, good, (gptr, gcol))
    assert np.array_equal(items[good], ref_i) and np.array_equal(scores[good], ref_s.astype(np.float32))


def test_ranking_evaluator_condensed_equals_the_expanded_call():
    from gdd.rankeval import RankingEvaluator
    c = R.fixture_inputs()
    rng = np.random.RandomState(21)
    num_cu, num_ci, d = 30, 50, 16
    cu, ci = dev(R.grid(rng, num_cu, d)), dev(R.grid(rng, num_ci, d))
    u2cu, i2ci = labels(rng, c["n"], num_cu), labels(rng, c["m"], num_ci)
    train = (np.ones(len(c["train_u"]), np.float32), (c["train_u"], c["train_i"]))
    import scipy.sparse as sp
    ev = RankingEvaluator(sp.coo_matrix(train, shape=(c["n"], c["m"])).tocsr(), c["valid_u"], c["valid_i"],
                          R.FIXTURE_TOPKS, "cuda")
    want = ev(cu[dev(u2cu)], ci[dev(i2ci)])
    got = ev.condensed(cu, ci, u2cu, i2ci)
    assert sorted(got) == sorted(want) and got["users"] == want["users"] > 0
    for key in ("precision", "recall", "ndcg"):
        assert np.array_equal(got[key], want[key])
    assert want["ndcg"].max() > 0


def test_round_trip_through_the_saved_artefact(tmp_path, capsys):
    import gdd
    from gdd import distill_recsys as D
    from rankformer_ref import planted_blocks
    tr_u, tr_i, te_u, te_i = planted_blocks()
    os.makedirs(tmp_path / "planted")
    for name, (a, b) in (("train", (tr_u, tr_i)), ("valid", (te_u, te_i)), ("test", (te_u, te_i))):
        np.savetxt(tmp_path / "planted" / f"{name}.txt", np.stack([a, b], 1), fmt="%d")
    base = ["--data_dir", str(tmp_path), "--dataset", "planted", "--refine_epochs", "3", "--svd_dim", "8",
            "--svd_backend", "device", "--reduction_rate", "0.25", "--batch_size", "256", "--device", "cuda",
            "--report_ranking", "--report_topks", "[5, 20]"]
    D.run(D.parse_args(base), out_root=str(tmp_path / "plain"))
    plain = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[rank] condensed")]
    args = D.parse_args(base + ["--report_from_clusters"])
    model = D.run(args, out_root=str(tmp_path / "out"))
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("[rank] condensed")]
    assert len(lines) == 2 and lines == plain

    out_dir = str(tmp_path / "out" / "distilled_recsys" / "planted")
    rec = gdd.CondensedRecommender.load(out_dir, num_layers=args.lgn_layers)
    assert (rec.num_users, rec.num_items, rec.num_cu, rec.num_ci) == (120, 80, 30, 20)
    with torch.no_grad():
        cu_z, ci_z = model.propagate()
    assert torch.allclose(rec.cu_z, cu_z, rtol=1e-5, atol=1e-6)
    assert torch.allclose(rec.ci_z, ci_z, rtol=1e-5, atol=1e-6)
    train = R.csr_of(tr_u, tr_i, 120)
    items, scores = rec.recommend(20, exclude=train, mask_value=-1e9, return_scores=True)
    u2cu, i2ci = dev(np.load(os.path.join(out_dir, "u2cu.npy"))), dev(np.load(os.path.join(out_dir, "i2ci.npy")))
    want_i, want_s = gdd.recommend(rec.cu_z[u2cu], rec.ci_z[i2ci], 20, exclude=train, mask_value=-1e9,
                                   return_scores=True)
    assert torch.equal(items, want_i) and np.array_equal(bits(scores), bits(want_s))
    again = gdd.CondensedRecommender.from_model(model, np.load(os.path.join(out_dir, "u2cu.npy")),
                                                np.load(os.path.join(out_dir, "i2ci.npy")))
    assert torch.allclose(again.cu_z, cu_z, rtol=1e-5, atol=1e-6)
    assert torch.allclose(again.ci_z, ci_z, rtol=1e-5, atol=1e-6)
