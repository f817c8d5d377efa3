"""gdd.rankpos without a device: argument errors (raised before the device is touched, so they are
raised here, where there may be none), the host metrics against the plain definition, and the numpy
model of the cluster formula against the expanded definition.

Bounds. ``metrics_from_positions`` performs the fp64 operations of tests/rankeval_ref.py ``metrics``
per user in the same order (hits / k, hits / min(n, k), DCG and IDCG added one term at a time in rank
order), so the per-user values must be bit-equal. MRR and the mean rank are means of B per-user fp64
values: numpy's pairwise sum against a plain one, rel 1e-12. The cluster formula is integer.
"""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rankeval_ref as R  # noqa: E402
import rankpos_ref as P  # noqa: E402

from gdd import rankpos  # noqa: E402
from gdd.condrank import CondensedRecommender  # noqa: E402


def tables(nu=6, ni=9, d=4, seed=0):
    rng = np.random.RandomState(seed)
    return torch.from_numpy(R.grid(rng, nu, d)), torch.from_numpy(R.grid(rng, ni, d))


@pytest.mark.parametrize("targets,match", [
    (np.zeros(6, np.int64), r"expected \[6, T\]"),                     # 1-D
    (np.zeros((5, 2), np.int64), r"expected \[6, T\]"),                # one row short
    (np.zeros((6, 2, 1), np.int64), r"expected \[6, T\]"),
    (np.zeros((6, 2), np.float32), "integers"),
    (np.full((6, 2), 9, np.int64), "outside"),                         # id == I
    (np.full((6, 2), -1, np.int64), "outside"),
    ((np.arange(6) * 2, np.zeros(10, np.int64)), "ptr of 6 entries"),  # ptr needs B + 1
    ((np.array([0, 2, 1, 3, 3, 3, 3]), np.zeros(3, np.int64)), "not decrease"),
    ((np.array([0, 1, 1, 1, 1, 1, 2]), np.zeros(3, np.int64)), "end at len"),
    ((np.array([0, 1, 1, 1, 1, 1, 2]), np.array([0, 9])), "outside"),
    ((np.arange(7), np.zeros(6, np.int64), np.zeros(6, np.int64)), "2-D integer array"),
])
def test_bad_targets_raise_before_the_device(targets, match):
    U, V = tables()
    with pytest.raises(ValueError, match=match):
        rankpos.rank_positions(U, V, targets)
    rng = np.random.RandomState(1)
    rec = CondensedRecommender(U[:3], V[:4], rng.randint(0, 3, 6), rng.randint(0, 4, 9))
    with pytest.raises(ValueError, match=match):
        rec.positions(targets)


def test_bad_users_tables_and_exclude_raise_before_the_device():
    U, V = tables()
    t = np.zeros((2, 3), np.int64)
    with pytest.raises(ValueError, match="users holds an id"):
        rankpos.rank_positions(U, V, t, users=[0, 6])
    with pytest.raises(ValueError, match="users holds an id"):
        rankpos.rank_positions(U, V, t, users=[-1, 2])
    with pytest.raises(ValueError, match="differ in width"):
        rankpos.rank_positions(U, V[:, :3], np.zeros((6, 1), np.int64))
    with pytest.raises(ValueError, match="exclude has no row"):
        rankpos.rank_positions(U, V, np.zeros((6, 1), np.int64), exclude=sp.csr_matrix((3, 9)))
    with pytest.raises(ValueError, match="users holds an id"):
        rankpos.rank_positions_condensed(U[:3], V[:4], np.zeros(6, np.int64), np.zeros(9, np.int64), t, users=[0, 6])
    with pytest.raises(ValueError, match="i2ci holds a cluster id"):
        rankpos.rank_positions_condensed(U[:3], V[:4], np.zeros(6, np.int64), np.full(9, 4), t)


@pytest.mark.parametrize("topks,match", [((), "at least one"), ((0, 5), "strictly ascending"),
                                         ((5, 5), "strictly ascending"), ((20, 5), "strictly ascending"),
                                         ((5, 10), "exceeds the number of items"), (5, "sequence")])
def test_bad_cutoffs(topks, match):
    with pytest.raises(ValueError, match=match):
        rankpos.check_cutoffs(topks, 9)
    train = sp.csr_matrix((6, 9))
    with pytest.raises(ValueError, match=match):
        rankpos.PositionEvaluator(train, [0, 1], [2, 3], topks)


def test_cutoffs_have_no_limit_but_the_items():
    many = tuple(range(1, 301))
    assert rankpos.check_cutoffs(many, 300) == many  # more than 8 cut-offs, past 256
    assert rankpos.parse_cutoffs("[20, 500]", 500) == (20, 500) and rankpos.parse_cutoffs("7") == (7,)
    with pytest.raises(ValueError, match="list of integers"):
        rankpos.parse_cutoffs("[1.5]")
    ev = rankpos.PositionEvaluator(sp.csr_matrix((6, 400)), [0, 1], [2, 3], (1, 300, 400))
    assert ev.topks == (1, 300, 400) and list(ev.users) == [0, 1]
    with pytest.raises(ValueError, match="evaluator of 6 x 400"):
        ev(*tables())


def test_metrics_argument_errors():
    with pytest.raises(ValueError, match="does not describe"):
        rankpos.metrics_from_positions(np.zeros(3), [0, 2], None, (1,))
    with pytest.raises(ValueError, match="deg does not match"):
        rankpos.metrics_from_positions(np.zeros(3), [0, 3], [1, 1], (1,))
    with pytest.raises(ValueError, match="negative"):
        rankpos.metrics_from_positions(np.array([0, -1, 2]), [0, 3], None, (1,))
    with pytest.raises(ValueError, match="strictly ascending"):
        rankpos.metrics_from_positions(np.zeros(3), [0, 3], None, (2, 1))
    with pytest.raises(ValueError, match="lists hold 4"):
        rankpos.fidelity(np.zeros((2, 4), int), np.zeros((2, 4), int), (5,))
    with pytest.raises(ValueError, match="shape"):
        rankpos.fidelity(np.zeros((2, 4), int), np.zeros((2, 3), int), (2,))


@pytest.fixture(scope="module")
def full_lists():
    """The fixture's evaluated users with full-length lists (K = I = 500) and the positions of their
    distinct valid items in those lists."""
    c = R.fixture_inputs()
    n, m = int(c["n"]), int(c["m"])
    users = np.unique(c["valid_u"])
    tr = R.take_rows(*R.csr_of(c["train_u"], c["train_i"], n), users)
    te = R.take_rows(*R.csr_of(c["valid_u"], c["valid_i"], n), users)
    deg = np.bincount(c["valid_u"], minlength=n)[users]
    lists, _ = R.ranked(R.scores64(c["U"], c["V"], users, tr), m)
    inverse = np.empty_like(lists)
    np.put_along_axis(inverse, lists, np.arange(m, dtype=lists.dtype)[None, :].repeat(len(users), 0), 1)
    pos = np.concatenate([inverse[b, te[1][te[0][b]:te[0][b + 1]]] for b in range(len(users))])
    return dict(lists=lists, te=te, deg=deg, pos=pos, m=m)


def test_metrics_from_positions_are_the_definition_bit_for_bit(full_lists):
    f = full_lists
    topks = (1, 5, 20, 50, 300, 500)
    per, sums, count = R.metrics(f["lists"], f["te"][0], f["te"][1], f["deg"], topks)
    got = rankpos.metrics_from_positions(f["pos"], f["te"][0], f["deg"], topks)
    assert got["users"] == count == len(f["deg"]) and got["per_user"].shape == per.shape
    assert np.array_equal(got["per_user"], per)
    assert per[:, 2, -1].min() > 0 and (per[:, 1, -1] <= 1).all()  # at k = I every unmasked hit is in
    for j, key in enumerate(("precision", "recall", "ndcg")):
        assert np.allclose(got[key], sums[j] / count, rtol=2 * count * 2.0 ** -53, atol=0)
    # deg None: the row lengths; a user without relevant items counts for nothing
    lens = np.diff(f["te"][0])
    per_n, _, _ = R.metrics(f["lists"], f["te"][0], f["te"][1], None, topks)
    assert np.array_equal(rankpos.metrics_from_positions(f["pos"], f["te"][0], None, topks)["per_user"], per_n)
    deg0 = f["deg"].copy()
    deg0[::3] = 0
    got0 = rankpos.metrics_from_positions(f["pos"], f["te"][0], deg0, topks)
    per0, _, count0 = R.metrics(f["lists"], f["te"][0], f["te"][1], deg0, topks)
    assert got0["users"] == count0 < count and np.array_equal(got0["per_user"], per0)
    assert lens.min() > 0


def test_block_edges_of_the_padded_rows(full_lists, monkeypatch):
    """The users are processed in blocks of padded rows: one user per block gives the same values."""
    f = full_lists
    want = rankpos.metrics_from_positions(f["pos"], f["te"][0], f["deg"], (1, 20, 500))
    monkeypatch.setattr(rankpos, "_BLOCK_ELEMS", 1)
    got = rankpos.metrics_from_positions(f["pos"], f["te"][0], f["deg"], (1, 20, 500))
    for key in ("per_user", "rr", "rank"):
        assert np.array_equal(got[key], want[key])


def test_mrr_and_mean_rank_against_numpy(full_lists):
    f = full_lists
    got = rankpos.metrics_from_positions(f["pos"], f["te"][0], f["deg"], (20,))
    mrr, mean_rank, count = P.direct_metrics(f["pos"], f["te"][0], f["deg"])
    assert got["users"] == count
    assert got["mrr"] == pytest.approx(mrr, rel=1e-12) and got["mean_rank"] == pytest.approx(mean_rank, rel=1e-12)
    assert 0 < got["mrr"] <= 1 and 1 <= got["mean_rank"] <= f["m"]
    # by hand: two users, positions {3, 0} and {9}; an empty third user is not counted
    m = rankpos.metrics_from_positions([3, 0, 9], [0, 2, 3, 3], None, (1, 4))
    assert m["users"] == 2 and m["mrr"] == (1.0 + 0.1) / 2 and m["mean_rank"] == (2.5 + 10.0) / 2
    assert list(m["rr"]) == [1.0, 0.1, 0.0] and list(m["precision"]) == [0.5, 0.25]
    assert list(m["recall"]) == [0.5, 0.5]


def test_fidelity_against_numpy():
    rng = np.random.RandomState(4)
    B, K = 13, 20
    lists = np.stack([rng.permutation(50)[:K] for _ in range(B)])
    pos = rng.randint(0, 50, (B, K))
    f = rankpos.fidelity(lists, pos, (1, 5, 20))
    for j, k in enumerate((1, 5, 20)):
        assert f["overlap"][j] == pytest.approx(np.mean([(pos[b, :k] < k).mean() for b in range(B)]), rel=1e-12)
        assert f["mean_position"][j] == pytest.approx(np.mean([pos[b, :k].mean() for b in range(B)]), rel=1e-12)
    same = rankpos.fidelity(lists, np.arange(K)[None, :].repeat(B, 0), (1, 5, 20))
    assert list(same["overlap"]) == [1.0, 1.0, 1.0] and list(same["mean_position"]) == [0.0, 2.0, 9.5]
    assert f["users"] == B


MASK_VALUES = (-1024.0, 0.5, 0.0, -0.0, 1e9, -0.25)


@pytest.mark.parametrize("seed", range(12))
def test_cluster_formula_is_the_expanded_definition(seed):
    """25 random grid cases per seed (300 in all): duplicated cluster rows, empty clusters, masked and
    repeated targets, mask values that tie scores (grid scores are multiples of 1/4; +0 and -0 differ
    in key order)."""
    rng = np.random.RandomState(100 + seed)
    for _ in range(25):
        nu, ni = rng.randint(1, 8), rng.randint(1, 40)
        num_cu, num_ci, d = rng.randint(1, 5), rng.randint(1, 9), rng.randint(1, 4)
        cu, ci = R.grid(rng, num_cu, d), R.grid(rng, num_ci + 1, d)
        if num_ci > 1:
            ci[rng.randint(num_ci)] = ci[rng.randint(num_ci)]  # two clusters with one row
        u2cu = rng.randint(0, num_cu, nu)
        i2ci = rng.randint(0, num_ci, ni)  # cluster num_ci stays empty, others may
        mv = MASK_VALUES[rng.randint(len(MASK_VALUES))]
        M = rng.random_sample((nu, ni)) < 0.3
        mask_all = R.csr_of(*np.nonzero(M), nu)
        users = rng.randint(0, nu, rng.randint(1, 6))
        mask = R.take_rows(mask_all[0], mask_all[1], users)
        lens = rng.randint(0, 7, users.shape[0])
        tg_ptr = np.concatenate([[0], np.cumsum(lens)])
        tg_col = rng.randint(0, ni, tg_ptr[-1])
        for b in range(users.shape[0]):  # a masked target where the row has one
            row = mask[1][mask[0][b]:mask[0][b + 1]]
            if lens[b] and row.size:
                tg_col[tg_ptr[b]] = row[rng.randint(row.size)]
        want = P.positions(P.masked_scores32(cu[u2cu], ci[i2ci], users, mask, mv), tg_ptr, tg_col)
        got = P.cluster_positions(cu, ci, u2cu, i2ci, tg_ptr, tg_col, users, mask, mv)
        assert np.array_equal(got, want)


def test_reference_positions_are_the_index_in_the_full_list():
    """The definition of the reference itself: positions invert the stable sort of tests/rankeval_ref."""
    rng = np.random.RandomState(8)
    U, V = R.grid(rng, 5, 3), R.grid(rng, 70, 3)
    mask = R.csr_of(*np.nonzero(rng.random_sample((5, 70)) < 0.2), 5)
    lists, _ = R.ranked(R.scores64(U, V, None, mask, 0.5), 70)
    ptr = np.arange(6) * 70
    pos = P.positions(P.masked_scores32(U, V, None, mask, 0.5), ptr, lists.ravel())
    assert np.array_equal(pos.reshape(5, 70), np.arange(70)[None, :].repeat(5, 0))
