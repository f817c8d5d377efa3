"""gdd.condrank without a device: argument validation, the membership CSR, the numpy model of the
completion rule (tests/condrank_ref.py) and the command-line parsers."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import condrank_ref as C  # noqa: E402


def tables(num_cu=4, num_ci=5, d=3):
    return torch.zeros(num_cu, d), torch.zeros(num_ci, d)


def test_argument_errors_raise_before_the_device():
    import gdd
    cu, ci = tables()
    u2cu, i2ci = np.array([0, 3, 1, 1]), np.array([0, 4, 2, 2, 1, 0])
    for bad_u in ([0, 4, 1, 1], [0, -1, 1, 1]):
        with pytest.raises(ValueError, match="u2cu"):
            gdd.recommend_condensed(cu, ci, bad_u, i2ci, 2)
    for bad_i in ([0, 5, 2, 2, 1, 0], [-1, 4, 2, 2, 1, 0]):
        with pytest.raises(ValueError, match="i2ci"):
            gdd.recommend_condensed(cu, ci, u2cu, bad_i, 2)
    with pytest.raises(ValueError, match="width"):
        gdd.recommend_condensed(cu, torch.zeros(5, 4), u2cu, i2ci, 2)
    for k in (0, 7, 257):
        with pytest.raises(ValueError, match="k = "):
            gdd.recommend_condensed(cu, ci, u2cu, i2ci, k)
    with pytest.raises(ValueError, match="k = "):
        gdd.recommend_condensed(cu, ci, u2cu, np.zeros(300, np.int64), 257)
    with pytest.raises(ValueError, match="users"):
        gdd.CondensedRecommender(cu, ci, u2cu, i2ci).recommend(2, users=[4])


def test_membership_csr_matches_a_numpy_grouping():
    from gdd.condrank import membership_csr
    rng = np.random.RandomState(3)
    num_ci = 40
    lab = rng.choice(np.setdiff1d(np.arange(num_ci), [0, 7, 8, 39]), 500)  # four empty clusters
    ptr, item = membership_csr(lab, num_ci)
    assert ptr.dtype == np.int32 and item.dtype == np.int32 and ptr.shape == (num_ci + 1,)
    assert ptr[0] == 0 and ptr[-1] == 500
    for c, want in enumerate(C.membership(lab, num_ci)):
        assert np.array_equal(item[ptr[c]:ptr[c + 1]], want)
    for c in (0, 7, 8, 39):
        assert ptr[c] == ptr[c + 1]
    with pytest.raises(ValueError):
        membership_csr([0, 40], num_ci)


def test_repeated_mask_columns_are_entered_once():
    from gdd.condrank import _distinct_columns
    ptr, col = np.array([0, 3, 3, 6], np.int32), np.array([1, 1, 2, 2, 2, 5], np.int32)
    p, c = _distinct_columns(ptr, col)
    assert p.tolist() == [0, 2, 2, 4] and c.tolist() == [1, 2, 2, 5]


def test_mask_rows_of_scipy_matrices_and_csr_pairs():
    """Canonical scipy CSR is sliced without a sort, anything else is sorted and loses its repeats:
    either way the rows of gdd.rankeval._rows_of, each column once."""
    import scipy.sparse as sp
    from gdd.condrank import _distinct_columns, mask_rows
    from gdd.rankeval import _rows_of
    rng = np.random.RandomState(4)
    nu, I = 12, 30
    r, c = np.nonzero(rng.random_sample((nu + 2, I)) < 0.2)  # two rows more than users
    canon = sp.coo_matrix((np.ones(len(r), np.float32), (r, c)), shape=(nu + 2, I)).tocsr()
    assert canon.has_canonical_format
    # the same entries unsorted within rows, some stored twice
    ptr, col = [0], []
    for u in range(nu + 2):
        row = canon.indices[canon.indptr[u]:canon.indptr[u + 1]]
        row = rng.permutation(np.concatenate([row, row[:2]]))
        col += row.tolist()
        ptr.append(len(col))
    messy = sp.csr_matrix((np.ones(len(col), np.float32), np.array(col), np.array(ptr)), shape=(nu + 2, I))
    assert not messy.has_canonical_format
    kept = messy.indices.copy()
    for ids in (None, np.array([3, 3, 0, 11, 7])):
        sel = np.arange(nu) if ids is None else ids
        want = _distinct_columns(*_rows_of(canon, sel, I))
        for ex in (canon, messy, (np.array(ptr), np.array(col))):
            got = mask_rows(ex, ids, nu, I)
            assert got[0].dtype == np.int32 and got[1].dtype == np.int32
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(messy.indices, kept)  # the caller's matrix is left as it was
    with pytest.raises(ValueError, match="no row"):
        mask_rows(canon[:5], None, nu, I)
    with pytest.raises(ValueError, match="no row"):
        mask_rows(canon, np.array([nu + 2]), nu, I)


def test_completion_rule_model_on_hand_written_cases():
    # every cluster was ranked: nothing is unseen
    assert not C.rule_incomplete([1.0, 1.0, 1.0], [0, 0, 0], 3, 3)
    # two members beat s_1 = 2, four beat s_2 = 1: complete at j = 1
    assert not C.rule_incomplete([3.0, 2.0, 1.0], [2, 2, 2], 3, 5)
    # all tie: no member scores strictly above the next cluster, nor above an unseen one
    assert C.rule_incomplete([1.0, 1.0, 1.0], [5, 5, 5], 3, 4)
    # the last cluster only ties s_L := s_{L-1}: one member above it
    assert C.rule_incomplete([3.0, 2.0], [1, 5], 3, 3)
    # the per-cluster quota: a cluster of 50 counts K members
    assert not C.rule_incomplete([3.0, 2.0], [50, 0], 20, 3)
    assert C.rule_incomplete([3.0, 2.0], [19, 50], 20, 3)


def test_model_of_the_rule_from_tables():
    cu = np.array([[1.0], [0.0]], np.float32)
    ci = np.arange(300, 0, -1, dtype=np.float32)[:, None]  # cluster c scores 300 - c for user cluster 0
    i2ci = np.arange(300)
    got = C.must_fall_back(cu, ci, [0, 1, 0], i2ci, 5, users=[0, 1, 2],
                           mask=C.csr_of(np.full(256, 2), np.arange(256), 3))
    # user 0: distinct scores, one member each; user 1: all tie; user 2: its best 256 masked
    assert got.tolist() == [False, True, True]


def test_parsers():
    from gdd import distill_recsys, recommend_distilled
    a = distill_recsys.parse_args([])
    assert a.report_from_clusters is False and a.report_ranking is False
    assert distill_recsys.parse_args(["--report_ranking", "--report_from_clusters"]).report_from_clusters is True
    r = recommend_distilled.parse_args(["--artifacts", "dir", "--out", "lists.npy"])
    assert (r.artifacts, r.k, r.users, r.exclude, r.out) == ("dir", 20, None, None, "lists.npy")
    r = recommend_distilled.parse_args(["--artifacts", "d", "--k", "5", "--users", "u.npy", "--exclude", "train.txt",
                                        "--out", "o.npy"])
    assert (r.k, r.users, r.exclude) == (5, "u.npy", "train.txt")
    with pytest.raises(SystemExit):
        recommend_distilled.parse_args(["--k", "5"])


def test_public_names():
    import gdd
    assert gdd.recommend_condensed is gdd.condrank.recommend_condensed
    assert gdd.CondensedRecommender is gdd.condrank.CondensedRecommender
    assert hasattr(gdd.RankingEvaluator, "condensed")
