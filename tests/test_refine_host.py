"""Host side of the device refinement loop (gdd.recsys.DeviceRefiner): the triplet grouping
``gdd_bpr_group`` against numpy's stable argsort, and the driver's ``--refine_backend`` flag. No GPU."""
import numpy as np
import pytest

from gdd import distill_recsys as D
from gdd import recsys


def _check_record(u, pos, neg, num_cu, num_ci):
    u, pos, neg = (np.asarray(a, np.int64) for a in (u, pos, neg))
    b = u.shape[0]
    rec = recsys.group_bpr_triplets(u, pos, neg, num_cu, num_ci)
    assert rec.dtype == np.int32 and rec.shape == (6 * b + num_cu + num_ci + 2,)
    p = recsys.split_batch_record(rec, b, num_cu, num_ci)
    assert np.array_equal(p["u"], u) and np.array_equal(p["pos"], pos) and np.array_equal(p["neg"], neg)
    # users: a stable sort of the triplets by user, rows as a prefix sum of the counts
    assert np.array_equal(p["uidx"], np.argsort(u, kind="stable"))
    assert np.array_equal(p["uptr"], np.concatenate([[0], np.cumsum(np.bincount(u, minlength=num_cu))]))
    # items: entry 2t is triplet t's positive, 2t+1 its negative; a stable sort of the entries by item
    items = np.stack([pos, neg], 1).ravel()
    assert np.array_equal(p["ient"], np.argsort(items, kind="stable"))
    assert np.array_equal(p["iptr"], np.concatenate([[0], np.cumsum(np.bincount(items, minlength=num_ci))]))
    return p


def test_group_repeated_users_and_shared_items():
    # user 2 three times; item 4 is triplet 0's positive and triplet 3's negative; users 0, 3 and
    # items 1, 5 are rows nobody drew
    p = _check_record([2, 1, 2, 4, 2], [4, 0, 3, 2, 0], [2, 3, 0, 4, 3], 5, 6)
    assert list(p["uptr"]) == [0, 0, 1, 4, 4, 5] and list(p["uidx"]) == [1, 0, 2, 4, 3]
    assert list(p["ient"][p["iptr"][4]:p["iptr"][5]]) == [0, 7]


def test_group_batch_of_one():
    p = _check_record([0], [0], [0], 1, 1)  # the only item is positive and negative
    assert list(p["ient"]) == [0, 1]
    _check_record([3], [1], [0], 4, 2)


@pytest.mark.parametrize("num_cu,num_ci,b", [(7, 5, 300), (1773, 1004, 4096), (300, 2, 64)])
def test_group_random(num_cu, num_ci, b):
    rng = np.random.default_rng(b)
    _check_record(rng.integers(0, num_cu, b), rng.integers(0, num_ci, b), rng.integers(0, num_ci, b), num_cu, num_ci)


def test_group_rejects_bad_ids_and_shapes():
    with pytest.raises(IndexError):
        recsys.group_bpr_triplets([0, 3], [0, 0], [1, 1], 3, 2)  # user == num_cu
    with pytest.raises(IndexError):
        recsys.group_bpr_triplets([0, 1], [0, 2], [1, 1], 3, 2)  # item == num_ci
    with pytest.raises(IndexError):
        recsys.group_bpr_triplets([0, 1], [0, 0], [1, -1], 3, 2)
    with pytest.raises(ValueError):
        recsys.group_bpr_triplets([0, 1], [0], [1, 1], 3, 2)
    with pytest.raises(ValueError):
        recsys.group_bpr_triplets([0, 1], [0, 0], [1, 1], 3, 2, out=np.empty(5, np.int32))


def test_parse_args_refine_backend():
    assert D.parse_args([]).refine_backend == "torch"
    assert D.parse_args(["--refine_backend", "device"]).refine_backend == "device"
    with pytest.raises(SystemExit):
        D.parse_args(["--refine_backend", "graph"])
