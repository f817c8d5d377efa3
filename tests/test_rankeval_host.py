"""CPU checks of gdd.rankeval (no GPU): the plain numpy definition (tests/rankeval_ref.py) against
the reference's recorded metrics (tests/golden/golden_rankeval.npz, tools/make_golden_rankeval.py),
the argument errors, which are raised before the device is touched, and the --topks parsing.

Bound against the reference: its ``test`` (model.py:27-53) forms every per-user term in fp32 and
sums the users in fp32, ours is fp64 throughout. Each of the at most 300 terms lies in [0, 1], so
the fp32 sum is within (n - 1) 2^-24 = 1.8e-5 of exact relative to the sum itself, plus a few fp32
ulps from the log2 terms and the final division: rel 5e-5. The count is an integer and exact."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rankeval_ref as R  # noqa: E402

REL = 5e-5


@pytest.fixture(scope="module")
def fx():
    return R.load_fixture()


def test_fixture_holds_what_it_is_for(fx):
    assert os.path.getsize(R.GOLDEN) < 2 ** 20
    assert int(fx["self_generated"]) == 0  # recorded from the reference's model.test
    n, m = int(fx["n"]), int(fx["m"])
    assert (n, m, fx["U"].shape, fx["V"].shape) == (300, 500, (300, 16), (500, 16))
    assert tuple(fx["topks"]) == R.FIXTURE_TOPKS
    for t in (fx["U"], fx["V"]):
        assert t.dtype == np.float32 and set(np.unique(t * 2)) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    for u, i in ((fx["train_u"], fx["train_i"]), (fx["valid_u"], fx["valid_i"])):
        key = u * m + i
        assert np.unique(key).shape[0] < key.shape[0]  # repeated lines
    lines = np.bincount(fx["valid_u"], minlength=n)
    distinct = np.diff(R.csr_of(fx["valid_u"], fx["valid_i"], n)[0])
    assert (lines == 0).sum() >= 10 and (distinct > 50).sum() >= 5 and (lines > distinct).any()
    assert int(fx["ref_count"]) == int((lines > 0).sum())
    # the same generator the tool used
    c = R.fixture_inputs()
    for k in ("U", "V", "train_u", "train_i", "valid_u", "valid_i"):
        assert np.array_equal(c[k], fx[k])


def test_plain_definition_equals_the_reference(fx):
    r = R.fixture_reference_run(fx, tuple(int(k) for k in fx["topks"]))
    assert r["count"] == int(fx["ref_count"])
    for j, name in enumerate(("ref_precision", "ref_recall", "ref_ndcg")):
        rel = np.abs(r["means"][j] - fx[name]) / np.abs(fx[name])
        print(f"{name}: rel {rel}")
        assert (fx[name] > 0).all() and (rel <= REL).all()


def test_plain_metrics_on_a_hand_case():
    lists = np.array([[7, 3, 9, 1], [0, 1, 2, 3]], np.int32)
    te_ptr, te_col = np.array([0, 2, 2], np.int32), np.array([1, 3], np.int32)
    per, sums, count = R.metrics(lists, te_ptr, te_col, np.array([3, 0]), (1, 4))
    w = 1.0 / np.log2(np.arange(4) + 2.0)
    assert count == 1 and np.array_equal(per[1], np.zeros((3, 2)))
    assert np.allclose(per[0, :, 0], (0.0, 0.0, 0.0), atol=0)
    assert np.allclose(per[0, :, 1], (2 / 4, 2 / 3, (w[1] + w[3]) / (w[0] + w[1] + w[2])), rtol=1e-15)
    assert np.array_equal(sums, per[0])


def test_argument_errors_come_before_the_device():
    from gdd import rankeval
    U, V = torch.zeros(5, 4), torch.zeros(7, 4)  # CPU tensors: the checks never reach the device
    for k in (0, -1, 257, 8):
        with pytest.raises(ValueError):
            rankeval.recommend(U, V, k)
    with pytest.raises(ValueError, match="width"):
        rankeval.recommend(U, torch.zeros(7, 3), 2)
    for users in ([0, 5], [-1], torch.tensor([2, 7])):
        with pytest.raises(ValueError, match="users"):
            rankeval.recommend(U, V, 2, users=users)
    with pytest.raises(ValueError):
        rankeval.recommend(torch.zeros(5, 257), torch.zeros(7, 257), 2)
    import scipy.sparse as sp
    train = sp.csr_matrix((5, 7), dtype=np.float32)
    for topks in ((5, 5), (5, 3), (0, 2), (), (2, 8), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            rankeval.RankingEvaluator(train, [0], [1], topks=topks)
    with pytest.raises(ValueError):
        rankeval.RankingEvaluator(train, [0, 1], [1], topks=(2,))
    with pytest.raises(ValueError):
        rankeval.RankingEvaluator(train, [5], [1], topks=(2,))
    ev = rankeval.RankingEvaluator(train, [0, 0, 3], [1, 1, 2], topks=(1, 5))
    assert ev.topks == (1, 5) and ev.k == 5 and list(ev.users) == [0, 3]
    with pytest.raises(ValueError):
        ev(torch.zeros(5, 4), torch.zeros(7, 3))
    with pytest.raises(ValueError):
        ev(torch.zeros(4, 4), torch.zeros(7, 4))
    with pytest.raises(ValueError):
        rankeval.rank_metrics(torch.zeros(2, 4, dtype=torch.int32), torch.zeros(3, dtype=torch.int32),
                              torch.zeros(0, dtype=torch.int32), None, (2, 5))


def test_evaluator_host_preparation_counts_repeated_lines():
    import scipy.sparse as sp
    from gdd import rankeval
    train = sp.csr_matrix((np.ones(3, np.float32), ([0, 0, 2], [4, 1, 6])), shape=(4, 7))
    eu, ei = [2, 0, 2, 2, 0], [3, 5, 3, 1, 2]
    for repeats, deg in ((True, [2, 3]), (False, [2, 2])):
        ev = rankeval.RankingEvaluator(train, eu, ei, topks=(2,), count_repeats=repeats)
        (mp, mc), te_ptr, te_col, d = ev._host
        assert list(ev.users) == [0, 2] and list(d) == deg
        assert list(mp) == [0, 2, 3] and list(mc) == [1, 4, 6]  # columns ascending
        assert list(te_ptr) == [0, 2, 4] and list(te_col) == [2, 5, 1, 3]
    ev = rankeval.RankingEvaluator(train, eu, ei, topks=(2,), max_users=1)
    assert list(ev.users) == [0] and list(ev._host[3]) == [2]


def test_topks_parsing():
    from gdd import rankeval, train_teacher
    assert rankeval.parse_topks("[20]") == (20,)
    assert rankeval.parse_topks("[5, 20, 50]") == (5, 20, 50)
    assert rankeval.parse_topks("(1, 2)") == (1, 2)
    assert rankeval.parse_topks("20") == (20,)
    for bad in ("[20, 5]", "[0]", "[1.5]", "[True]", "'x'", "[300]", "[]"):
        with pytest.raises(ValueError):
            rankeval.parse_topks(bad)
    with pytest.raises((ValueError, SyntaxError)):
        rankeval.parse_topks("__import__('os').getcwd()")  # literal_eval, not eval
    a = train_teacher.parse_args([])
    assert a.select_by == "recall" and a.topks == [20]
    a = train_teacher.parse_args(["--select_by", "ndcg", "--topks", "[5, 20]"])
    assert a.select_by == "ndcg" and a.topks == [5, 20]
    for bad in ("[20, 5]", "__import__('os').getcwd()", "[1,"):
        with pytest.raises(SystemExit):
            train_teacher.parse_args(["--topks", bad])
    with pytest.raises(SystemExit):
        train_teacher.parse_args(["--select_by", "auc"])


def test_trainer_rejects_an_unknown_selection_before_the_device():
    from gdd.rankformer import train_teacher
    with pytest.raises(ValueError, match="select_by"):
        train_teacher(4, 5, [0], [1], [0], [2], select_by="auc")
    with pytest.raises(ValueError):
        train_teacher(4, 5, [0], [1], [0], [2], select_by="ndcg", topks=[20])  # 20 > 5 items


def test_report_ranking_is_opt_in():
    from gdd import distill_recsys
    assert distill_recsys.parse_args([]).report_ranking is False
    a = distill_recsys.parse_args(["--report_ranking", "--report_topks", "[5, 20]"])
    assert a.report_ranking is True and a.report_topks == "[5, 20]"
