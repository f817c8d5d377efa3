"""PositionEvaluator, ranking_fidelity and the two distill_recsys flags on the device.

Bounds. Per user, ``metrics_from_positions`` and ``gdd_rank_metrics`` do the same fp64 operations in
the same order (tests/test_rankpos_host.py), so precision, recall and NDCG per user are bit-equal
wherever the cut-off is within the list. The means add B non-negative fp64 terms in two different
orders (numpy's pairwise sum, the kernel's fixed tree): each sum is within B 2^-53 relative of the
exact one, so they agree within 2 B 2^-53 relative. The fidelity means are compared against plain
numpy means of the same integers: rel 1e-12.
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

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


@pytest.fixture(scope="module")
def fx():
    f = R.load_fixture()
    n, m = int(f["n"]), int(f["m"])
    f["train"] = sp.coo_matrix((np.ones(f["train_u"].shape[0], np.float32), (f["train_u"], f["train_i"])),
                               shape=(n, m)).tocsr()
    return f


@pytest.mark.parametrize("count_repeats", [True, False])
def test_per_user_metrics_are_those_of_the_ranked_lists(fx, count_repeats):
    import gdd
    topks = R.FIXTURE_TOPKS
    U, V = dev(fx["U"]), dev(fx["V"])
    kw = dict(device="cuda", count_repeats=count_repeats)
    lists_ev = gdd.RankingEvaluator(fx["train"], fx["valid_u"], fx["valid_i"], topks, **kw)
    pos_ev = gdd.PositionEvaluator(fx["train"], fx["valid_u"], fx["valid_i"], topks, **kw)
    assert np.array_equal(pos_ev.users, lists_ev.users)
    want = lists_ev(U, V)
    g = lists_ev._dev
    per, _, _ = gdd.rank_metrics(lists_ev.ranked(U, V), g["te_ptr"], g["te_col"], g["deg"], topks)
    got = pos_ev(U, V)
    assert sorted(got) == ["mean_rank", "mrr", "ndcg", "precision", "recall", "users"]
    assert got["users"] == want["users"] == len(pos_ev.users)
    assert np.array_equal(pos_ev.last["per_user"], per.cpu().numpy())
    B = got["users"]
    for key in ("precision", "recall", "ndcg"):
        rel = np.abs(got[key] - want[key]) / want[key]
        print(f"{key}: means rel {rel}, bound {2 * B * 2.0 ** -53}")
        assert (rel <= 2 * B * 2.0 ** -53).all() and want[key].min() > 0
    # the positions themselves against the definition (grid tables), then MRR and the mean rank
    (mp, mc), te_ptr, te_col, deg = lists_ev._host
    pos = pos_ev.positions(U, V).cpu().numpy()
    assert np.array_equal(pos, P.positions(P.masked_scores32(fx["U"], fx["V"], pos_ev.users, (mp, mc)), te_ptr, te_col))
    mrr, mean_rank, count = P.direct_metrics(pos, te_ptr, deg)
    assert count == B and got["mrr"] == pytest.approx(mrr, rel=1e-12)
    assert got["mean_rank"] == pytest.approx(mean_rank, rel=1e-12)


def test_cutoffs_past_the_list_limit_and_the_condensed_route(fx):
    """Cut-offs 300 and 500 = I, nine of them (RankingEvaluator takes neither); ``.condensed`` gives the
    dictionary of ``__call__`` on the expanded tables, value for value."""
    import gdd
    rng = np.random.RandomState(21)
    n, m = int(fx["n"]), int(fx["m"])
    topks = (1, 2, 5, 10, 20, 50, 256, 300, 500)
    num_cu, num_ci, d = 30, 50, 16
    cu, ci = dev(R.grid(rng, num_cu, d)), dev(R.grid(rng, num_ci, d))
    u2cu, i2ci = rng.randint(0, num_cu, n), rng.randint(0, num_ci, m)
    ev = gdd.PositionEvaluator(fx["train"], fx["valid_u"], fx["valid_i"], topks, "cuda")
    want = ev(cu[dev(u2cu)], ci[dev(i2ci)])
    want_per = ev.last["per_user"]
    got = ev.condensed(cu, ci, u2cu, i2ci)
    assert sorted(got) == sorted(want) and got["users"] == want["users"] > 0
    for key in ("precision", "recall", "ndcg"):
        assert np.array_equal(got[key], want[key]) and got[key].shape == (9,)
    assert got["mrr"] == want["mrr"] and got["mean_rank"] == want["mean_rank"]
    assert np.array_equal(ev.last["per_user"], want_per)
    # against the definition on full-length lists
    users = ev.users
    (mp, mc), te_ptr, te_col, deg = ev._prep._host
    U = cu.cpu().numpy()[u2cu]
    V = ci.cpu().numpy()[i2ci]
    lists, _ = R.ranked(R.scores64(U, V, users, (mp, mc)), m)
    ref_per, ref_sums, ref_count = R.metrics(lists, te_ptr, te_col, deg, (1, 50, 300, 500))
    assert np.array_equal(want_per[:, :, [0, 5, 7, 8]], ref_per) and ref_count == want["users"]
    assert 0 < want["recall"][-1] <= 1.0


def test_fidelity_of_a_model_against_itself_and_a_shuffled_copy(fx):
    import gdd
    from gdd import rankpos
    rng = np.random.RandomState(5)
    topks = (1, 5, 20, 50)
    U, V = dev(fx["U"]), dev(fx["V"])
    users = rng.permutation(int(fx["n"]))[:100]
    same = gdd.ranking_fidelity((U, V), (U, V), topks, users=users, exclude=fx["train"])
    assert list(same["overlap"]) == [1.0] * 4 and same["users"] == 100
    assert list(same["mean_position"]) == [(k - 1) / 2 for k in topks]

    # the student: the teacher's items under a shuffled item table (another ranking of the same items)
    Vs = V[dev(rng.permutation(int(fx["m"])))]
    f = gdd.ranking_fidelity((U, V), (U, Vs), topks, users=users, exclude=fx["train"])
    lists = gdd.recommend(U, V, 50, users=users, exclude=fx["train"]).cpu().numpy()
    full = gdd.recommend(U, Vs, 256, users=users, exclude=fx["train"]).cpu().numpy()
    spos = gdd.rank_positions(U, Vs, lists, users=users, exclude=fx["train"]).cpu().numpy()
    for j, k in enumerate(topks):
        inter = np.mean([len(np.intersect1d(lists[b, :k], full[b, :k])) / k for b in range(100)])
        assert f["overlap"][j] == pytest.approx(inter, rel=1e-12)
        assert f["mean_position"][j] == pytest.approx(np.mean([spos[b, :k].mean() for b in range(100)]), rel=1e-12)
    assert f["overlap"][-1] < 1.0

    # a condensed student goes through gdd_cluster_positions: the same numbers as its expanded tables
    num_cu, num_ci = 30, 50
    cu, ci = dev(R.grid(rng, num_cu, 16)), dev(R.grid(rng, num_ci, 16))
    u2cu, i2ci = rng.randint(0, num_cu, int(fx["n"])), rng.randint(0, num_ci, int(fx["m"]))
    rec = gdd.CondensedRecommender(cu, ci, u2cu, i2ci)
    a = gdd.ranking_fidelity((U, V), rec, topks, users=users, exclude=fx["train"])
    b = gdd.ranking_fidelity((U, V), (cu[dev(u2cu)], ci[dev(i2ci)]), topks, users=users, exclude=fx["train"])
    assert np.array_equal(a["overlap"], b["overlap"]) and np.array_equal(a["mean_position"], b["mean_position"])
    assert rec.last_info["ranked_clusters"] == len(np.unique(u2cu[users]))
    with pytest.raises(ValueError, match="outside"):
        rankpos.ranking_fidelity((U, V), (U, V), (300,), users=users)  # the teacher's list is recommend()'s


def test_distill_recsys_flags(tmp_path, capsys):
    """--report_full_ranking and --report_fidelity print their lines, the same through the cluster
    kernel; the full-ranking lines repeat --report_ranking's numbers; without the flags stdout is as
    before."""
    from gdd import distill_recsys as D
    from rankformer_ref import planted_blocks
    tr_u, tr_i, te_u, te_i = planted_blocks()
    os.makedirs(tmp_path / "planted")
    for name, (a, b) in (("train", (tr_u, tr_i)), ("valid", (te_u, te_i)), ("test", (te_u, te_i))):
        np.savetxt(tmp_path / "planted" / f"{name}.txt", np.stack([a, b], 1), fmt="%d")
    gen = torch.Generator().manual_seed(3)
    teacher = str(tmp_path / "teacher.pt")
    torch.save({"user_emb": torch.randn(120, 64, generator=gen), "item_emb": torch.randn(80, 64, generator=gen)},
               teacher)
    base = ["--data_dir", str(tmp_path), "--dataset", "planted", "--refine_epochs", "3", "--svd_dim", "8",
            "--svd_backend", "device", "--reduction_rate", "0.25", "--batch_size", "256", "--device", "cuda",
            "--teacher_path", teacher, "--report_ranking", "--report_topks", "[5, 20, 70]"]

    def run(extra, out):
        D.run(D.parse_args(base + extra), out_root=str(tmp_path / out))
        return [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith("[save]")]

    new = ("[rank-full]", "[fidelity]")
    plain = run([], "plain")
    assert not [ln for ln in plain if ln.startswith(new)]
    flags = run(["--report_full_ranking", "--report_fidelity"], "flags")
    assert [ln for ln in flags if not ln.startswith(new)] == plain
    full = [ln for ln in flags if ln.startswith("[rank-full] condensed (")]
    fid = [ln for ln in flags if ln.startswith("[fidelity] overlap@")]
    assert len(full) == 4 and len(fid) == 3
    rank = [ln for ln in plain if ln.startswith("[rank] condensed")]
    assert [ln.replace("[rank-full]", "[rank]") for ln in full[:3]] == rank
    assert full[0].split(": ")[1].startswith("ndcg@5 = ") and ", recall@5 = " in full[0] and ", pre@5 = " in full[0]
    assert full[3].split(": ")[1].startswith("mrr = ") and ", mean rank = " in full[3]
    for k, ln in zip((5, 20, 70), fid):
        assert ln.startswith(f"[fidelity] overlap@{k} = ") and f", mean position of the teacher's top {k} = " in ln
        assert 0.0 <= float(ln.split(" = ")[1].split(",")[0]) <= 1.0
    clusters = run(["--report_full_ranking", "--report_fidelity", "--report_from_clusters"], "clusters")
    assert [ln for ln in clusters if ln.startswith(new)] == full + fid

    with pytest.raises(ValueError, match="needs --teacher_path"):
        D.run(D.parse_args([a for a in base if a not in ("--teacher_path", teacher)] + ["--report_fidelity"]),
              out_root=str(tmp_path / "none"))
