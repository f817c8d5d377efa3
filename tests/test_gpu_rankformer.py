"""The Rankformer teacher on the MI355X (gdd/rankformer.py, csrc/gdd_rankformer.hip): the two row
passes against numpy fp64, the layer and its gradient against the reference layer's recorded fp64
outputs, determinism, the negative sampler, and a short training run exported into the
distillation driver's KD branch.

Bounds. Kernels: every output element within 2 (deg + d) 2^-24 Σ|terms| of the exact value, the
forward bound of a sum of that many fp32 terms in any order (deg the row's length, d the dot
product's; the factor 2 covers the second-order terms); Σ|terms| is computed in fp64 from absolute
values (for A_r = Σ s_e V_c the terms are |q_f k_cf| |v_cg|). Layers: the largest absolute error
against the fixture's fp64 output is at most 4 x the reference's own fp32 error on the same input
(recorded in the fixture): the same sums in another order.

The kernel widths run from 1 to 256, so all four instantiations (one to four features per lane:
d <= 64, 128, 192, 256) execute under the same kernel bound, the out-of-range column also at
d = 193. The chunk geometry with poisoned buffers, the autograd functions against fp64 autograd
(2 (Dmax + d + 4) 2^-24 Σ|terms|), the clamp, cut rows, d = 193 and stacked layers against the second
fixture (4 x the reference's fp32 error), and a graph without pairs are in
test_gpu_rankformer_edges.py, with their bounds in its docstring."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rankformer_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
DIMS = [1, 8, 63, 64, 65, 128, 129, 192, 193, 255, 256]  # one to four features per lane
ROWS = 70


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def make_csr(n_cols, long_row, seed=5):
    """70 rows; lengths 0, 1, 2, 63, 64, 65 among random short ones; with ``long_row`` one row of
    3,000 distinct columns (cut into many chunks). Columns ascend within a row; the narrow variant
    (50 columns) repeats columns in its longer rows, which the passes sum entry by entry."""
    rng = np.random.RandomState(seed)
    lens = rng.randint(0, 12, ROWS)
    lens[[3, 10, 11, 20, 21, 22]] = [0, 1, 2, 63, 64, 65]
    lens[[0, ROWS - 1]] = [0, 0]
    if long_row:
        lens[40] = 3000
    cols = [np.sort(rng.choice(n_cols, l, replace=l > n_cols)) for l in lens]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return rowptr, np.concatenate(cols).astype(np.int32), lens


@pytest.fixture(scope="module", params=[(50, False), (4000, True)], ids=["narrow", "longrow"])
def csr(request):
    from gdd.rankformer import _Side
    n_cols, long_row = request.param
    rowptr, col, lens = make_csr(n_cols, long_row)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    side = _Side(ROWS, n_cols, dev(rowptr), dev(col), bad)
    return {"side": side, "rowptr": rowptr, "col": col, "lens": lens, "n_cols": n_cols,
            "rows": np.repeat(np.arange(ROWS), lens)}


def row_sum(rows, terms):
    out = np.zeros((ROWS,) + terms.shape[1:])
    np.add.at(out, rows, terms)
    return out


def check(name, got, exact, mag, count):
    got = got.cpu().numpy().astype(np.float64)
    bound = 2.0 * count * U24 * mag
    worst = float(np.max(np.abs(got - exact) - bound))
    ratio = float(np.max(np.abs(got - exact) / np.maximum(bound, 1e-300)))
    print(f"{name}: max err/bound = {ratio:.3f}")
    assert worst <= 0, (name, ratio)


@pytest.mark.parametrize("d", DIMS)
def test_rowpass_vs_fp64(csr, d):
    from gdd import rankformer as RF
    rng = np.random.RandomState(100 + d)
    n_cols, rows, col, lens = csr["n_cols"], csr["rows"], csr["col"], csr["lens"]
    Q = rng.standard_normal((ROWS, d)).astype(np.float32)
    K = rng.standard_normal((n_cols, d)).astype(np.float32)
    V = rng.standard_normal((n_cols, d)).astype(np.float32)
    s, s_sum, SK, SV, A = RF.rank_rowpass(csr["side"], dev(Q), dev(K), dev(V))
    torch.cuda.synchronize()
    assert int(csr["side"].bad.item()) == 0
    q, k, v = Q.astype(np.float64)[rows], K.astype(np.float64)[col], V.astype(np.float64)[col]
    s_x, s_m = (q * k).sum(1), (np.abs(q) * np.abs(k)).sum(1)
    deg1 = lens[:, None].astype(np.float64)
    check("s", s, s_x, s_m, d)
    check("s_sum", s_sum, row_sum(rows, s_x), row_sum(rows, s_m), lens + d)
    check("SK", SK, row_sum(rows, k), row_sum(rows, np.abs(k)), deg1 + d)
    check("SV", SV, row_sum(rows, v), row_sum(rows, np.abs(v)), deg1 + d)
    check("A", A, row_sum(rows, s_x[:, None] * v), row_sum(rows, s_m[:, None] * np.abs(v)), deg1 + d)
    empty = np.flatnonzero(lens == 0)
    assert not SK.cpu().numpy()[empty].any() and not A.cpu().numpy()[empty].any()
    assert not s_sum.cpu().numpy()[empty].any()


@pytest.mark.parametrize("d", DIMS)
def test_wsum_vs_fp64(csr, d):
    from gdd import rankformer as RF
    rng = np.random.RandomState(200 + d)
    n_cols, rows, col, lens = csr["n_cols"], csr["rows"], csr["col"], csr["lens"]
    E = col.shape[0]
    w, a, b = (rng.standard_normal(E).astype(np.float32) for _ in range(3))
    V = rng.standard_normal((n_cols, d)).astype(np.float32)
    Y, ta, tb = RF.rank_wsum(csr["side"], dev(w), dev(V), dev(a), dev(b))
    Y2, ta2, tb2 = RF.rank_wsum(csr["side"], dev(w), dev(V))
    torch.cuda.synchronize()
    assert ta2 is None and tb2 is None and torch.equal(Y, Y2)
    v, w64 = V.astype(np.float64)[col], w.astype(np.float64)[:, None]
    deg1 = lens[:, None].astype(np.float64)
    check("Y", Y, row_sum(rows, w64 * v), row_sum(rows, np.abs(w64) * np.abs(v)), deg1 + d)
    check("ta", ta, row_sum(rows, a.astype(np.float64)), row_sum(rows, np.abs(a).astype(np.float64)), lens + d)
    check("tb", tb, row_sum(rows, b.astype(np.float64)), row_sum(rows, np.abs(b).astype(np.float64)), lens + d)
    empty = np.flatnonzero(lens == 0)
    assert not Y.cpu().numpy()[empty].any() and not ta.cpu().numpy()[empty].any()


def test_width_above_the_limit_raises(csr):
    from gdd import _lib, rankformer as RF
    side, d = csr["side"], RF.MAX_DIM + 1
    Q = torch.zeros(ROWS, d, device="cuda")
    T = torch.zeros(csr["n_cols"], d, device="cuda")
    with pytest.raises(ValueError):
        RF.rank_rowpass(side, Q, T, T)
    with pytest.raises(ValueError):
        RF.rank_wsum(side, torch.zeros(side.nnz, device="cuda"), T)
    with pytest.raises(ValueError):
        RF.RankformerLayer()(torch.zeros(5, d, device="cuda"), None)
    # the library refuses it too (host-side validation, nothing launched)
    lib = _lib.device_lib()
    ws = _lib.workspace(lib.gdd_rank_ws_bytes(side.nnz, RF.MAX_DIM), "cuda")
    rc = lib.gdd_rank_wsum(ROWS, csr["n_cols"], side.nnz, side.rowptr.data_ptr(), side.col.data_ptr(), d,
                           T.data_ptr(), T.data_ptr(), None, None, Q.data_ptr(), None, None, None,
                           ws.data_ptr(), ws.numel(), None)
    assert rc != 0 and b"rank_wsum" in lib.gdd_last_error()


def test_out_of_range_column_sets_the_flag():
    out_of_range_column(64)


def test_out_of_range_column_sets_the_flag_four_features_per_lane():
    out_of_range_column(193)


def out_of_range_column(d):
    from gdd import rankformer as RF
    n_cols = 50
    rowptr, col, lens = make_csr(n_cols, False)
    rows = np.repeat(np.arange(ROWS), lens)
    hit = [int(rowptr[20]) + 5, int(rowptr[22]) + 64]  # inside a row, and a row's last entry
    col_bad = col.copy()
    col_bad[hit] = [n_cols, -1]
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    side = RF._Side(ROWS, n_cols, dev(rowptr), dev(col_bad), bad)
    rng = np.random.RandomState(9)
    Q = rng.standard_normal((ROWS, d)).astype(np.float32)
    K = rng.standard_normal((n_cols, d)).astype(np.float32)
    s, _, SK, _, _ = RF.rank_rowpass(side, dev(Q), dev(K), dev(K))
    torch.cuda.synchronize()
    assert int(bad.item()) != 0
    s = s.cpu().numpy()
    assert np.isnan(s[hit]).all() and np.isfinite(np.delete(s, hit)).all()
    keep = np.ones(col.shape[0], bool)
    keep[hit] = False
    exact = np.zeros((ROWS, d))
    np.add.at(exact, rows[keep], K.astype(np.float64)[col[keep]])
    np.testing.assert_allclose(SK.cpu().numpy(), exact, rtol=0, atol=1e-4)  # the entry left out
    bad.zero_()
    w = np.ones(col.shape[0], np.float32)
    Y, _, _ = RF.rank_wsum(side, dev(w), dev(K))
    torch.cuda.synchronize()
    assert int(bad.item()) != 0
    np.testing.assert_allclose(Y.cpu().numpy(), exact, rtol=0, atol=1e-4)


# ---- the layers against the reference's recorded outputs ---------------------------------------
@pytest.fixture(scope="module", params=R.CASES)
def case(request):
    from gdd.rankformer import InteractionGraph
    c = R.load_case(request.param)
    c["graph"] = InteractionGraph(c["u"], c["i"], int(c["n"]), int(c["m"]), "cuda")
    c["name"] = request.param
    return c


def layer_run(c):
    from gdd.rankformer import RankformerLayer
    x = dev(c["x"].astype(np.float32)).requires_grad_(True)
    z = RankformerLayer(2.0, 0.0)(x, c["graph"])
    (z * dev(c["W"].astype(np.float32))).sum().backward()
    c["graph"].check()
    return z.detach(), x.grad.detach()


def test_layer_forward_and_gradient_vs_reference(case):
    z, g = layer_run(case)
    for what, got, k64, k32 in (("forward", z, "z64", "z32"), ("gradient", g, "g64", "g32")):
        ref_err = float(np.abs(case[k32].astype(np.float64) - case[k64]).max())
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - case[k64]).max())
        print(f"{case['name']} {what}: err {err:.3e}, reference fp32 err {ref_err:.3e}, ratio {err / ref_err:.2f}")
        assert err <= 4 * ref_err, (what, err, ref_err)


@pytest.mark.parametrize("left,right,key", [(1.0, 0.0, "gcn"), (0.5, 0.5, "gcnb")])
def test_gcn_layer_vs_reference(case, left, right, key):
    from gdd.rankformer import GCNLayer
    x = dev(case["x"].astype(np.float32))
    z = GCNLayer(left, right)(x, case["graph"])
    case["graph"].check()
    ref_err = float(np.abs(case[key + "32"].astype(np.float64) - case[key + "64"]).max())
    err = float(np.abs(z.cpu().numpy().astype(np.float64) - case[key + "64"]).max())
    print(f"{case['name']} GCN({left}, {right}): err {err:.3e}, reference fp32 err {ref_err:.3e}, "
          f"ratio {err / ref_err:.2f}")
    assert err <= 4 * ref_err


def test_gcn_layer_gradient_is_the_transposed_sum(case):
    """d/dx of sum(GCN(x) * W) against the dense definition's autograd (fp64)."""
    from gdd.rankformer import GCNLayer
    x = dev(case["x"].astype(np.float32)).requires_grad_(True)
    (GCNLayer(0.5, 0.5)(x, case["graph"]) * dev(case["W"].astype(np.float32))).sum().backward()
    M = R.mask_of(case["u"], case["i"], int(case["n"]), int(case["m"]))
    x64 = torch.from_numpy(case["x"]).requires_grad_(True)
    (R.dense_gcn(x64, M, 0.5, 0.5) * torch.from_numpy(case["W"])).sum().backward()
    # a sum of at most max-degree terms of size |W| / sqrt(du di): the fp32 forward bound
    deg = max(int(M.sum(0).max()), int(M.sum(1).max()))
    bound = 2 * deg * U24 * float(R.dense_gcn(torch.from_numpy(np.abs(case["W"])), M, 0.5, 0.5).max())
    err = float((x.grad.cpu().double() - x64.grad).abs().max())
    print(f"{case['name']} GCN gradient: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def test_two_runs_are_bit_identical(case):
    z1, g1 = layer_run(case)
    z2, g2 = layer_run(case)
    assert torch.equal(z1, z2) and torch.equal(g1, g2)


def test_two_runs_are_bit_identical_with_cut_rows():
    """400 users x 150 items at density 0.1 with item 0 held by every user: rows of both
    orientations span several chunks."""
    from gdd.rankformer import InteractionGraph
    rng = np.random.RandomState(3)
    M = rng.random_sample((400, 150)) < 0.1
    M[:, 0] = True
    u, i = np.nonzero(M)
    c = {"graph": InteractionGraph(u, i, 400, 150, "cuda"),
         "x": 0.1 * rng.standard_normal((550, 64)), "W": rng.standard_normal((550, 64))}
    z1, g1 = layer_run(c)
    z2, g2 = layer_run(c)
    assert torch.equal(z1, z2) and torch.equal(g1, g2)
    assert bool(torch.isfinite(z1).all()) and bool(torch.isfinite(g1).all())
    # and the cut rows are summed right: the dense definition in fp64
    Mt = torch.from_numpy(M.astype(np.float64))
    x64 = torch.from_numpy(c["x"].astype(np.float32).astype(np.float64))
    z64 = R.dense_rankformer(x64, Mt)
    assert float((z1.cpu().double() - z64).abs().max()) <= 1e-5 * float(z64.abs().max())


def test_sampler_draws_no_training_pair():
    from gdd.rankformer import InteractionGraph, NegativeSampler
    c = R.load_case("wide")
    n, m = int(c["n"]), int(c["m"])
    g = InteractionGraph(c["u"], c["i"], n, m, "cuda")
    pick = torch.randint(0, g.E, (4096,), generator=torch.Generator().manual_seed(1))
    u = g.train_u[pick.to("cuda")]
    sampler = NegativeSampler(g, seed=7)
    j = sampler(u)
    assert j.shape == u.shape and int(j.min()) >= 0 and int(j.max()) < m
    pairs = set(zip(c["u"].tolist(), c["i"].tolist()))
    assert not any((a, b) in pairs for a, b in zip(u.tolist(), j.tolist()))
    assert len(set(j.tolist())) > m // 2  # draws, not a constant
    assert torch.equal(j, NegativeSampler(g, seed=7)(u))  # deterministic for a seed


# ---- training and the export -------------------------------------------------------------------
@pytest.fixture(scope="module")
def trained():
    from gdd.rankformer import train_teacher
    tr_u, tr_i, te_u, te_i = R.planted_blocks()
    model, hist = train_teacher(120, 80, tr_u, tr_i, te_u, te_i, max_epochs=40)
    return model, hist, (tr_u, tr_i, te_u, te_i)


def test_training_lowers_the_loss_and_raises_recall(trained):
    from gdd.recsys import RecallEvaluator
    model, hist, (tr_u, tr_i, te_u, te_i) = trained
    loss = hist["loss"]
    assert len(loss) == 40 and np.isfinite(loss).all()
    before = hist["valid"][0][1]
    with torch.no_grad():
        users, items = model.computer()
    after = RecallEvaluator(model.graph.to_scipy(), te_u, te_i, 20, "cuda", max_users=120)(users, items)
    print(f"loss {loss[0]:.4f} -> {loss[-1]:.4f}; held-out Recall@20 {before:.4f} -> {after:.4f}")
    assert loss[-1] < loss[0]
    assert after > before
    assert after == hist["best_recall"] and hist["best_epoch"] in (20, 40)


def test_saved_teacher_feeds_the_distillation_kd_branch(trained, tmp_path, capsys):
    from gdd import distill_recsys as D
    from gdd.rankformer import save_teacher
    model, _, (tr_u, tr_i, te_u, te_i) = trained
    os.makedirs(tmp_path / "planted")
    for name, (a, b) in (("train", (tr_u, tr_i)), ("valid", (te_u, te_i)), ("test", (te_u, te_i))):
        np.savetxt(tmp_path / "planted" / f"{name}.txt", np.stack([a, b], 1), fmt="%d")
    path = str(tmp_path / "teacher.pt")
    save_teacher(path, model)
    args = D.parse_args(["--data_dir", str(tmp_path), "--dataset", "planted", "--teacher_path", path,
                         "--refine_epochs", "3", "--svd_dim", "8", "--reduction_rate", "0.25",
                         "--batch_size", "256", "--device", "cuda"])
    D.run(args, out_root=str(tmp_path / "out"))
    out = capsys.readouterr().out
    assert "[teacher] KD will be applied during refinement." in out
    assert "[refine] ep=0003" in out and "[save]" in out
    assert os.path.exists(tmp_path / "out" / "distilled_recsys" / "planted" / "condensed_embeddings.pt")


def test_train_teacher_command_line(tmp_path, capsys):
    """python -m gdd.train_teacher's run(): two mini-batch epochs with a GCN layer in front, the
    file written where --out says."""
    from gdd import train_teacher as T
    tr_u, tr_i, te_u, te_i = R.planted_blocks()
    os.makedirs(tmp_path / "planted")
    for name, (a, b) in (("train", (tr_u, tr_i)), ("valid", (te_u, te_i)), ("test", (te_u, te_i))):
        np.savetxt(tmp_path / "planted" / f"{name}.txt", np.stack([a, b], 1), fmt="%d")
    out = str(tmp_path / "made" / "teacher.pt")
    model, hist = T.run(T.parse_args(["--data_dir", str(tmp_path), "--dataset", "planted", "--out", out,
                                      "--use_gcn", "--gcn_mean", "--gcn_left", "0.5", "--gcn_right", "0.5",
                                      "--loss_batch_size", "200", "--max_epochs", "2", "--valid_interval", "1",
                                      "--hidden_dim", "32"]))
    assert "[save] teacher embeddings saved to" in capsys.readouterr().out
    data = torch.load(out, map_location="cpu", weights_only=True)
    assert data["user_emb"].shape == (120, 32) and data["item_emb"].shape == (80, 32)
    assert len(hist["loss"]) == 2 and np.isfinite(hist["loss"]).all()
    assert torch.equal(data["user_emb"], model.embedding_user.weight.detach().cpu())
