"""The teacher's contrastive branch and ablation switches on the MI355X (gdd/rankformer.py).

* The layer under each switch and under all three against the fixture recorded from the reference
  (tests/golden/rankformer_cl.npz): forward and gradient within 4 x the reference's own fp32 error of
  the fp64 values (the dense definition of tests/infonce_ref.py, which test_infonce_host.py anchors
  in the fixture's stored rows). ``wide`` has an item without users: under ``del_neg`` at clamp 0 its
  row is 0/0 in the reference too; the NaN rows must coincide, and nothing is asserted of the
  gradient where the reference's is NaN.
* With the switches off the layer is bit-equal to ``RankformerLayer()``.
* ``computer()``'s contrastive view, with ``cl_eps = 0``, is bit-equal to the GCN layer applied
  ``cl_layer`` times to the raw table (one or two GCN layers, every ``cl_layer``, with ``gcn_mean``,
  and the raw table itself without GCN layers), and ``loss_bpr`` equals the dense fp64 loss of the
  same embeddings (BPR + reg + cl_lambda CL) within the sum of the parts' bounds. With E pairs of
  width d and u = 2^-24: a score is d rounded products summed, at most d u Σ|terms|; the difference
  of two scores, softplus (1-Lipschitz, 2u of its own) and the mean of E terms add
  u |x| + (E + 2) u softplus; the regulariser is a sum of 3 E d squares, at most (E d + 8) u of its
  value; the two InfoNCE terms carry infonce_ref.bounds_infonce; the final additions 3u of the total.
* The noise: every row of ``x_noisy − x_clean`` has norm ``cl_eps`` within fp32 rounding and the
  sign pattern of ``x``; none in ``eval()``.
* A 30-epoch full-batch run with ``use_cl`` and ``use_gcn``: finite losses, two runs with one seed
  bit-identical, the export in the ``--teacher_path`` format."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import infonce_ref as N  # noqa: E402
import rankformer_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
U = 2.0 ** -24


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


@pytest.fixture(scope="module")
def graphs():
    from gdd.rankformer import InteractionGraph
    out = {}
    for name in R.CASES:
        c = R.load_case(name)
        c["graph"] = InteractionGraph(c["u"], c["i"], int(c["n"]), int(c["m"]), "cuda")
        c["M"] = R.mask_of(c["u"], c["i"], int(c["n"]), int(c["m"]))
        out[name] = c
    return out


@pytest.mark.parametrize("name", N.LAYER_CASES)
def test_switched_layer_vs_reference(graphs, name):
    from gdd.rankformer import RankformerLayer
    base, fx = graphs[name.split("_")[0]], N.load_cl_case(name)
    sw = [bool(v) for v in fx["switches"]]
    x = dev(base["x"].astype(np.float32)).requires_grad_(True)
    z = RankformerLayer(2.0, 0.0, *sw)(x, base["graph"])
    (z * dev(base["W"].astype(np.float32))).sum().backward()
    base["graph"].check()
    x64 = torch.from_numpy(base["x"]).double().requires_grad_(True)
    with torch.no_grad():
        z64 = N.dense_rankformer(x64, base["M"], 2.0, 0.0, *sw)
    good = ~torch.isnan(z64).any(1)
    (N.dense_rankformer(x64, base["M"], 2.0, 0.0, *sw, rows=good) * torch.from_numpy(base["W"])[good]).sum().backward()
    zd, gd = z.detach().cpu().double(), x.grad.cpu().double()
    assert torch.equal(torch.isnan(zd), torch.isnan(z64)), "the 0/0 rows differ from the reference's"
    rows = fx["rows"]
    assert np.allclose(z64.numpy()[rows], fx["z64"], rtol=1e-12, atol=1e-14, equal_nan=True)
    g_ok = good.clone()  # the reference's gradient is NaN in the 0/0 item's own row
    z_err = float((zd - z64)[good].abs().max())
    g_err = float((gd - x64.grad)[g_ok].abs().max())
    for what, err, ref in (("forward", z_err, float(fx["z32_err"])), ("gradient", g_err, float(fx["g32_err"]))):
        print(f"{name} {what}: err {err:.3e}, reference fp32 err {ref:.3e}, ratio {err / ref:.2f}")
        assert err <= 4 * ref, (name, what, err, ref)


def test_switches_off_same_bits(graphs):
    from gdd.rankformer import RankformerLayer
    for name, c in graphs.items():
        outs = []
        for layer in (RankformerLayer(0.5, 0.6), RankformerLayer(0.5, 0.6, False, False, False)):
            x = dev(c["x"].astype(np.float32)).requires_grad_(True)
            z = layer(x, c["graph"])
            (z * dev(c["W"].astype(np.float32))).sum().backward()
            outs.append((z.detach(), x.grad))
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), name


# ---- the model -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted_graph():
    from gdd.rankformer import InteractionGraph
    tr_u, tr_i, te_u, te_i = R.planted_blocks()
    return InteractionGraph(tr_u, tr_i, 120, 80, "cuda"), (tr_u, tr_i, te_u, te_i)


def dense_loss(users, items, users_cl, items_cl, u0, i0, j0, u, i, j, reg_lambda, cl_lambda, cl_tau):
    """model.py:402-468 in fp64 from the embeddings given, and the bound of the module docstring."""
    E, d = u.shape[0], users.shape[1]
    ue, ie, je = users[u], items[i], items[j]
    s_ui, s_uj = (ue * ie).sum(-1), (ue * je).sum(-1)
    sp = F.softplus(s_uj - s_ui)
    reg = 0.5 * (u0.pow(2).sum() + i0.pow(2).sum() + j0.pow(2).sum()) / E
    uu, ii = torch.unique(u), torch.unique(i)
    cl_u, cl_i = N.dense_infonce(users[uu], users_cl[uu], cl_tau), N.dense_infonce(items[ii], items_cl[ii], cl_tau)
    total = sp.mean() + reg_lambda * reg + cl_lambda * (cl_u + cl_i)
    mags = (ue.abs() * ie.abs()).sum(-1) + (ue.abs() * je.abs()).sum(-1)
    bound = float((d * U * mags + U * (s_uj - s_ui).abs() + (E + 2) * U * sp).mean())
    bound += reg_lambda * (E * d + 8) * U * float(reg)
    bound += cl_lambda * (N.bounds_infonce(users[uu], users_cl[uu], cl_tau)[0]
                          + N.bounds_infonce(items[ii], items_cl[ii], cl_tau)[0])
    return float(total), bound + 3 * U * abs(float(total)), float(cl_u + cl_i)


CONFIGS = [dict(use_gcn=False), dict(use_gcn=True, gcn_layers=1, cl_layer=1),
           dict(use_gcn=True, gcn_layers=2, cl_layer=1), dict(use_gcn=True, gcn_layers=2, cl_layer=2),
           dict(use_gcn=True, gcn_layers=2, cl_layer=2, gcn_mean=True),
           dict(use_gcn=True, gcn_layers=2, cl_layer=1, gcn_mean=True)]


@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "-".join(f"{k}={v}" for k, v in c.items()))
def test_cl_view_and_loss(planted_graph, cfg):
    from gdd.rankformer import GCNLayer, RankformerTeacher
    graph, _ = planted_graph
    torch.manual_seed(5)
    model = RankformerTeacher(graph, hidden_dim=24, use_cl=True, cl_eps=0.0, cl_lambda=0.05, cl_tau=0.15,
                              seed=3, **cfg)
    model.train()
    users, items = model.computer()
    users_cl, items_cl = model.cl_view
    # the view: GCN applied cl_layer times to the raw table, whatever gcn_mean; the raw table without GCN
    raw = torch.cat([model.embedding_user.weight, model.embedding_item.weight], 0)
    want = raw
    if cfg["use_gcn"]:
        for _ in range(cfg["cl_layer"]):
            want = GCNLayer(1.0, 0.0)(want, graph)
    assert torch.equal(torch.cat([users_cl, items_cl], 0), want)
    u, i = graph.train_u, graph.train_i
    j = model.sampler(u)
    loss = model.loss_bpr(users, items, u, i, 1e-4, j=j)
    loss.backward()
    assert bool(torch.isfinite(model.embedding_user.weight.grad).all())
    f64 = lambda t: t.detach().cpu().double()  # noqa: E731
    uc, ic, jc = u.cpu(), i.cpu(), j.cpu()
    ref, bound, cl = dense_loss(f64(users), f64(items), f64(users_cl), f64(items_cl),
                                f64(model.embedding_user.weight)[uc], f64(model.embedding_item.weight)[ic],
                                f64(model.embedding_item.weight)[jc], uc, ic, jc, 1e-4, 0.05, 0.15)
    loss = loss.detach()
    err = abs(float(loss) - ref)
    print(f"{cfg}: loss {float(loss):.6f} (CL part {cl:.4f}), err {err:.3e}, bound {bound:.3e}, "
          f"err/bound {err / bound:.3f}")
    assert err <= bound
    assert 0.05 * cl > 100 * bound  # the contrastive term is far above the bound: leaving it out would show
    # a mini-batch takes the unique users and items of the batch
    pick = torch.arange(0, graph.E, 7, device="cuda")
    users, items = model.computer()
    part = model.loss_bpr(users, items, u[pick], i[pick], 1e-4, j=j[pick])
    users_cl, items_cl = model.cl_view
    pc = pick.cpu()
    ref, bound, _ = dense_loss(f64(users), f64(items), f64(users_cl), f64(items_cl),
                               f64(model.embedding_user.weight)[uc[pc]], f64(model.embedding_item.weight)[ic[pc]],
                               f64(model.embedding_item.weight)[jc[pc]], uc[pc], ic[pc], jc[pc], 1e-4, 0.05, 0.15)
    assert abs(float(part.detach()) - ref) <= bound


def test_noise_norm_sign_and_eval(planted_graph):
    from gdd.rankformer import GCNLayer, RankformerTeacher
    graph, _ = planted_graph
    eps, d = 0.1, 32
    model = RankformerTeacher(graph, hidden_dim=d, use_gcn=True, gcn_layers=1, use_rankformer=False, use_cl=True,
                              cl_eps=eps, seed=11)
    raw = torch.cat([model.embedding_user.weight, model.embedding_item.weight], 0).detach()
    clean = GCNLayer(1.0, 0.0)(raw, graph)
    model.train()
    with torch.no_grad():
        model.computer()
        noisy = torch.cat(model.cl_view, 0)
        model.computer()
        again = torch.cat(model.cl_view, 0)
    diff = (noisy.double() - clean.double()).cpu()
    full = (clean != 0).all(1).cpu()  # a row without pairs is all zeros: sign(0) = 0, no noise
    assert int(full.sum()) >= 190
    tol = eps * (d + 4) * U + 2 * d ** 0.5 * U * (float(clean.abs().max()) + eps)
    norms = diff.norm(dim=1)
    print(f"noise norms in [{float(norms[full].min()):.9f}, {float(norms[full].max()):.9f}], tol {tol:.2e}")
    assert bool(((norms[full] - eps).abs() <= tol).all())
    assert bool((diff * torch.sign(clean.double().cpu()) >= 0).all())
    assert not diff[~full].any()
    assert not torch.equal(noisy, again)  # a fresh draw per pass
    fresh = RankformerTeacher(graph, hidden_dim=d, use_gcn=True, gcn_layers=1, use_rankformer=False, use_cl=True,
                              cl_eps=eps, seed=11)
    fresh.load_state_dict(model.state_dict())
    fresh.train()
    with torch.no_grad():
        fresh.computer()
    assert torch.equal(torch.cat(fresh.cl_view, 0), noisy)  # the seed reproduces the draw
    model.eval()
    with torch.no_grad():
        users, items = model.computer()
    assert torch.equal(torch.cat(model.cl_view, 0), clean) and torch.equal(torch.cat([users, items], 0), clean)


def test_training_with_cl_is_reproducible(planted_graph, tmp_path):
    from gdd.rankformer import save_teacher, train_teacher
    _, (tr_u, tr_i, te_u, te_i) = planted_graph
    runs = []
    for _ in range(2):
        model, hist = train_teacher(120, 80, tr_u, tr_i, te_u, te_i, max_epochs=30, use_cl=True, use_gcn=True)
        runs.append((model, hist))
    (m1, h1), (m2, h2) = runs
    assert len(h1["loss"]) == 30 and np.isfinite(h1["loss"]).all()
    assert np.array_equal(np.asarray(h1["loss"]).view(np.uint64), np.asarray(h2["loss"]).view(np.uint64))
    assert torch.equal(m1.embedding_user.weight, m2.embedding_user.weight)
    assert torch.equal(m1.embedding_item.weight, m2.embedding_item.weight)
    plain = train_teacher(120, 80, tr_u, tr_i, te_u, te_i, max_epochs=3, use_gcn=True)[1]
    assert h1["loss"][0] > plain["loss"][0]  # the contrastive term is in the loss
    path = str(tmp_path / "teacher.pt")
    save_teacher(path, m1)
    data = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(data) == ["item_emb", "user_emb"]
    assert data["user_emb"].shape == (120, 64) and data["item_emb"].shape == (80, 64)
    assert data["user_emb"].dtype == torch.float32
    assert torch.equal(data["user_emb"], m1.embedding_user.weight.detach().cpu())
