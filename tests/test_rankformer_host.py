"""CPU checks of the Rankformer teacher (no GPU): the dense fp64 definition of the layer
(tests/rankformer_ref.py) against the reference layer's recorded outputs
(tests/golden/rankformer_layer.npz, tools/make_golden_rankformer.py), the input validation, and the
export's format.

Bounds: the dense definition and the reference's linearised evaluation are the same function in
fp64; on outputs of size 0.15 (gradients of size 1.4) their difference is a few ulps (measured
7e-17 and 2.5e-15), so 1e-12 absolute separates rounding from any change of the definition. The
second fixture (rankformer_layer_more.npz: the clamp at (alpha, clamp) = (0.5, 0.6) and (0.25, 0.3),
the cut-row case, d = 193, two stacked layers) is held to the same 1e-12 (measured at most 2.6e-16
and 5.9e-15), and its clamp cases to the conditions that make them worth running: each of the three
clamped denominators is clamped on some rows and not on others, and none lies within 1e-4 of the
clamp value (their fp32 error is about 1e-7; a kink that close would make the fp32 and fp64
gradients differ legitimately)."""
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rankformer_ref as R  # noqa: E402

ABS = 1e-12


@pytest.fixture(scope="module", params=R.CASES)
def case(request):
    c = R.load_case(request.param)
    n, m = int(c["n"]), int(c["m"])
    c["M"] = R.mask_of(c["u"], c["i"], n, m)
    return c


def test_fixture_holds_the_edge_cases():
    small, wide = R.load_case("small"), R.load_case("wide")
    for c, shape in ((small, (37, 29, 8)), (wide, (61, 45, 64))):
        n, m = int(c["n"]), int(c["m"])
        assert (n, m, c["x"].shape[1]) == shape and c["x"].shape[0] == n + m
        deg = np.bincount(c["u"], minlength=n)
        assert deg[0] == 0  # a user with no positives
        assert 0.1 < c["u"].shape[0] / (n * m) < 0.25
        assert np.array_equal(c["x"], c["x"].astype(np.float32).astype(np.float64))
    assert np.bincount(small["u"], minlength=37)[1] == 29  # a user with every item
    assert np.bincount(wide["i"], minlength=45)[2] == 0  # an item with no user
    assert np.bincount(wide["u"], minlength=61)[1] == 44


def test_dense_definition_equals_reference_layer(case):
    z = R.dense_rankformer(torch.from_numpy(case["x"]), case["M"])
    err = float((z - torch.from_numpy(case["z64"])).abs().max())
    print(f"dense layer vs reference fp64: {err:.3e}")
    assert err <= ABS


def test_dense_gcn_equals_reference_layer(case):
    x = torch.from_numpy(case["x"])
    for key, (left, right) in (("gcn64", (1.0, 0.0)), ("gcnb64", (0.5, 0.5))):
        err = float((R.dense_gcn(x, case["M"], left, right) - torch.from_numpy(case[key])).abs().max())
        print(f"dense GCN({left}, {right}) vs reference fp64: {err:.3e}")
        assert err <= ABS


def test_dense_definition_gradient_equals_reference(case):
    x = torch.from_numpy(case["x"]).requires_grad_(True)
    (R.dense_rankformer(x, case["M"]) * torch.from_numpy(case["W"])).sum().backward()
    err = float((x.grad - torch.from_numpy(case["g64"])).abs().max())
    print(f"dense gradient vs reference fp64: {err:.3e}")
    assert err <= ABS


@pytest.fixture(scope="module", params=list(R.MORE_CASES))
def more(request):
    c = R.load_more_case(request.param)
    c["M"] = R.mask_of(c["u"], c["i"], int(c["n"]), int(c["m"]))
    return c


def test_second_fixture_holds_what_it_is_for():
    assert os.path.getsize(R.GOLDEN_MORE) < 2 ** 20
    cut = R.load_more_case("cut_c05")
    n, m = int(cut["n"]), int(cut["m"])
    assert (n, m, cut["x"].shape) == (100, 80, (180, 65))
    du, di = np.bincount(cut["u"], minlength=n), np.bincount(cut["i"], minlength=m)
    assert du[0] == 0 and du[1] == m - 1 and di[0] == n - 1 and di[5] == 0
    assert 0.1 < cut["u"].shape[0] / (n * m) < 0.25
    # rows of both orientations span more than one 32-entry chunk
    assert du.max() > 64 and di.max() > 96
    assert R.load_more_case("small193")["x"].shape == (66, 193)
    for name in R.MORE_CASES:
        c = R.load_more_case(name)
        assert c["z64"].dtype == c["g64"].dtype == np.float64 and c["z64"].shape == c["x"].shape == c["W"].shape
        assert np.array_equal(c["x"], c["x"].astype(np.float32).astype(np.float64))
        assert 0 < float(c["z32_err"]) < 1e-5 and 0 < float(c["g32_err"]) < 1e-4


def test_dense_definition_equals_reference_on_the_second_fixture(more):
    """Output and gradient at the clamp settings, on cut rows, at d = 193 and stacked twice."""
    x = torch.from_numpy(more["x"]).requires_grad_(True)
    z = R.dense_stack(x, more["M"], more["alpha"], more["clamp"], more["layers"])
    (z * torch.from_numpy(more["W"])).sum().backward()
    ez = float((z.detach() - torch.from_numpy(more["z64"])).abs().max())
    eg = float((x.grad - torch.from_numpy(more["g64"])).abs().max())
    print(f"{more['name']}: dense vs reference fp64: output {ez:.3e}, gradient {eg:.3e}")
    assert ez <= ABS and eg <= ABS


@pytest.mark.parametrize("name", [k for k, v in R.MORE_CASES.items() if v[2] > 0])
def test_clamp_is_active_on_some_rows_and_no_denominator_sits_on_it(name):
    """Each of the three denominators is clamped for at least one row and unclamped for at least
    one, and none lies within 1e-4 of the clamp value (their fp32 error is about 1e-7)."""
    more = R.load_more_case(name)
    more["M"] = R.mask_of(more["u"], more["i"], int(more["n"]), int(more["m"]))
    counts, gap = R.clamp_conditions(torch.from_numpy(more["x"]), more["M"], more["alpha"], more["clamp"])
    print(f"{more['name']}: clamped (D_u, item sum of Omega+, item -sum of Omega-) = {counts}, closest {gap:.2e}")
    assert all(0 < k < total for k, total in counts)
    assert gap >= 1e-4


def test_plain_passes_are_the_dense_sums():
    """rankformer_ref's gather / index_add_ definitions of the two passes against dense matrix
    products on the autograd tests' graph (fp64: a few ulps)."""
    u, i, n, m = R.autograd_pairs()
    M = R.mask_of(u, i, n, m)
    deg_r, deg_c = M.sum(1), M.sum(0)
    assert deg_c[0] == n - 1 and deg_r[3] == m - 1 and deg_r[5] == 0 and deg_c[7] == 0
    assert 0.1 < len(u) / (n * m) < 0.25
    g = torch.Generator().manual_seed(0)
    Q, K, V = (torch.randn(r, 5, dtype=torch.float64, generator=g) for r in (n, m, m))
    rows, col = torch.from_numpy(u), torch.from_numpy(i)
    s, s_sum, SK, SV, A = R.plain_rowpass(rows, col, n, Q, K, V)
    S = Q @ K.t()
    for got, want in ((s, S[rows, col]), (s_sum, (M * S).sum(1)), (SK, M @ K), (SV, M @ V), (A, (M * S) @ V)):
        assert float((got - want).abs().max()) <= ABS
    w, a = torch.randn(len(u), dtype=torch.float64, generator=g), torch.randn(len(u), dtype=torch.float64, generator=g)
    Wm = torch.zeros(n, m, dtype=torch.float64)
    Wm[rows, col] = w
    Y, ta, tb = R.plain_wsum(rows, col, n, w, V, a)
    assert tb is None and float((Y - Wm @ V).abs().max()) <= ABS
    Am = torch.zeros(n, m, dtype=torch.float64)
    Am[rows, col] = a
    assert float((ta - Am.sum(1)).abs().max()) <= ABS
    assert [sum(p) for p in R.PATTERNS] == [0, 1, 31, 32, 33, 96, 96, 96, 96, 75, 100, 73]


def test_duplicate_pairs_raise():
    from gdd.rankformer import InteractionGraph
    with pytest.raises(ValueError, match="duplicate"):
        InteractionGraph([0, 1, 0], [2, 3, 2], 4, 5)
    with pytest.raises(IndexError):
        InteractionGraph([0, 4], [2, 3], 4, 5)
    with pytest.raises(ValueError):
        InteractionGraph([0, 1], [2], 4, 5)


def test_width_limit_is_the_librarys():
    from gdd import _lib, rankformer
    assert _lib.load().gdd_rank_max_dim() == rankformer.MAX_DIM >= 128  # host-only query
    assert _lib.load().gdd_rank_ws_bytes(121178, 64) >= 2 * (121178 // 32) * (3 * 64 + 1) * 4
    with pytest.raises(ValueError):
        rankformer._check_dim(rankformer.MAX_DIM + 1)


def test_save_teacher_file_passes_the_drivers_loader_checks(tmp_path):
    """The checks of gdd.distill_recsys.run on --teacher_path (keys, row counts, width, a
    weights-only load) on a file written by save_teacher."""
    from gdd import distill_recsys as D
    from gdd.rankformer import save_teacher
    n, m, d = 13, 7, D.parse_args([]).embed_dim
    model = types.SimpleNamespace(embedding_user=torch.nn.Embedding(n, d), embedding_item=torch.nn.Embedding(m, d))
    path = str(tmp_path / "teacher.pt")
    save_teacher(path, model)
    data = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(data) == ["item_emb", "user_emb"]
    tu, ti = data["user_emb"], data["item_emb"]
    assert tu.shape == (n, d) and ti.shape == (m, d)
    assert tu.dtype == ti.dtype == torch.float32 and tu.device.type == "cpu" and not tu.requires_grad
    assert torch.equal(tu, model.embedding_user.weight.detach())
    assert torch.equal(ti, model.embedding_item.weight.detach())
