"""CPU checks of the Rankformer teacher (no GPU): the dense fp64 definition of the layer
(tests/rankformer_ref.py) against the reference layer's recorded outputs
(tests/golden/rankformer_layer.npz, tools/make_golden_rankformer.py), the input validation, and the
export's format.

Bounds: the dense definition and the reference's linearised evaluation are the same function in
fp64; on outputs of size 0.15 (gradients of size 1.4) their difference is a few ulps (measured
7e-17 and 2.5e-15), so 1e-12 absolute separates rounding from any change of the definition."""
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
