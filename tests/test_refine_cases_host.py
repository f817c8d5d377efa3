"""That the inputs of tests/test_gpu_refine_forms.py (tests/refine_cases.py) have the properties its
cases rest on, asserted from the fp64 reference (tests/refine_ref.py) and the host grouping alone. No GPU.

* the row ladder: both sides' row lengths from the CSR, the long rows in different waves of their blocks;
* the group ladder: both sides' group sizes from ``group_bpr_triplets``' record, an item positive and
  negative in interleaved triplets, ``pos == neg``, repeated triplets;
* the loss fold's block count, the logits inside rows and the vanishing row and column, the non-zero
  edge gradient at L = 0;
* the bound: F times the yardstick stays below the earlier contract (1e-4) for every tensor of every
  case, and every loss term, dropped from the fp64 reference at the designated case, moves the loss and
  each gradient it enters by at least 100 F yardsticks;
* the reference's own additions: ``reverse=`` is the same function in fp64, ``drop=`` of a term that is
  absent changes nothing, ``adam_step64`` against ``manual_adam_step``."""
import numpy as np
import pytest
import torch

import refine_cases as RC
import refine_ref as R
from gdd import recsys

KEPT_CONTRACT = 1e-4  # tests/test_gpu_refine.py: gradients rtol 1e-4


def _lengths(c):
    nu, ni = c["params"]["user_emb.weight"].shape[0], c["params"]["item_emb.weight"].shape[0]
    cu, ci = c["edge_index"]
    return np.bincount(cu, minlength=nu), np.bincount(ci, minlength=ni)


# ---- 1. rows -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 8])
def test_row_ladder_lengths_on_both_sides(d):
    n = len(RC.LADDER)
    rows, cols = _lengths(RC.row_ladder(False, d))
    assert tuple(rows[:n]) == RC.LADDER and rows[n:].max() < RC.GATHER and cols.max() <= RC.LADDER_ROWS
    assert cols.min() >= 1  # the full row
    rows_t, cols_t = _lengths(RC.row_ladder(True, d))
    assert tuple(cols_t[:n]) == RC.LADDER and np.array_equal(rows_t, cols) and np.array_equal(cols_t, rows)
    # the edges are in CSR order on both (DeviceRefiner's graph wants it), the transpose through perm
    for t in (False, True):
        cu, ci = RC.row_ladder(t, d)["edge_index"]
        key = cu * (RC.LADDER_ITEMS if not t else RC.LADDER_ROWS) + ci
        assert (np.diff(key) > 0).all()
    # turns of the 64-entry loops: 0, 1, 2, 3 and 4; every side of a 16-entry gather batch and of a turn
    assert {(x + RC.CHUNK - 1) // RC.CHUNK for x in RC.LADDER} == {0, 1, 2, 3, 4}
    for edge in (RC.GATHER, RC.CHUNK, 2 * RC.CHUNK):
        assert {edge - 1, edge, edge + 1} <= set(RC.LADDER)
    # the rows of 63+ entries: as users node r, as items node 200 + r, 200 a multiple of the four waves
    long_rows = [r for r, x in enumerate(RC.LADDER) if x >= RC.CHUNK - 1]
    assert RC.LADDER_ITEMS % 4 == 0 and {r % 4 for r in long_rows} == {0, 1, 2, 3}
    for length in (RC.CHUNK, 2 * RC.CHUNK):  # each edge's three rows in three different waves
        assert len({RC.LADDER.index(length + k) % 4 for k in (-1, 0, 1)}) == 3


# ---- 2. groups -----------------------------------------------------------------------------------------
def test_group_ladder_sizes_from_the_record():
    c = RC.group_ladder()
    u, pos, neg = c["u"], c["pos_i"], c["neg_i"]
    nu, ni, b = len(RC.GROUPS), len(RC.ITEM_GROUPS), u.shape[0]
    assert c["params"]["user_emb.weight"].shape[0] == nu and c["params"]["item_emb.weight"].shape[0] == ni
    p = recsys.split_batch_record(recsys.group_bpr_triplets(u, pos, neg, nu, ni), b, nu, ni)
    assert tuple(np.diff(p["uptr"])) == RC.GROUPS and tuple(np.diff(p["iptr"])) == RC.ITEM_GROUPS
    for sizes in (RC.GROUPS, RC.ITEM_GROUPS):
        assert {0, 1, 63, 64, 65, 128, 129} <= set(sizes) and max(sizes) >= 193
    # positive and negative in interleaved triplets: in every item group of 63+ entries the signs
    # change many times along the group's (triplet) order
    for it in range(ni):
        ent = p["ient"][p["iptr"][it]:p["iptr"][it + 1]]
        assert (np.diff(ent) > 0).all()
        if ent.shape[0] >= 63:
            assert np.count_nonzero(np.diff(ent & 1)) >= 10, it
    same = np.flatnonzero(pos == neg)
    assert same.size >= 1 and c["edge_index"].shape[1] > 0
    # such a triplet's two entries are neighbours in its item's group
    t = int(same[0])
    ent = list(p["ient"][p["iptr"][pos[t]]:p["iptr"][pos[t] + 1]])
    assert ent.index(2 * t + 1) == ent.index(2 * t) + 1
    _, counts = np.unique(np.stack([u, pos, neg]), axis=1, return_counts=True)
    assert counts.max() >= 3  # repeated identical triplets


# ---- 3 .. 7 --------------------------------------------------------------------------------------------
def test_width_and_layer_cases_have_edges_and_no_idle_row():
    for d in RC.WIDTHS:
        rows, cols = _lengths(RC.width(d))
        assert rows.shape == (9,) and cols.shape == (7,) and rows.min() >= 1 and cols.min() >= 1
        assert RC.width(d)["params"]["user_emb.weight"].shape[1] == d and RC.width(d)["u"].shape == (40,)
    # both sides of every per-lane slot edge, of the 16-lane triplet dot and of d % 4
    assert {63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 15, 16, 17} <= set(RC.WIDTHS)
    assert {d % 4 for d in RC.WIDTHS} == {0, 1, 2, 3}
    for n in RC.LAYERS:
        assert _lengths(RC.layers(n))[0].sum() > 0
    assert RC.layers(2, True)["edge_index"].shape[1] == 0 and RC.adam(True)["edge_index"].shape[1] == 0


def test_edge_gradient_at_zero_layers_is_the_weight_regulariser_alone():
    c = RC.case("layers-0")
    g = R.references("layers-0")["ref"][1]["edge_logit"]
    assert g.size > 0 and np.abs(g).min() > 0
    x = c["params"]["edge_logit"].astype(np.float64)
    w = np.where(x > 20, x, np.log1p(np.exp(x))) + 1e-8
    np.testing.assert_allclose(g, 2e-6 * c["reg_lambda"] * w / (1 + np.exp(-x)), rtol=1e-12)
    _, without = R.run_case(c, drop="weight")
    assert not without["edge_logit"].any()


def test_loss_fold_takes_a_second_turn():
    c = RC.loss_fold()
    b = c["u"].shape[0]
    blocks = (b + 15) // 16  # k_triplets: 16 triplets per block, one partial each
    assert blocks == 258 and b % 16 == 5
    nu, ni = c["params"]["user_emb.weight"].shape[0], c["params"]["item_emb.weight"].shape[0]
    assert nu > 256 and nu + ni > 256 and c["params"]["user_emb.weight"].shape[1] == 4 and c["num_layers"] == 1
    # the partials past the 256th carry a visible share of the loss: triplets 4096.. are 21 of 4117
    assert R.references("fold")["ref"][0] * 21 / b > 100 * RC.F * R.references("fold")["yard"]["loss"]


def test_logit_case_mixes_the_branches_inside_rows():
    c = RC.logits()
    cu, ci = c["edge_index"]
    lg = c["params"]["edge_logit"]
    assert set(np.float32(RC.LOGITS)) == set(lg)
    assert (lg[cu == RC.LOGIT_ROW] == -100).all() and (lg[ci == RC.LOGIT_COL] == -100).all()
    assert (cu == RC.LOGIT_ROW).sum() >= 2 and (ci == RC.LOGIT_COL).sum() >= 2
    for r in set(cu) - {RC.LOGIT_ROW}:
        assert len(set(lg[cu == r])) >= 3, r  # several branches meet in one row's sums
    # each side of softplus' threshold, an exp(-x) that overflows fp32, a weight that is 1e-8 alone
    with np.errstate(over="ignore"):
        assert (lg > 20).any() and (lg == 20).any() and (lg < 20).any() and np.isinf(np.exp(-lg)).any()
    ref = R.references("logits")["ref"]
    assert np.isfinite(ref[0]) and all(np.isfinite(g).all() for g in ref[1].values())
    # torch's softplus has the kernel's threshold: above it the value is x itself
    x = torch.tensor([19.999, 20.0, 20.001, 30.0], dtype=torch.float64)
    sp = torch.nn.functional.softplus(x)
    assert sp[0] > x[0] and sp[1] > x[1] and sp[2] == x[2] and sp[3] == x[3]


def test_logits_above_10_show_a_softplus_that_gives_up_early():
    """With w = x in place of log1p(exp(x)) above 10, the edge gradient of this case (2e-6 w sigmoid(x)
    at L = 0) leaves the fp64 one by more than two bounds."""
    c, r = RC.case("logits-above-10"), R.references("logits-above-10")
    x = c["params"]["edge_logit"].astype(np.float64)
    assert c["num_layers"] == 0 and x.min() > 10 and x.max() <= 10.25 and x.size >= 9
    g = r["ref"][1]["edge_logit"]
    early = 2e-6 * c["reg_lambda"] * (x + 1e-8) / (1 + np.exp(-x))
    print(R.measure(early, g), "bound", RC.F * r["yard"]["edge_logit"])
    assert R.measure(early, g) > 2 * RC.F * r["yard"]["edge_logit"]


# ---- the bound -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.CASES))
def test_bound_is_never_looser_than_the_kept_contract(name):
    r = R.references(name)
    for k in R.TENSORS:
        print(name, k, "fp32", r["e32"][k], "reversed", r["e32r"][k], "bound", RC.F * r["yard"][k])
        assert r["yard"][k] >= R.FLOOR and RC.F * r["yard"][k] < KEPT_CONTRACT, k
    assert np.isfinite(r["ref"][0])


ENTERS = {"reg": ("user_emb.weight", "item_emb.weight", "loss"), "delta": ("user_delta", "item_delta", "loss"),
          "weight": ("edge_logit", "loss"), "kd": R.NAMES}


@pytest.mark.parametrize("drop", R.DROPS)
def test_every_loss_term_is_visible(drop):
    """Without the term, the fp64 result leaves the full one by at least 100 bounds in the loss (KD
    excepted) and in the gradient of each parameter the term enters, and by nothing elsewhere."""
    c, r = RC.case(RC.TERMS_CASE), R.references(RC.TERMS_CASE)
    assert c["reg_lambda"] == 1.0 and c["kd_lambda"] == 1.0 and c["teacher"] is not None
    e = R.measures(R.run_case(c, drop=drop), r["ref"])
    for k in R.TENSORS:
        print(drop, k, e[k], "needs", 100 * RC.F * r["yard"][k])
        if k in ENTERS[drop]:
            assert e[k] >= 100 * RC.F * r["yard"][k], k
        elif k != "loss":
            assert e[k] == 0.0, k


def test_driver_scales_share_the_designated_inputs():
    full = RC.case("terms")
    for name, (reg, kd, teacher) in zip(("terms-driver-kd", "terms-driver"), RC.DRIVER_SCALES):
        c = RC.case(name)
        assert (c["reg_lambda"], c["kd_lambda"], c["teacher"] is not None) == (reg, kd, teacher)
        for k in R.NAMES:
            assert np.array_equal(c["params"][k], full["params"][k])
        assert all(np.array_equal(c[k], full[k]) for k in ("edge_index", "u", "pos_i", "neg_i"))
    assert RC.DRIVER_SCALES == ((1e-4, 0.01, True), (1e-4, 0.01, False))


# ---- the reference's additions ---------------------------------------------------------------------------
def test_reverse_is_the_same_function():
    """In fp64 the reversed order moves nothing beyond fp64 rounding; in fp32 it is a second order (it
    changes bits on the ladder case, whose rows are long)."""
    c, r = RC.case("rows-n-d5"), R.references("rows-n-d5")
    e = R.measures(R.run_case(c, reverse=True), r["ref"])
    assert max(e.values()) < 1e-13
    a, b = R.run_case(c, dtype=torch.float32), R.run_case(c, dtype=torch.float32, reverse=True)
    assert any(not np.array_equal(a[1][k], b[1][k]) for k in R.NAMES)
    assert a[1]["edge_logit"].shape == c["params"]["edge_logit"].shape


def test_drop_of_an_absent_term_changes_nothing():
    c = RC.case("terms-driver")  # no teacher
    full, without = R.run_case(c), R.run_case(c, drop="kd")
    assert full[0] == without[0] and all(np.array_equal(full[1][k], without[1][k]) for k in R.NAMES)
    with pytest.raises(ValueError):
        R.run_case(c, drop="bpr")


def test_measure():
    assert R.measure([1.0, 2.0, 4.5], [1.0, 2.0, 4.0]) == 0.125
    assert R.measure([0.0, 1e-3], [0.0, 0.0]) == 1e-3  # identically zero: the absolute maximum
    assert R.measure(np.zeros(0), np.zeros(0)) == 0.0
    assert R.measure(3.0, 4.0) == 0.25


@pytest.mark.parametrize("step", [1, 2, 1000])
def test_adam_step64_against_manual_adam_step(step):
    rng = np.random.default_rng(step)
    p, g = rng.standard_normal(500), rng.standard_normal(500) * 1e-3
    m, v = (0.5 * g, 0.3 * g * g) if step > 1 else (np.zeros(500), np.zeros(500))
    tp = torch.tensor(p, dtype=torch.float64)
    tp.grad = torch.tensor(g, dtype=torch.float64)
    state = {id(tp): {"m": torch.tensor(m), "v": torch.tensor(v)}}
    recsys.manual_adam_step([tp], state, lr=1e-2, step=step)
    p2, m2, v2 = R.adam_step64(p, m, v, g, 1e-2, step)
    np.testing.assert_allclose(p2, tp.numpy(), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(m2, state[id(tp)]["m"].numpy(), rtol=1e-13)
    np.testing.assert_allclose(v2, state[id(tp)]["v"].numpy(), rtol=1e-13)
    assert np.abs(p2 - p).max() > 1e-3  # it moved
