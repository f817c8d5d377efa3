"""The refinement epoch's kernels (csrc/gdd_refine.hip) at the loop turns, widths, layer counts, loss
terms and logit branches that test_gpu_refine.py never reaches, against the fp64 restatement
(tests/refine_ref.py) under a bound worked out per case and per tensor — needs a gfx950 GPU.

The measure is e(x) = max |x - g64| / max |g64| per parameter tensor (the absolute maximum where g64
is identically zero) and |loss - loss64| / |loss64|. A case's yardstick is the largest of e of the
fp32 restatement, e of the fp32 restatement with the edges and triplets reversed, and 2^-23; the device
must stay within F = refine_cases.F yardsticks. That F yardsticks never exceed the earlier 1e-4, and
that every loss term shows by 100 F yardsticks where it enters, is asserted on the host
(test_refine_cases_host.py) together with the properties of the inputs (tests/refine_cases.py):

* rows of 0 .. 200 entries on the user and on the item side (every turn of the 64-entry loops of
  k_spmm, k_degrees and k_degrad, each side of a 16-entry gather batch), d = 5 and d = 8;
* triplet groups of 0 .. 643 entries on both sides (k_seed's turns), shared items, pos == neg, repeats;
* d from 1 to 256 at each side of the per-lane slots, of the 16-lane dot and of d % 4; L from 0 to 8,
  with and without edges; every loss term at weight 1 and at the driver's weights; 258 loss partials;
  logits on each side of softplus' threshold, beyond fp32's exp, rows of vanishing weights;
* gdd_refine_adam_step (k_adam) bit for bit against the fused step, and both against Adam in fp64;
  run() bit for bit against step_with on the sampler's draws; grads() twice.

Each case prints its measures: `pytest -s` shows the ratios behind F."""
import ctypes

import numpy as np
import pytest
import torch

import refine_cases as RC
import refine_ref as R

pytestmark = pytest.mark.gpu

from gdd import _lib, recsys  # noqa: E402

LR = 1e-2


def _model(c):
    p = c["params"]
    nu, d = p["user_emb.weight"].shape
    ni = p["item_emb.weight"].shape[0]
    ei = torch.from_numpy(np.asarray(c["edge_index"], np.int64)).cuda()
    m = recsys.LightGCNCondensed(nu, ni, d, c["num_layers"], ei, torch.ones(ei.shape[1]).cuda(),
                                 device=torch.device("cuda")).cuda()
    with torch.no_grad():
        for k, q in m.named_parameters():
            q.copy_(torch.from_numpy(np.asarray(p[k])))
    return m


def _refiner(c, rng=None, pos=None):
    m = _model(c)
    pos = pos if pos is not None else [np.zeros(1, np.int64)] * m.num_cu
    t = None if c["teacher"] is None else tuple(torch.from_numpy(a).cuda() for a in c["teacher"])
    return recsys.DeviceRefiner(m, pos, lr=LR, reg_lambda=c["reg_lambda"], batch_size=c["u"].shape[0], rng=rng,
                                teacher=t, kd_lambda=c["kd_lambda"])


def _trip(c):
    return c["u"], c["pos_i"], c["neg_i"]


def _grads(c, r=None):
    loss, g = (r or _refiner(c)).grads(*_trip(c))
    return loss, {k: g[k].cpu().numpy() for k in R.NAMES}


def _state(r):
    out = {k: [p.detach().clone()] for k, p in zip(r.NAMES, r.params)}
    for k in r.NAMES:
        out[k] += [t.clone() for t in r.moments[k]]
    return out


def _same_bits(a, b, what=""):
    a, b = (x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x) for x in (a, b))
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, what
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), what


# ---- 1 .. 7: loss and gradients against fp64 -------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.CASES))
def test_case_against_fp64(name):
    c, r = RC.case(name), R.references(name)
    got = _grads(c)
    assert np.isfinite(got[0]) and all(np.isfinite(g).all() for g in got[1].values())
    e = R.measures(got, r["ref"])
    for k in R.TENSORS:
        print(f"RATIO {RC.FAMILY_OF[name]} {name} {k} e={e[k]:.3e} yard={r['yard'][k]:.3e} "
              f"ratio={e[k] / r['yard'][k]:.3f}")
    for k in R.TENSORS:
        assert e[k] <= RC.F * r["yard"][k], (k, e[k], r["yard"][k])


@pytest.mark.parametrize("drop", R.DROPS)
def test_device_has_every_loss_term(drop):
    """The device's result at the designated case lies 99 bounds or more from the fp64 result without
    the term, in the loss (KD excepted) and in each gradient the term enters."""
    c, r = RC.case(RC.TERMS_CASE), R.references(RC.TERMS_CASE)
    loss, g = _grads(c)
    w_loss, w_g = R.run_case(c, drop=drop)
    enters = {"reg": ("user_emb.weight", "item_emb.weight"), "delta": ("user_delta", "item_delta"),
              "weight": ("edge_logit",), "kd": R.NAMES}[drop]
    for k in enters:
        dist = np.abs(g[k] - w_g[k]).max() / np.abs(r["ref"][1][k]).max()
        print(drop, k, dist, "bound", RC.F * r["yard"][k])
        assert dist >= 99 * RC.F * r["yard"][k], k
    if drop != "kd":
        assert abs(loss - w_loss) / abs(r["ref"][0]) >= 99 * RC.F * r["yard"]["loss"]


# ---- 8. Adam -------------------------------------------------------------------------------------------
def _adam_step_through_lib(r, g, step):
    _lib.check(r.lib.gdd_refine_adam_step(ctypes.addressof(r._problem), *(g[k].data_ptr() for k in r.NAMES),
                                          ctypes.addressof(r._adam), step, _lib.stream_ptr(r.dev)))
    r.step = step


@pytest.mark.parametrize("step,no_edges", [(1, False), (2, False), (1000, False), (1, True), (2, True), (1000, True)])
def test_adam_step_kernel_bit_for_bit(step, no_edges):
    """grads() then gdd_refine_adam_step (k_adam) leaves the bits of step_with (k_final's fused Adam) in
    every parameter and moment; both sit within |dp| <= 1e-6 lr + 2^-23 |p| and rtol 1e-6 on the moments
    (test_gpu_refine.py's bound) of Adam in fp64 from the same state and the device's gradients."""
    c = RC.adam(no_edges)
    assert (c["edge_index"].shape[1] == 0) == no_edges
    split, fused = _refiner(c), _refiner(c)
    if step == 2:
        for r in (split, fused):
            r.step_with(*_trip(c))
    elif step > 1:  # moments as after many steps on this gradient (same signs: no cancellation in m)
        _, g0 = split.grads(*_trip(c))
        for r in (split, fused):
            for k in r.NAMES:
                r.moments[k][0].copy_(0.5 * g0[k])
                r.moments[k][1].copy_(0.3 * g0[k] * g0[k])
            r.step = step - 1
    before = _state(split)
    for k in split.NAMES:
        for a, b in zip(before[k], _state(fused)[k]):
            assert torch.equal(a, b)
    loss, g = split.grads(*_trip(c))
    _adam_step_through_lib(split, g, step)
    loss_fused = fused.step_with(*_trip(c))
    assert fused.step == step and np.float32(loss).view(np.uint32) == np.float32(loss_fused).view(np.uint32)
    after, after_fused = _state(split), _state(fused)
    for k in split.NAMES:
        for a, b, what in zip(after[k], after_fused[k], "pmv"):
            _same_bits(a, b, f"{what} of {k}")
        p0, m0, v0 = (t.cpu().numpy() for t in before[k])
        p64, m64, v64 = R.adam_step64(p0, m0, v0, g[k].cpu().numpy(), LR, step)
        p, m, v = (t.cpu().numpy().astype(np.float64) for t in after[k])
        np.testing.assert_allclose(m, m64, rtol=1e-6, atol=2.0 ** -126, err_msg=f"m of {k}")
        np.testing.assert_allclose(v, v64, rtol=1e-6, atol=2.0 ** -126, err_msg=f"v of {k}")
        if p.size:
            bound = 1e-6 * LR + 2.0 ** -23 * np.abs(p64)
            print(k, "max |dp| over its bound:", float((np.abs(p - p64) / bound).max()))
            assert (np.abs(p - p64) <= bound).all(), k
            assert not np.array_equal(p, p0.astype(np.float64)), k  # it moved


# ---- 9. the loop ---------------------------------------------------------------------------------------
def test_run_is_step_with_on_the_samplers_draws():
    c = RC.adam()
    cu, ci = c["edge_index"]
    nu, ni = c["params"]["user_emb.weight"].shape[0], c["params"]["item_emb.weight"].shape[0]
    pos = [ci[cu == r] for r in range(nu)]
    b = c["u"].shape[0]
    loop = _refiner(c, rng=np.random.RandomState(11), pos=pos)
    losses = loop.run(5)
    steps, twin = _refiner(c, pos=pos), np.random.RandomState(11)
    one_by_one = []
    for _ in range(5):
        one_by_one.append(steps.step_with(*recsys.sample_bpr_triplets_from_condensed(pos, ni, b, twin)))
    assert loop.step == steps.step == 5 and losses.dtype == np.float32
    _same_bits(losses, np.asarray(one_by_one, np.float32), "losses")
    assert len(set(losses.tolist())) == 5  # the parameters move, the batches differ
    a, s = _state(loop), _state(steps)
    for k in loop.NAMES:
        for x, y, what in zip(a[k], s[k], "pmv"):
            _same_bits(x, y, f"{what} of {k}")
    for x, y in zip(loop.rng.get_state(), twin.get_state()):
        assert np.array_equal(x, y)


# ---- 10. determinism -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(RC.FAMILIES["rows"]) + list(RC.FAMILIES["groups"]))
def test_grads_twice_same_bits(name):
    c = RC.case(name)
    r = _refiner(c)
    runs = [_grads(c, r), _grads(c, r), _grads(c)]  # the same workspace again, and a fresh one
    for other in runs[1:]:
        assert np.float32(runs[0][0]).view(np.uint32) == np.float32(other[0]).view(np.uint32)
        for k in R.NAMES:
            _same_bits(runs[0][1][k], other[1][k], k)
