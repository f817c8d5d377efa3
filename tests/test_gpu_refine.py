"""The refinement loop on the device (gdd.recsys.DeviceRefiner over gdd_refine.hip): one epoch as a
fixed chain of launches with every sum in a fixed order.

* gradients against the reference's own (G8, golden_recsys.npz) at the tolerances the eager path is held
  to, and against an fp64 restatement (tests/refine_ref.py) on shapes that cross every edge of the
  kernels: one row, d of 1 / not a multiple of 64 / 256, L = 0..3, no edges, empty and full rows,
  batches far larger than the tables, with and without the KD term;
* Adam against manual_adam_step; the same bits from two runs; chunking and the sampler's state;
* the driver with ``--refine_backend device`` under the assertions of the two driver tests of
  tests/test_gpu_recsys.py; the guards.
"""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import refine_ref
import test_gpu_recsys as T
from golden_util import load

pytestmark = pytest.mark.gpu

from gdd import recsys  # noqa: E402

GRAD_RTOL, GRAD_ATOL = 1e-4, 1e-7  # tests/test_gpu_recsys.py:77-85
REG, KD, LR = 1e-4, 0.01, 1e-2


def _model(params, edge_index, num_layers):
    nu, d = params["user_emb.weight"].shape
    ni = params["item_emb.weight"].shape[0]
    ei = torch.from_numpy(np.asarray(edge_index, np.int64)).cuda()
    m = recsys.LightGCNCondensed(nu, ni, d, num_layers, ei, torch.ones(ei.shape[1]).cuda(),
                                 device=torch.device("cuda")).cuda()
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(torch.from_numpy(np.asarray(params[k])))
    return m


def _refiner(m, batch, teacher=None, rng=None, pos=None, **kw):
    pos = pos if pos is not None else [np.zeros(1, np.int64)] * m.num_cu
    t = None if teacher is None else tuple(torch.from_numpy(a).cuda() for a in teacher)
    return recsys.DeviceRefiner(m, pos, lr=LR, reg_lambda=REG, batch_size=batch, rng=rng, teacher=t,
                                kd_lambda=KD, **kw)


def _assert_grads(got, want, who):
    for k in refine_ref.NAMES:
        g = got[k].detach().cpu().numpy() if isinstance(got[k], torch.Tensor) else got[k]
        np.testing.assert_allclose(g, want[k], rtol=GRAD_RTOL, atol=GRAD_ATOL, err_msg=f"{who}: {k}")


# ---- 1. the reference's own gradients -----------------------------------------------------------------
def _golden_params(z):
    return {k: z["param_" + k.replace(".", "_")] for k in refine_ref.NAMES}


def test_grads_vs_reference():
    z = load("golden_recsys.npz")
    m = _model(_golden_params(z), z["edge_index"], int(z["layers"]))
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    loss, g = _refiner(m, int(z["bpr_u"].shape[0])).grads(z["bpr_u"], z["bpr_pos"], z["bpr_neg"])
    print("loss", loss, "reference", float(z["loss"]))
    assert abs(loss - float(z["loss"])) <= 1e-6
    _assert_grads(g, {k: z["grad_" + k.replace(".", "_")] for k in refine_ref.NAMES}, "device")
    for k, p in m.named_parameters():
        assert torch.equal(p, before[k]), k  # grads() updates nothing


# ---- 2. the edges, against fp64 -------------------------------------------------------------------------
CASES = [(1, 1, 1, 0, 1), (5, 3, 3, 1, 7), (37, 23, 20, 1, 300), (64, 65, 64, 2, 257), (130, 70, 256, 3, 1000)]


@functools.lru_cache(maxsize=None)
def _case(shape, kd):
    c = refine_ref.edge_case(*shape, seed=1, no_edges=shape == CASES[0])
    teacher = c["teacher"] if kd else None
    ref = refine_ref.loss_and_grads(c["params"], c["edge_index"], c["num_layers"], c["u"], c["pos_i"], c["neg_i"],
                                    REG, teacher, KD)
    return c, teacher, ref


@pytest.mark.parametrize("kd", [False, True])
@pytest.mark.parametrize("shape", CASES)
def test_grads_at_the_edges(shape, kd):
    c, teacher, (ref_loss, ref_g) = _case(shape, kd)
    nu, ni = shape[0], shape[1]
    cu, ci = c["edge_index"]
    if shape == CASES[0]:
        assert cu.size == 0
    else:  # a full row (up to the empty column), an empty row, an empty column
        counts = np.bincount(cu, minlength=nu)
        assert counts[0] == ni - 1 and counts[-1] == 0 and np.bincount(ci, minlength=ni)[-1] == 0
    u, pos, neg = (torch.from_numpy(c[k]).cuda() for k in ("u", "pos_i", "neg_i"))
    # the input is fair: the eager path meets the tolerance on it
    m = _model(c["params"], c["edge_index"], c["num_layers"])
    loss = m.bpr_loss(u, pos, neg, reg_lambda=REG)
    if kd:
        su, si = m.propagate()
        loss = loss + KD * (F.mse_loss(su, torch.from_numpy(teacher[0]).cuda())
                            + F.mse_loss(si, torch.from_numpy(teacher[1]).cuda()))
    loss.backward()
    print("eager loss", loss.item(), "fp64", ref_loss)
    assert abs(loss.item() - ref_loss) <= 1e-6
    _assert_grads({k: p.grad for k, p in m.named_parameters()}, ref_g, "eager")
    # the device chain
    m2 = _model(c["params"], c["edge_index"], c["num_layers"])
    got_loss, got = _refiner(m2, shape[4], teacher).grads(c["u"], c["pos_i"], c["neg_i"])
    print("device loss", got_loss)
    assert abs(got_loss - ref_loss) <= 1e-6
    _assert_grads(got, ref_g, "device")


# ---- 3. Adam ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 1000])
def test_adam_vs_manual_adam_step(step):
    """step_with and manual_adam_step from the same parameters, moments and gradients. Both apply about
    ten fp32 roundings of 2^-24 to the update, whose size is about lr: p within 1e-6 lr + 2^-23 |p|, the
    moments within rtol 1e-6 (below the smallest normal fp32 a value carries fewer bits: atol 2^-126)."""
    c, teacher, _ = _case(CASES[3], True)
    trip = (c["u"], c["pos_i"], c["neg_i"])
    m_dev, m_ref = (_model(c["params"], c["edge_index"], c["num_layers"]) for _ in range(2))
    r = _refiner(m_dev, CASES[3][4], teacher)
    _, g = r.grads(*trip)
    state = {}
    named = dict(m_ref.named_parameters())
    if step > 1:  # moments as after many steps on this gradient (same signs: no cancellation in m)
        for k in r.NAMES:
            m0, v0 = 0.5 * g[k], 0.3 * g[k] * g[k]
            r.moments[k][0].copy_(m0)
            r.moments[k][1].copy_(v0)
            state[id(named[k])] = {"m": m0.clone(), "v": v0.clone()}
        r.step = step - 1
    for k in r.NAMES:
        named[k].grad = g[k].clone()
    recsys.manual_adam_step(list(named.values()), state, lr=LR, step=step)
    r.step_with(*trip)
    assert r.step == step
    dev = dict(m_dev.named_parameters())
    for k in r.NAMES:
        for got, want, what in zip(r.moments[k], (state[id(named[k])]["m"], state[id(named[k])]["v"]), "mv"):
            np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=1e-6, atol=2.0 ** -126,
                                       err_msg=f"{what} of {k}")
        p, q = dev[k].detach().cpu().numpy().astype(np.float64), named[k].detach().cpu().numpy().astype(np.float64)
        excess = np.abs(p - q) - (1e-6 * LR + 2.0 ** -23 * np.abs(q))
        print(k, "max |dp| over its bound:", float((np.abs(p - q) / (1e-6 * LR + 2.0 ** -23 * np.abs(q))).max()))
        assert excess.max() <= 0, k
        assert not np.array_equal(p, np.asarray(c["params"][k], np.float64)), k  # it moved


# ---- 4 and 5. determinism, chunking, the sampler -------------------------------------------------------------
def _golden_setup(seed=7, batch=256):
    z = load("golden_recsys.npz")
    m = _model(_golden_params(z), z["edge_index"], int(z["layers"]))
    nu, ni = int(z["num_cu"]), int(z["num_ci"])
    C = sp.csr_matrix((z["C_data"], z["C_indices"], z["C_indptr"]), shape=(nu, ni))
    pos = recsys._csr_row_to_set_list(C)
    rng = np.random.RandomState(seed)
    tr = np.random.default_rng(3)
    teacher = (0.1 * tr.standard_normal((nu, m.dim)).astype(np.float32),
               0.1 * tr.standard_normal((ni, m.dim)).astype(np.float32))
    return m, pos, rng, _refiner(m, batch, teacher, rng=rng, pos=pos), ni


def _state_of(r):
    out = [p.detach().clone() for p in r.params]
    for k in r.NAMES:
        out += [t.clone() for t in r.moments[k]]
    return out


def test_same_bits_twice():
    runs = []
    for _ in range(2):
        m, pos, rng, r, _ = _golden_setup()
        losses = r.run(10)
        assert losses.shape == (10,) and np.isfinite(losses).all() and r.step == 10
        runs.append((losses, _state_of(r)))
    assert np.array_equal(runs[0][0].view(np.uint32), runs[1][0].view(np.uint32))
    for a, b in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a, b)
    assert len(set(runs[0][0].tolist())) > 1  # the epochs differ: the parameters move


def test_chunking_and_sampler_state():
    m, pos, rng, r, ni = _golden_setup()
    whole = r.run(10)
    m2, pos2, rng2, r2, _ = _golden_setup()
    parts = np.concatenate([r2.run(3), r2.run(7)])
    assert np.array_equal(whole.view(np.uint32), parts.view(np.uint32))
    for a, b in zip(_state_of(r), _state_of(r2)):
        assert torch.equal(a, b)
    ref_rng = np.random.RandomState(7)
    for _ in range(10):
        recsys.sample_bpr_triplets_from_condensed(pos, ni, 256, ref_rng)
    for a, b in zip(rng.get_state(), ref_rng.get_state()):
        assert np.array_equal(a, b)
    for a, b in zip(rng2.get_state(), ref_rng.get_state()):
        assert np.array_equal(a, b)


# ---- 6. the driver ---------------------------------------------------------------------------------------------
def _device_backend(monkeypatch):
    """The driver's parsed arguments with --refine_backend device; counts DeviceRefiner.run calls."""
    from gdd import distill_recsys as D
    parse, run, calls = D.parse_args, recsys.DeviceRefiner.run, []

    def parse_device(argv=None):
        return parse(list(argv) + ["--refine_backend", "device"])

    def counted(self, n):
        calls.append(n)
        return run(self, n)
    monkeypatch.setattr(D, "parse_args", parse_device)
    monkeypatch.setattr(recsys.DeviceRefiner, "run", counted)
    return calls


def test_driver_device_backend_vs_reference(tmp_path, capsys, monkeypatch):
    calls = _device_backend(monkeypatch)
    T.test_distill_recsys_driver_vs_reference(tmp_path, capsys, monkeypatch)
    assert calls and calls[0] == 1  # epoch 1 is logged on its own


def test_driver_device_backend_real_alidisplay_vs_reference(tmp_path, capsys, monkeypatch):
    """The shape at which the r03 graph capture faulted (1,773 x 1,004 clusters, 51,539 edges, d = 64,
    4,096 triplets)."""
    calls = _device_backend(monkeypatch)
    T.test_distill_recsys_real_alidisplay_vs_reference(tmp_path, capsys, monkeypatch)
    assert calls and calls[0] == 1


# ---- 7. guards ---------------------------------------------------------------------------------------------------
def test_guards():
    c, teacher, _ = _case(CASES[2], False)
    nu, ni, d, L, b = CASES[2]
    m = _model(c["params"], c["edge_index"], L)
    r = _refiner(m, b)
    for which, bound in (("u", nu), ("pos_i", ni), ("neg_i", ni)):
        trip = {k: c[k].copy() for k in ("u", "pos_i", "neg_i")}
        trip[which][5] = bound
        with pytest.raises(IndexError):
            r.grads(trip["u"], trip["pos_i"], trip["neg_i"])
        with pytest.raises(IndexError):
            r.step_with(trip["u"], trip["pos_i"], trip["neg_i"])
    assert r.step == 0
    loss, _ = r.grads(c["u"], c["pos_i"], c["neg_i"])  # the next call still works
    assert np.isfinite(loss) and np.isfinite(r.step_with(c["u"], c["pos_i"], c["neg_i"])) and r.step == 1
    with pytest.raises(ValueError, match="torch backend"):
        wide = {k: (np.zeros((v.shape[0], 257), np.float32) if v.ndim == 2 else v) for k, v in c["params"].items()}
        _refiner(_model(wide, c["edge_index"], L), b)
    with pytest.raises(ValueError, match="teacher"):
        _refiner(m, b, (c["teacher"][0][:-1], c["teacher"][1]))
    with pytest.raises(ValueError, match="teacher"):
        _refiner(m, b, (c["teacher"][0], c["teacher"][1][:, :-1]))
