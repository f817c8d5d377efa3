"""The order-free fixed-point M-step on the device (gdd_lloyd_reduce_*, ShardedKMeans(mstep="reduce")):
the kernels' int64 buffers against the numpy restatement (tests/reduce_util) as exact integers, the
update front end's fp32 bits, a whole one-rank fit against the CPU restatement bit for bit, and worlds
2 and 3 (processes sharing cuda:0 over gloo) against world 1 bit for bit."""
import functools
import os
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from gdd import _lib, synth  # noqa: E402
from gdd.sharded import ShardedKMeans  # noqa: E402
from reduce_util import ReduceOps, reduce_exponents, reduce_local, reduce_sums32  # noqa: E402
from sharded_util import OracleOps, free_port  # noqa: E402

DEV = "cuda:0"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _nearest(X, k, rng):
    C = X[rng.choice(X.shape[0], k, replace=False)].astype(np.float64)
    d = (X.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * X.astype(np.float64) @ C.T + (C ** 2).sum(1)[None]
    return d.argmin(1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(X, [labels of a nearest-centre pass, a random labelling], k)."""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "columns":  # an all-zero column, one scaled by 1e30, one by 1e-30, mixed signs
        n, dim, k = 2000, 6, 7
        X = rng.standard_normal((n, dim)).astype(np.float32)
        X[:, 0] = 0.0
        X[:, 1] *= np.float32(1e30)
        X[:, 2] *= np.float32(1e-30)
        X[:, 3] = np.abs(X[:, 3]) * np.where(np.arange(n) % 3 == 0, -1.0, 1.0).astype(np.float32)
        labs = [_nearest(X[:, 3:], k, rng), rng.integers(0, k, n).astype(np.int32)]
        return X, labs, k
    n, dim, k = map(int, name.split("x"))
    X = (synth.blobs(n, dim, max(1, min(k, 16)), seed=n + dim) - np.float32(0.25)).astype(np.float32)
    return X, [_nearest(X, k, rng), rng.integers(0, k, n).astype(np.int32)], k


def _splits(n, parts, rng):
    """`parts` uneven row ranges covering [0, n), one of them empty."""
    cuts = np.sort(rng.choice(np.arange(1, n), parts - 2, replace=False)) if parts > 2 else np.zeros(0, np.int64)
    cuts = np.concatenate([[0], cuts, [n]]).astype(np.int64)
    at = int(rng.integers(0, len(cuts)))
    cuts = np.insert(cuts, at, cuts[at])  # r0 == r1
    return list(zip(cuts[:-1].tolist(), cuts[1:].tolist()))


class _Dev:
    def __init__(self, X, k):
        self.lib = _lib.device_lib()
        self.n, self.dim = X.shape
        self.k = k
        self.X = torch.from_numpy(X).to(DEV)
        self.words = self.lib.gdd_lloyd_reduce_words(self.dim, k)
        assert self.words == k * self.dim + k + 1
        self.ws = _lib.workspace(self.lib.gdd_lloyd_reduce_ws_bytes(self.n, self.dim, k), DEV)
        self.exps = torch.full((self.dim,), 77, dtype=torch.int32, device=DEV)
        self.state = torch.zeros(self.lib.gdd_lloyd_state_bytes(), dtype=torch.uint8, device=DEV)
        _lib.check(self.lib.gdd_lloyd_reduce_exponents(self.n, self.dim, self.X.data_ptr(),
                                                       self.exps.data_ptr(), _lib.stream_ptr(self.X.device)))

    def local(self, labels, labels_old, r0, r1, it=0):
        buf = torch.full((self.words,), 0x5a5a5a5a, dtype=torch.int64, device=DEV)  # the call zeroes it
        _lib.check(self.lib.gdd_lloyd_reduce_local(self.n, r0, r1, self.dim, self.X.data_ptr(),
                                                   labels.data_ptr(), labels_old.data_ptr(), self.k,
                                                   self.exps.data_ptr(), buf.data_ptr(), self.state.data_ptr(),
                                                   it, self.ws.data_ptr(), self.ws.numel(),
                                                   _lib.stream_ptr(self.X.device)))
        return buf


@pytest.mark.parametrize("name", ["3001x8x12", "4099x47x33", "4099x100x20", "20000x24x3", "65x5x64",
                                  "500x6x1", "4096x7x5", "4097x7x5", "columns"])
def test_local_phase_is_exact(name):
    """The local phase's int64 buffer over [0, n) equals the restatement as integers, and so does the
    sum of the buffers of 2, 3 and 7 uneven row splits (one of them empty); the changed count and the
    labels_old update too. dims 47 and 100 are no multiple of 4 or 64, 20000x24x3 has clusters far
    larger than a tile, 65x5x64 nearly only singletons and empty clusters, 4096 / 4097 straddle L."""
    X, labs, k = _case(name)
    n, dim = X.shape
    d = _Dev(X, k)
    exps = reduce_exponents(X)
    assert np.array_equal(d.exps.cpu().numpy(), exps)
    rng = np.random.default_rng(5)
    for lab in labs:
        old = lab.copy()
        flip = rng.random(n) < 0.3
        old[flip] = -1
        want = reduce_local(X, lab, old.copy(), k, exps, 0, n)
        assert want[-1] == np.count_nonzero(flip)
        lab_d = torch.from_numpy(lab).to(DEV)
        old_d = torch.from_numpy(old).to(DEV)
        got = d.local(lab_d, old_d, 0, n).cpu().numpy()
        assert np.array_equal(got, want)
        assert np.array_equal(old_d.cpu().numpy(), lab)
        for parts in (2, 3, 7):
            if n < parts:
                continue
            old_d = torch.from_numpy(old).to(DEV)
            total = torch.zeros(d.words, dtype=torch.int64, device=DEV)
            for r0, r1 in _splits(n, parts, rng):
                before = old_d.clone()
                total += d.local(lab_d, old_d, r0, r1)
                after = old_d.cpu().numpy()
                assert np.array_equal(after[:r0], before.cpu().numpy()[:r0])  # only its own rows
                assert np.array_equal(after[r1:], before.cpu().numpy()[r1:])
            assert np.array_equal(total.cpu().numpy(), want), parts
            assert np.array_equal(old_d.cpu().numpy(), lab)


def test_local_phase_is_gated_but_still_zeroes():
    X, labs, k = _case("3001x8x12")
    d = _Dev(X, k)
    d.state.view(torch.int32)[0] = 2  # iteration 0 converged (stop_at = 2*0 + 2): iteration 1's local phase, step 2, is past it
    lab_d = torch.from_numpy(labs[0]).to(DEV)
    old_d = torch.full_like(lab_d, -1)
    got = d.local(lab_d, old_d, 0, X.shape[0], it=1).cpu().numpy()
    assert not got.any()
    assert (old_d.cpu().numpy() == -1).all()


def _update(lib, buf, exps, k, dim, C_old, it, changed0=0, from_cnew=False, C_new=None, wsum=None):
    st = torch.zeros(lib.gdd_lloyd_state_bytes() // 4, dtype=torch.int32, device=DEV)
    st[3] = changed0
    C_new = torch.full((k, dim), 7.0, device=DEV) if C_new is None else torch.from_numpy(C_new).to(DEV)
    wsum = torch.full((k,), -1.0, device=DEV) if wsum is None else torch.from_numpy(wsum).to(DEV)
    shift = torch.zeros(k, device=DEV)
    b = torch.from_numpy(buf).to(DEV)
    e = torch.from_numpy(exps).to(DEV)
    co = torch.from_numpy(C_old).to(DEV)
    _lib.check(lib.gdd_lloyd_reduce_update(dim, k, b.data_ptr(), e.data_ptr(), int(from_cnew), C_new.data_ptr(),
                                           wsum.data_ptr(), co.data_ptr(), shift.data_ptr(), 0.0,
                                           st.data_ptr(), it, _lib.stream_ptr(b.device)))
    return C_new.cpu().numpy(), wsum.cpu().numpy(), shift.cpu().numpy(), st.cpu().numpy()


@pytest.mark.parametrize("k,dim", [(33, 47), (5, 100), (300, 3)])
def test_update_front_end_bits(k, dim):
    """fp32 sums and weights from a reduced buffer equal the restatement's bits (sums up to 2^62 that
    round, exponents of either sign, a count past 2^24); without an empty cluster the averaging and
    the convergence step follow; a count-0 cluster stops at this step with reason 3, the sums left in
    C_new and the changed flag in the state; from_cnew averages what C_new holds."""
    lib = _lib.device_lib()
    rng = np.random.default_rng(k)
    exps = rng.integers(-20, 100, dim).astype(np.int32)
    buf = np.zeros(k * dim + k + 1, np.int64)
    buf[:k * dim] = rng.integers(-(1 << 62), 1 << 62, k * dim, dtype=np.int64) >> rng.integers(0, 60, k * dim)
    buf[k * dim:k * dim + k] = rng.integers(1, 1000, k)
    buf[k * dim] = (1 << 24) + 3
    buf[-1] = 5
    C_old = rng.standard_normal((k, dim)).astype(np.float32)
    sums, w = reduce_sums32(buf, k, dim, exps)
    it = 4
    cn, ws, sh, st = _update(lib, buf, exps, k, dim, C_old, it)
    assert np.array_equal(_bits(ws), _bits(w)) and ws[0] == np.float32((1 << 24) + 3)
    want_c, want_s = OracleOps().average(torch.from_numpy(sums), torch.from_numpy(w), torch.from_numpy(C_old))
    assert np.array_equal(_bits(cn), _bits(want_c.numpy()))
    assert np.array_equal(_bits(sh), _bits(want_s.numpy()))
    assert st[0] == 0 and st[3] == 0 and st[4] == it + 1  # changed, shift^2 > tol 0: goes on
    # no label changed: strict convergence
    buf0 = buf.copy()
    buf0[-1] = 0
    st = _update(lib, buf0, exps, k, dim, C_old, it)[3]
    assert (st[0], st[1], st[2], st[4]) == (2 * it + 2, 1, it, it + 1)
    # an empty cluster
    if k > 2:
        bufe = buf.copy()
        bufe[k * dim + k - 2] = 0
        cn, ws, sh, st = _update(lib, bufe, exps, k, dim, C_old, it)
        we = w.copy()
        we[k - 2] = 0
        assert np.array_equal(_bits(cn), _bits(sums)) and np.array_equal(_bits(ws), _bits(we))
        assert (st[0], st[1], st[2], st[3]) == (2 * it + 1, 3, it, 1)
        assert not sh.any()
        # the resume: the (relocated) sums are in C_new, buf is stale
        w2 = we.copy()
        w2[k - 2] = 1
        junk = np.full_like(buf, -1)
        cn, ws, sh, st = _update(lib, junk, exps, k, dim, C_old, it, changed0=1, from_cnew=True, C_new=sums, wsum=w2)
        want_c, want_s = OracleOps().average(torch.from_numpy(sums), torch.from_numpy(w2), torch.from_numpy(C_old))
        assert np.array_equal(_bits(cn), _bits(want_c.numpy())) and np.array_equal(_bits(ws), _bits(w2))
        assert np.array_equal(_bits(sh), _bits(want_s.numpy()))
        assert st[0] == 0 and st[3] == 0 and st[4] == it + 1


def _dup_blobs(n, dim, k):
    X = synth.blobs(n, dim, max(1, k // 3), seed=n)
    X[1::7] = X[0]
    return X


def _res(m):
    return dict(labels=m.labels_, centers=m.cluster_centers_, n_iter=m.n_iter_, inertia=m.inertia_)


def _same(a, b):
    assert int(a["n_iter"]) == int(b["n_iter"])
    assert np.array_equal(a["labels"], b["labels"])
    assert np.array_equal(_bits(a["centers"]), _bits(b["centers"]))
    assert float(a["inertia"]) == float(b["inertia"])


@pytest.mark.parametrize("n,dim,k", [(3001, 8, 12), (4099, 47, 33), (50, 4, 50)])
def test_one_rank_fit_equals_cpu_restatement(n, dim, k):
    """(50, 4, 50): empty clusters, so the reason-3 stop, the relocation and the resume run."""
    X = _dup_blobs(n, dim, k)
    dev = ShardedKMeans(n_clusters=k, random_state=7, device=DEV, mstep="reduce").fit(X)
    cpu = ShardedKMeans(n_clusters=k, random_state=7, ops=ReduceOps(), mstep="reduce").fit(X)
    assert dev.mode_ == cpu.mode_ == "reduce"
    _same(_res(dev), _res(cpu))


def _world_inputs():
    X = synth.blobs(20000, 24, 40, seed=4)
    X[1::9] = X[0]
    n, dim = 100003, 47  # >= 65,536 rows at dim 47: the E-step's padded-X path
    rng = np.random.default_rng(8)
    Xp = (rng.standard_normal((n, 32)) @ rng.standard_normal((32, dim)) / 5.0 + rng.standard_normal(dim)).astype(np.float32)
    return X, Xp


def _world_fits(group):
    X, Xp = _world_inputs()
    np.random.seed(15)
    a = ShardedKMeans(n_clusters=40, device=DEV, group=group, mstep="reduce").fit(X)
    b = ShardedKMeans(n_clusters=60, random_state=15, device=DEV, group=group, mstep="reduce").fit(Xp)
    assert a.mode_ == b.mode_ == "reduce"
    out = {"a_" + key: v for key, v in _res(a).items()}
    out.update({"b_" + key: v for key, v in _res(b).items()})
    return out


@functools.lru_cache(maxsize=None)
def _world_one():
    return _world_fits(None)


def _world_worker(rank, world, port, out):
    sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(HERE),
                                                          "graph-distillation-for-recommendation_amd"), HERE]
    import torch.distributed as dist
    from sharded_util import init_gloo
    init_gloo(rank, world, port)
    np.savez(os.path.join(out, f"w{rank}.npz"), **_world_fits(dist.group.WORLD))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_worlds_match_one_rank(world):
    one = _world_one()
    out = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"gdd_reduce_{os.getpid()}_{world}")
    os.makedirs(out, exist_ok=True)
    mp.spawn(_world_worker, args=(world, free_port(), out), nprocs=world, join=True)
    for r in range(world):
        p = np.load(os.path.join(out, f"w{r}.npz"))
        for tag in ("a_", "b_"):
            _same({key: p[tag + key] for key in ("labels", "centers", "n_iter", "inertia")},
                  {key: one[tag + key] for key in ("labels", "centers", "n_iter", "inertia")})


def test_pipeline_routes_reduce_on_one_rank():
    from gdd.pipeline import _lloyd
    X = _dup_blobs(3001, 8, 12)
    km = _lloyd(12, None, mstep="reduce", random_state=7, device=DEV).fit(X)
    assert isinstance(km, ShardedKMeans) and km.mode_ == "reduce"
    _same(_res(km), _res(ShardedKMeans(n_clusters=12, random_state=7, device=DEV, mstep="reduce").fit(X)))
    assert not isinstance(_lloyd(12, None, random_state=7, device=DEV), ShardedKMeans)
