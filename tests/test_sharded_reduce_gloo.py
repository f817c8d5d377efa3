"""gdd.sharded.ShardedKMeans(mstep="reduce") on the CPU (gloo, no GPU): the order-free fixed-point
M-step's distributed logic with the numpy restatement of the device phases (tests/reduce_util.ReduceOps)
and the oracle's other primitives.

Two properties: worlds 1 - 4 are byte-identical (integer partial sums are exact and associative), and
the mode's contract against scikit-learn / the oracle's ordered Lloyd (SURVEY §7 hard part 1): labels
and n_iter_ equal, ARI >= 0.999, inertia within 1e-4 relative.
"""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _paths():
    for p in (ROOT, os.path.join(ROOT, "graph-distillation-for-recommendation_amd"), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)


def _fit(X, k, n_init, seed, **kw):
    from gdd import sharded
    from reduce_util import ReduceOps
    if seed is None:
        np.random.seed(15)
    m = sharded.ShardedKMeans(n_clusters=k, n_init=n_init, random_state=seed, ops=ReduceOps(), **kw).fit(X)
    return m, dict(labels=m.labels_, centers=m.cluster_centers_, n_iter=m.n_iter_, inertia=m.inertia_)


def _worker(rank, world, port, X, k, n_init, seed, out_dir):
    _paths()
    import torch.distributed as dist
    from sharded_util import init_gloo
    init_gloo(rank, world, port)
    m, res = _fit(X, k, n_init, seed, mstep="reduce")
    assert m.mode_ == "reduce"
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), **res)
    dist.destroy_process_group()


def _run(world, X, k, n_init, seed, tmp):
    from sharded_util import free_port
    os.makedirs(tmp, exist_ok=True)
    mp.spawn(_worker, args=(world, free_port(), X, k, n_init, seed, str(tmp)), nprocs=world, join=True)
    parts = [dict(np.load(os.path.join(tmp, f"r{r}.npz"))) for r in range(world)]
    for p in parts[1:]:  # every rank ends with the same result
        _same(p, parts[0])
    return parts[0]


def _same(a, b):
    assert a.keys() == b.keys()
    for key in a:
        assert np.array_equal(np.atleast_1d(a[key]).view(np.uint8), np.atleast_1d(b[key]).view(np.uint8)), key


def _ari(a, b):
    """Adjusted Rand index from the contingency table."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    ct = np.zeros((a.max() + 1, b.max() + 1), np.float64)
    np.add.at(ct, (a, b), 1.0)
    comb = lambda x: x * (x - 1.0) / 2.0  # noqa: E731
    s, sa, sb, tot = comb(ct).sum(), comb(ct.sum(1)).sum(), comb(ct.sum(0)).sum(), comb(float(a.shape[0]))
    exp = sa * sb / tot
    mx = 0.5 * (sa + sb)
    return 1.0 if mx == exp else (s - exp) / (mx - exp)


def _contract(X, res, ref_labels, ref_n_iter, ref_inertia, ref_centers, inertia=True):
    assert int(res["n_iter"]) == int(ref_n_iter)
    assert np.array_equal(res["labels"], ref_labels)
    assert _ari(res["labels"], ref_labels) >= 0.999
    if inertia:
        assert abs(float(res["inertia"]) - float(ref_inertia)) <= 1e-4 * abs(float(ref_inertia))
    # Not the ordered sums' bits. The reference's fp32 chain over a cluster's m members is within
    # (m - 1) * 2^-24 * sum|x| of the exact sum, so its mean is within (m - 1) * 2^-24 * max|Xc|; the
    # fixed-point sum is exact (quantisation below 2^-38 relative) and rounds once, the division once,
    # and adding the column mean back once more on either side: (m + 3) * 2^-24 of the largest entry.
    m_max = int(np.bincount(np.asarray(ref_labels, np.int64)).max())
    scale = max(float(np.abs(X - X.mean(axis=0)).max()), float(np.abs(ref_centers).max()))
    assert np.abs(res["centers"] - ref_centers).max() <= (m_max + 3) * 2.0 ** -24 * scale


def _dup_blobs(n, dim, k):
    from gdd import synth
    X = synth.blobs(n, dim, max(1, k // 3), seed=n)
    X[1::7] = X[0]
    return X


@pytest.mark.parametrize("n,dim,k", [(3001, 8, 12), (300, 3, 12), (50, 4, 50)])
def test_reduce_worlds_are_byte_identical(tmp_path, n, dim, k):
    # (50, 4, 50): duplicated rows and k = n, so clusters empty out and are relocated; worlds 3 and 4
    # leave ranks with almost no rows (m = 17 and 13: the last rank holds 16 and 11 rows)
    _paths()
    from oracle import oracle as O
    X = _dup_blobs(n, dim, k)
    one = _fit(X, k, 1, 7, mstep="reduce")[1]  # no process group: world 1
    runs = [_run(w, X, k, 1, 7, tmp_path / f"w{w}") for w in (1, 2, 3, 4)]
    for r in runs:
        _same({key: np.asarray(v) for key, v in one.items()}, r)
    ref = O.kmeans(X, k, random_state=7)
    _contract(X, runs[-1], ref["labels_"], ref["n_iter_"], ref["inertia_"], ref["cluster_centers_"],
              inertia=(n, dim, k) != (50, 4, 50))  # inertia ~ 0 there: labels and centres only


@pytest.mark.parametrize("n_init", [1, 10])
def test_reduce_contract_sklearn_fixture(n_init):
    _paths()
    from golden_util import load
    z = load("golden_kmeans.npz")
    m, res = _fit(z["km_X"], 70, n_init, None, mstep="reduce")
    assert m.mode_ == "reduce"
    tag = f"km{n_init}"
    _contract(z["km_X"], res, z[f"{tag}_labels"], z[f"{tag}_n_iter"], z[f"{tag}_inertia"], z[f"{tag}_centers"])


@pytest.mark.parametrize("n,dim,k,dup", [(4099, 47, 33, True), (4099, 100, 20, True),
                                         (3000, 8, 12, False), (4099, 47, 33, False)])
def test_reduce_contract_oracle(n, dim, k, dup):
    """dup: few wide blobs with every 7th row a copy of row 0; otherwise k separated blobs."""
    _paths()
    from gdd import synth
    from oracle import oracle as O
    X = _dup_blobs(n, dim, k) if dup else synth.blobs(n, dim, k, seed=n)
    ref = O.kmeans(X, k, random_state=7)
    res = _fit(X, k, 1, 7, mstep="reduce")[1]
    _contract(X, res, ref["labels_"], ref["n_iter_"], ref["inertia_"], ref["cluster_centers_"])


def test_reduce_refuses_column_split_and_unknown_mstep():
    _paths()
    from gdd import sharded
    with pytest.raises(ValueError):
        sharded.ShardedKMeans(n_clusters=4, split_columns=True, mstep="reduce").fit(np.zeros((8, 2), np.float32))
    with pytest.raises(ValueError):
        sharded.ShardedKMeans(n_clusters=4, mstep="sorted")


def test_default_mstep_keeps_the_ordered_bits():
    _paths()
    from oracle import oracle as O
    X = _dup_blobs(300, 3, 12)
    ref = O.kmeans(X, 12, random_state=7)
    m, res = _fit(X, 12, 1, 7)
    assert m.mode_ == "rows" and m.mstep == "ordered"
    assert int(res["n_iter"]) == ref["n_iter_"]
    assert np.array_equal(res["labels"], ref["labels_"])
    assert np.array_equal(res["centers"].view(np.uint32), ref["cluster_centers_"].view(np.uint32))
    assert float(res["inertia"]) == ref["inertia_"]
