"""The host model of the community node order (tests/community_util.py) on the stochastic block model
it was designed on: n = 8192, 256-node blocks, average degree 20, 90 % of the edges inside a block,
ids shuffled. Model only; the device path is pinned against it in test_gpu_community.py."""
import numpy as np
import pytest

import community_util as cu

N = 8192


def _near(seed, sweeps, **kw):
    rowptr, col = cu.sbm(seed, **kw)
    rho, lab, changed = cu.model("sbm", seed, sweeps, **kw)
    return cu.near_fraction(rowptr, col, rho), rho, lab, changed


@pytest.mark.parametrize("diag", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_sbm_8_sweeps_recovers_locality(seed, diag):
    rowptr, col = cu.sbm(seed, diag=diag)
    near, rho, lab, changed = _near(seed, 8, diag=diag)
    shuffled = cu.near_fraction(rowptr, col, np.arange(N))
    print(f"seed {seed} diag {diag}: near {near:.4f} shuffled {shuffled:.4f} changed {changed.tolist()}")
    assert np.array_equal(np.sort(rho), np.arange(N))
    assert near >= 0.80
    assert near >= shuffled + 0.5
    assert np.all(np.diff(changed) < 0)


def test_hubs_do_not_swallow_the_graph():
    rowptr, col = cu.sbm(0, hubs=3)
    assert np.sort(np.diff(rowptr))[-3] > 1000
    near, rho, lab, changed = _near(0, 8, hubs=3)
    biggest = int(np.bincount(lab).max())
    print(f"hubs: near {near:.4f} largest label {biggest}")
    assert near >= 0.75
    assert biggest <= N // 8


def test_fixed_point_matches_true_block_order():
    near, rho, lab, changed = _near(0, 16)
    rp_t, col_t = cu.sbm(0, shuffle=False)
    true = cu.near_fraction(rp_t, col_t, np.arange(N))
    print(f"16 sweeps: near {near:.4f} true order {true:.4f} changed {changed.tolist()}")
    assert changed[-1] == 0 and changed[-2] == 0
    assert abs(near - true) <= 0.01
    # a fixed point: a further sweep gives the same labels
    rowptr, col = cu.sbm(0)
    assert np.array_equal(cu.lpa_sweep(rowptr, col, lab), lab)


def test_small_cases():
    # 5-node path: ties resolve to the smallest label every sweep
    rowptr, col = cu.path(5)
    lab = np.arange(5)
    lab = cu.lpa_sweep(rowptr, col, lab)
    assert lab.tolist() == [0, 0, 1, 2, 3]
    rho, lab, changed = cu.community_order(rowptr, col, 0)
    assert rho.tolist() == [0, 1, 2, 3, 4] and changed.shape == (0,)
    # empty graph and n = 1: the identity
    rho, lab, changed = cu.community_order(np.zeros(8, np.int64), np.zeros(0, np.int64), 3)
    assert rho.tolist() == list(range(7)) and changed.tolist() == [0, 0, 0]
    rho, lab, changed = cu.community_order(np.zeros(2, np.int64), np.zeros(0, np.int64), 2)
    assert rho.tolist() == [0]

