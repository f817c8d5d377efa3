"""gdd_cluster_positions on the device: the integers of gdd_score_positions on the expanded tables
``cu_z[u2cu]``, ``ci_z[i2ci]`` (equality; the score of a pair is a function of its two rows alone, so
the cluster kernel sees the expanded kernel's bits), and on grid tables also the plain definition
(tests/rankpos_ref.py)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rankeval_ref as R  # noqa: E402
import rankpos_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def labels(rng, n, k):
    """Every cluster non-empty where n >= k, in a random order."""
    lab = np.concatenate([np.arange(min(n, k)), rng.randint(0, k, max(0, n - k))])
    return rng.permutation(lab).astype(np.int64)


def check(cu, ci, u2cu, i2ci, targets, users=None, mask=None, mask_value=-1024.0, exact=True):
    """Cluster kernel == dense kernel on the expanded tables (== the definition where ``exact``)."""
    import gdd
    cu_t, ci_t = dev(cu), dev(ci)
    got = gdd.rank_positions_condensed(cu_t, ci_t, u2cu, i2ci, targets, users=users, exclude=mask,
                                       mask_value=mask_value)
    want = gdd.rank_positions(cu_t[dev(u2cu)], ci_t[dev(i2ci)], targets, users=users, exclude=mask,
                                mask_value=mask_value)
    assert got.dtype == torch.int32 and got.is_cuda and got.shape == want.shape
    assert torch.equal(got, want)
    if exact:
        sel = np.arange(len(u2cu)) if users is None else np.asarray(users)
        m = None if mask is None else R.take_rows(mask[0], mask[1], sel)
        ptr, col = targets
        ref = P.positions(P.masked_scores32(cu[u2cu], ci[i2ci], sel, m, mask_value), ptr, col)
        assert np.array_equal(got.cpu().numpy(), ref)
    return got.cpu().numpy()


def targets_for(rng, B, I, lens_cycle, mask=None):
    lens = np.array([lens_cycle[b % len(lens_cycle)] for b in range(B)])
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = rng.randint(0, I, ptr[-1]).astype(np.int32)
    if mask is not None:
        for b in range(B):  # a masked target at the head of the row, a repeat at its end
            row = mask[1][mask[0][b]:mask[0][b + 1]]
            if lens[b] and row.size:
                col[ptr[b]] = row[rng.randint(row.size)]
            if lens[b] > 2:
                col[ptr[b + 1] - 1] = col[ptr[b] + 1]
    return ptr, col


def random_mask(rng, nu, I, frac=0.05):
    return R.csr_of(*np.nonzero(rng.random_sample((nu, I)) < frac), nu)


# (num_ci, num_cu, d, users, items, mask_value): 0.5 and 0.0 tie grid scores
CROSS = [(1, 1, 1, 5, 40, -1024.0), (5, 3, 3, 17, 200, 0.5), (64, 8, 64, 40, 300, -1024.0),
         (65, 40, 65, 40, 257, 0.0), (257, 5, 200, 33, 1000, 0.5), (300, 16, 256, 64, 1000, 1e9)]


@pytest.mark.parametrize("num_ci,num_cu,d,nu,I,mask_value", CROSS)
def test_grid_cross(num_ci, num_cu, d, nu, I, mask_value):
    """Users sharing a cluster (nu > num_cu) and users alone in one (num_cu = nu = 40); a subset of the
    users with a repeat; target rows of 0, 1, 7 and 70 items; masked and repeated targets."""
    rng = np.random.RandomState(num_ci * 5 + d)
    cu, ci = R.grid(rng, num_cu, d), R.grid(rng, num_ci, d)
    u2cu = np.arange(nu) % num_cu if num_cu == nu else labels(rng, nu, num_cu)
    i2ci = labels(rng, I, num_ci)
    mask = random_mask(rng, nu, I)
    users = rng.permutation(nu)[:max(1, nu - 3)]
    users[-1] = users[0]
    m = R.take_rows(mask[0], mask[1], users)
    check(cu, ci, u2cu, i2ci, targets_for(rng, len(users), I, (7, 0, 1, 70), m), users, mask, mask_value)
    check(cu, ci, u2cu, i2ci, targets_for(rng, nu, I, (3,)), None, None, mask_value)


def test_cluster_sizes_and_duplicate_rows():
    """Clusters of 0, 1, 63, 64, 65 and 300 members; clusters 2 and 4 (63 and 65 members) share one
    row, so their members interleave by item id; every item is a target once."""
    rng = np.random.RandomState(31)
    sizes = [0, 1, 63, 64, 65, 300, 0, 7]
    i2ci = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
    I, d, nu = len(i2ci), 6, 9
    ci = R.grid(rng, len(sizes), d)
    ci[4] = ci[2]
    cu = R.grid(rng, 4, d)
    u2cu = labels(rng, nu, 4)
    tg = (np.arange(nu + 1, dtype=np.int32) * I, np.concatenate([rng.permutation(I) for _ in range(nu)]).astype(np.int32))
    pos = check(cu, ci, u2cu, i2ci, tg).reshape(nu, I)
    assert np.array_equal(np.sort(pos, 1), np.arange(I)[None, :].repeat(nu, 0))  # a full ranking
    mask = random_mask(rng, nu, I, 0.1)
    check(cu, ci, u2cu, i2ci, tg, None, mask, -1024.0)


@pytest.mark.parametrize("mask_value", [-1024.0, 0.5, 1e9, -0.0])
def test_masked_items_inside_tied_clusters(mask_value):
    """All cluster rows equal up to three values, so most clusters tie; user 0's mask is every item,
    user 1's every member of one cluster, user 2's a row longer than a tile; targets are masked and
    unmasked members of tied clusters. mask_value 0.5 ties a cluster score, -0.0 ranks just below the
    +0 scores."""
    rng = np.random.RandomState(17)
    num_ci, I, nu, d = 12, 400, 6, 2
    ci = np.zeros((num_ci, d), np.float32)
    ci[:, 0] = rng.choice([0.0, 0.5, 1.0], num_ci)
    cu = np.array([[1.0, 0.0], [0.0, 1.0], [-1.0, 0.5]], np.float32)  # scores in {0, .5, 1}, all 0, {0, -.5, -1}
    u2cu = np.array([0, 1, 2, 0, 1, 2])
    i2ci = labels(rng, I, num_ci)
    rows = [np.arange(I), np.nonzero(i2ci == 3)[0], rng.permutation(I)[:150], np.zeros(0, int),
            rng.permutation(I)[:5], np.arange(0, I, 2)]
    mask = R.csr_of(np.concatenate([np.full(len(c), u) for u, c in enumerate(rows)]), np.concatenate(rows), nu)
    tg = targets_for(rng, nu, I, (40, 64, 65), mask)
    check(cu, ci, u2cu, i2ci, tg, None, mask, mask_value)


@pytest.mark.parametrize("num_ci", [4095, 4096, 4097])
@pytest.mark.parametrize("d", [2, 16])
def test_both_sides_of_the_ranked_row_limit(num_ci, d):
    """Up to 4096 item clusters the rows of the score table are ranked once and a target costs a binary
    search; past it every cluster is visited per target. d = 2: a handful of distinct scores, so
    thousands of tied clusters; d = 16: few ties. Empty clusters, a mask, mask_value tying scores."""
    rng = np.random.RandomState(num_ci + d)
    nu, I, num_cu = 9, 5000, 3
    cu, ci = R.grid(rng, num_cu, d), R.grid(rng, num_ci, d)
    u2cu = labels(rng, nu, num_cu)
    i2ci = rng.randint(0, num_ci, I)
    mask = random_mask(rng, nu, I, 0.02)
    check(cu, ci, u2cu, i2ci, targets_for(rng, nu, I, (5, 70, 0, 1), mask), None, mask, 0.5)


def test_random_normal_inputs_workspace_and_repeatability():
    """Arbitrary floats (no exact reference: the dense kernel on the expanded tables is one); the
    method, the function and a second call agree; the declared workspace is the G x num_ci table."""
    import gdd
    rng = np.random.RandomState(12)
    num_cu, num_ci, d, nu, I = 30, 300, 64, 200, 2000
    cu, ci = rng.randn(num_cu, d).astype(np.float32), rng.randn(num_ci, d).astype(np.float32)
    u2cu, i2ci = labels(rng, nu, num_cu), labels(rng, I, num_ci)
    mask = random_mask(rng, nu, I, 0.02)
    users = rng.permutation(nu)[:90]
    tg = targets_for(rng, 90, I, (20, 100, 0, 300), R.take_rows(mask[0], mask[1], users))
    a = check(cu, ci, u2cu, i2ci, tg, users, mask, -1e9, exact=False)
    rec = gdd.CondensedRecommender(dev(cu), dev(ci), u2cu, i2ci)
    b = rec.positions(tg, users=users, exclude=mask, mask_value=-1e9)
    c = rec.positions(tg, users=users, exclude=mask, mask_value=-1e9)
    assert np.array_equal(a, b.cpu().numpy()) and torch.equal(b, c)
    G = len(np.unique(u2cu[users]))
    # the score table, the ranked rows and their prefix sizes; past 4096 clusters the table alone
    assert rec.last_info == {"ranked_clusters": G, "workspace_bytes": 4 * G * (3 * num_ci + 1)}
    from gdd.rankpos import condensed_workspace_bytes
    assert condensed_workspace_bytes(G, num_ci) == 4 * G * (3 * num_ci + 1)
    assert condensed_workspace_bytes(7, 4096) == 4 * 7 * (3 * 4096 + 1) and condensed_workspace_bytes(7, 4097) == 4 * 7 * 4097
    # 2-D targets: the ranked lists of recommend() sit at positions 0 .. k-1
    lists = rec.recommend(50, users=users, exclude=mask, mask_value=-1e9)
    pos = rec.positions(lists, users=users, exclude=mask, mask_value=-1e9)
    assert torch.equal(pos.cpu(), torch.arange(50, dtype=torch.int32)[None, :].expand(90, 50))


def test_invalid_rows():
    """A mask column == I and a target == I (device tensor: checked by the kernel) give RuntimeError;
    the raw entry point marks those rows -1, counts them, and leaves the others right."""
    import gdd
    from gdd import _lib
    rng = np.random.RandomState(14)
    d, num_cu, num_ci, nu, I = 8, 4, 30, 10, 600
    cu, ci = R.grid(rng, num_cu, d), R.grid(rng, num_ci, d)
    u2cu, i2ci = labels(rng, nu, num_cu), labels(rng, I, num_ci)
    cu_t, ci_t = dev(cu), dev(ci)
    mp = np.array([0, 2, 2, 4, 4, 4, 4, 4, 4, 4, 4], np.int32)
    mc = np.array([3, 9, 7, I], np.int32)  # user 2: a column == I
    with pytest.raises(RuntimeError, match="out of range"):
        gdd.rank_positions_condensed(cu_t, ci_t, u2cu, i2ci, np.zeros((nu, 2), np.int64), exclude=(mp, mc))
    tgt = torch.zeros(nu, 2, dtype=torch.int32, device="cuda")
    tgt[5, 0] = I
    with pytest.raises(RuntimeError, match="out of range"):
        gdd.rank_positions_condensed(cu_t, ci_t, u2cu, i2ci, tgt)

    lib = _lib.device_lib()
    rec = gdd.CondensedRecommender(cu_t, ci_t, u2cu, i2ci)
    g = rec._prepare()
    users = np.arange(nu, dtype=np.int32)
    users[4] = nu
    groups, row = np.unique(u2cu, return_inverse=True)
    tp = (np.arange(nu + 1) * 2).astype(np.int32)
    tc = rng.randint(0, I, 2 * nu).astype(np.int32)
    tc[5 * 2] = I
    G = len(groups)
    ws_bytes = lib.gdd_cluster_positions_ws_bytes(G, num_ci)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    pos_t = torch.full((2 * nu,), 7, dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    t = [dev(a) for a in (users, row.astype(np.int32), groups.astype(np.int32), i2ci.astype(np.int32), mp, mc, tp, tc)]
    _lib.check(lib.gdd_cluster_positions(
        nu, I, num_cu, num_ci, d, cu_t.data_ptr(), ci_t.data_ptr(), t[0].data_ptr(), nu, t[1].data_ptr(), G,
        t[2].data_ptr(), t[3].data_ptr(), g["mem_ptr"].data_ptr(), g["mem_item"].data_ptr(), t[4].data_ptr(),
        t[5].data_ptr(), -1024.0, t[6].data_ptr(), t[7].data_ptr(), pos_t.data_ptr(), bad.data_ptr(), ws.data_ptr(),
        ws_bytes, _lib.stream_ptr(torch.device("cuda"))))
    assert int(bad.item()) == 3
    pos = pos_t.cpu().numpy().reshape(nu, 2)
    for b in (2, 4, 5):
        assert (pos[b] == -1).all()
    good = np.setdiff1d(np.arange(nu), [2, 4, 5])
    gm, gt = R.take_rows(mp, mc, good), R.take_rows(tp, tc, good)
    want = P.positions(P.masked_scores32(cu[u2cu], ci[i2ci], good, gm), gt[0], gt[1])
    assert np.array_equal(pos[good].ravel(), want)
    # a workspace smaller than declared is refused on the host
    rc = lib.gdd_cluster_positions(
        nu, I, num_cu, num_ci, d, cu_t.data_ptr(), ci_t.data_ptr(), t[0].data_ptr(), nu, t[1].data_ptr(), G,
        t[2].data_ptr(), t[3].data_ptr(), g["mem_ptr"].data_ptr(), g["mem_item"].data_ptr(), t[4].data_ptr(),
        t[5].data_ptr(), -1024.0, t[6].data_ptr(), t[7].data_ptr(), pos_t.data_ptr(), bad.data_ptr(),
        ws.data_ptr(), ws_bytes - 1, _lib.stream_ptr(torch.device("cuda")))
    assert rc != 0 and b"workspace" in lib.gdd_last_error()
