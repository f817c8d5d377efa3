"""gdd_score_positions on the device against the plain definition (tests/rankpos_ref.py).

Positions are integers, so every check is equality.

* Grid inputs (entries in {-2..2}/2, d <= 256): every fp32 chain is exact whatever its order, so the
  fp64 product cast to fp32 is the score and ``rankpos_ref.positions`` is the reference; mask values
  that tie scores (0.5) make the tie rule matter for masked items too.
* Random normal inputs: the reference is ``recommend``, whose lists the positions must index.
* The kernel takes a user's targets 256 at a time (kRpChunk): rows of 255, 256, 257, 511, 512, 513.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rankeval_ref as R  # noqa: E402
import rankpos_ref as P  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 256


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def mixed_mask(rng, B, I):
    """Rows that cycle through: empty, one entry, more than 64 entries (where I allows; else half the
    items), every item."""
    rows, cols = [], []
    for b in range(B):
        kind = b % 4
        if kind == 1:
            c = rng.randint(0, I, 1)
        elif kind == 2:
            c = rng.permutation(I)[:max(1, min(I - 1, 70 + b % 7)) if I > 70 else max(1, I // 2)]
        elif kind == 3:
            c = np.arange(I)
        else:
            c = np.zeros(0, np.int64)
        rows.append(np.full(len(c), b))
        cols.append(c)
    return R.csr_of(np.concatenate(rows), np.concatenate(cols), B)


def random_targets(rng, lens_cycle, B, I, mask):
    """Unsorted targets with repeats, row b of length lens_cycle[b % len]; the first target of a row
    with a mask is masked."""
    lens = np.array([lens_cycle[b % len(lens_cycle)] for b in range(B)])
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = rng.randint(0, I, ptr[-1]).astype(np.int32)
    for b in range(B):
        row = mask[1][mask[0][b]:mask[0][b + 1]]
        if lens[b] and row.size:
            col[ptr[b]] = row[rng.randint(row.size)]
    return ptr, col


# (I, d, B, a subset of the users with a repeat?, row lengths, mask_value): every value of the issue's
# lists at least once, and the chunk size and its multiples +-1
GRID_CASES = [
    (1, 1, 1, False, (3,), -1024.0),
    (63, 3, 15, True, (0, 1, 63), 0.5),
    (64, 64, 16, False, (64, 65, 1), -1024.0),
    (65, 65, 17, True, (65, 0, 300), 1e9),
    (257, 200, 16, False, (CHUNK - 1, CHUNK, CHUNK + 1), 0.5),
    (1000, 256, 15, True, (300, 1, 63, 2 * CHUNK + 1), -1024.0),
    (1000, 64, 300, False, (0, 1, 5, 64), 0.5),
    (257, 1, 300, True, (1, 2, 0), 1e9),
    (1000, 3, 17, False, (2 * CHUNK, 2 * CHUNK - 1, 20), -1024.0),
    (64, 200, 1, True, (300,), 0.5),
    # the prefetch depths on both sides of their edges: d = 68 and 128 stage a tile in eight float4 per
    # thread, d = 132 in sixteen (d = 64 in four, d = 256 in sixteen, above)
    (65, 68, 17, True, (0, 1, 65), 0.5),
    (257, 128, 16, False, (65, 1, 0), -1024.0),
    (65, 132, 15, True, (1, 65, 0), 1e9),
]


def dev_off4(a):
    """``a`` on the device, contiguous, its first element 4 bytes past a 16-byte boundary."""
    flat = torch.empty(a.size + 1, dtype=torch.float32, device="cuda")
    t = flat[1:1 + a.size].view(*a.shape)
    t.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4
    return t


@pytest.mark.parametrize("I,d,B,subset,lens,mask_value", GRID_CASES)
def test_grid_inputs_positions_are_the_definition(I, d, B, subset, lens, mask_value):
    check_grid_case(I, d, B, subset, lens, mask_value, dev)


def test_grid_inputs_item_table_off_16_byte_alignment():
    """d = 64 with the item table 4 bytes past a 16-byte boundary: d % 4 == 0, yet the tile is staged
    float by float."""
    check_grid_case(257, 64, 17, True, (0, 1, 65), 0.5, dev_off4)


def check_grid_case(I, d, B, subset, lens, mask_value, vdev):
    import gdd
    rng = np.random.RandomState(I * 7 + d * 3 + B)
    nu = B + 5 if subset else B
    U, V = R.grid(rng, nu, d), R.grid(rng, I, d)
    users = None
    if subset:
        users = rng.permutation(nu)[:B]
        if B > 1:
            users[-1] = users[0]  # a repeated id
    sel = np.arange(nu) if users is None else users
    mask = mixed_mask(rng, B, I)  # rows in call order
    # exclude is given over all users: scatter the call's rows to their users (a repeat shares its row)
    all_rows = [np.zeros(0, np.int64)] * nu
    for b, u in enumerate(sel):
        all_rows[u] = mask[1][mask[0][b]:mask[0][b + 1]]
    excl = R.csr_of(np.concatenate([np.full(len(c), u) for u, c in enumerate(all_rows)]),
                    np.concatenate(all_rows), nu)
    mask = R.take_rows(excl[0], excl[1], sel)
    ptr, col = random_targets(rng, lens, B, I, mask)
    Vt = vdev(V)
    got = gdd.rank_positions(dev(U), Vt, (ptr, col), users=users, exclude=excl, mask_value=mask_value)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (len(col),)
    want = P.positions(P.masked_scores32(U, V, sel, mask, mask_value), ptr, col)
    assert np.array_equal(got.cpu().numpy(), want)


def test_two_dimensional_targets_and_the_default_users():
    """A [B, T] array (here each user's full ranked list, on the device) gives [B, T]: the inverse of
    the list is 0 .. T-1; no exclude and an exclude without entries are the same."""
    import gdd
    rng = np.random.RandomState(2)
    U, V = R.grid(rng, 37, 5), R.grid(rng, 130, 5)
    lists = gdd.recommend(dev(U), dev(V), 130)
    for t in (lists, lists.cpu().numpy(), lists.to(torch.int64)):
        pos = gdd.rank_positions(dev(U), dev(V), t)
        assert tuple(pos.shape) == (37, 130) and pos.dtype == torch.int32
        assert torch.equal(pos.cpu(), torch.arange(130, dtype=torch.int32)[None, :].expand(37, 130))
    empty = (np.zeros(38, np.int32), np.zeros(0, np.int32))
    assert torch.equal(gdd.rank_positions(dev(U), dev(V), lists, exclude=empty), pos)
    none = gdd.rank_positions(dev(U), dev(V), np.zeros((37, 0), np.int64))
    assert tuple(none.shape) == (37, 0)


@pytest.fixture(scope="module")
def normal():
    rng = np.random.RandomState(11)
    nu, d = 21, 65
    U = rng.randn(nu, d).astype(np.float32)
    mask = R.csr_of(*np.nonzero(rng.random_sample((nu, 1000)) < 0.05), nu)
    return dict(rng=rng, U=U, V=rng.randn(1000, d).astype(np.float32), mask=mask, nu=nu)


def test_normal_floats_positions_invert_the_full_list(normal):
    """I = 200 <= 256: the positions of all items, asked in a shuffled order, are the inverse
    permutation of recommend(k = I); two runs give the same integers."""
    import gdd
    n, I = normal, 200
    U, V = dev(n["U"]), dev(n["V"][:I])
    keep = n["mask"][1] < I
    rows = np.repeat(np.arange(n["nu"]), np.diff(n["mask"][0]))
    mask = R.csr_of(rows[keep], n["mask"][1][keep], n["nu"])
    lists = gdd.recommend(U, V, I, exclude=mask).cpu().numpy()
    order = np.stack([np.random.RandomState(b).permutation(I) for b in range(n["nu"])])
    pos = gdd.rank_positions(U, V, order, exclude=mask)
    again = gdd.rank_positions(U, V, order, exclude=mask)
    assert torch.equal(pos, again)
    pos = pos.cpu().numpy()
    assert np.array_equal(np.take_along_axis(lists, pos, 1), order)


def test_normal_floats_positions_index_the_top_256(normal):
    """I = 1000: all items as targets (four chunks per user, users in another order with a repeat):
    a target with pos < 256 sits at that index of recommend(k = 256), every other has pos >= 256, and
    the positions of a row are a permutation of 0 .. I-1."""
    import gdd
    n, I, K = normal, 1000, 256
    U, V = dev(n["U"]), dev(n["V"])
    users = np.concatenate([np.random.RandomState(3).permutation(n["nu"]), [4]])
    lists = gdd.recommend(U, V, K, users=users, exclude=n["mask"]).cpu().numpy()
    order = np.stack([np.random.RandomState(b).permutation(I) for b in range(len(users))])
    pos = gdd.rank_positions(U, V, order, users=users, exclude=n["mask"]).cpu().numpy()
    assert np.array_equal(np.sort(pos, 1), np.arange(I)[None, :].repeat(len(users), 0))
    inside = pos < K
    assert (inside.sum(1) == K).all()
    b, j = np.nonzero(inside)
    assert np.array_equal(lists[b, pos[b, j]], order[b, j])
    assert np.array_equal(pos[-1], pos[list(users).index(4)][np.argsort(order[list(users).index(4)])][order[-1]])


def test_invalid_rows_are_minus_one_and_counted():
    """The raw entry point: user 4's id is outside the table, user 2's mask row holds the column I,
    user 6's target row the column -1; those rows are -1, bad == 3, the others are right. Through the
    Python surface a device tensor of targets is checked by the kernel: RuntimeError."""
    import gdd
    from gdd import _lib
    rng = np.random.RandomState(14)
    nu, I, d = 10, 100, 8
    U, V = R.grid(rng, nu, d), R.grid(rng, I, d)
    users = np.arange(nu, dtype=np.int32)
    users[4] = nu
    mp = np.array([0, 2, 2, 4, 4, 4, 4, 4, 4, 4, 4], np.int32)
    mc = np.array([3, 9, 7, I], np.int32)
    tp = (np.arange(nu + 1) * 3).astype(np.int32)
    tc = rng.randint(0, I, 3 * nu).astype(np.int32)
    tc[6 * 3 + 1] = -1
    lib = _lib.device_lib()
    Ut, Vt = dev(U), dev(V)
    t = [dev(a) for a in (users, mp, mc, tp, tc)]
    pos = torch.full((3 * nu,), 7, dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.gdd_score_positions(nu, I, d, t[0].data_ptr(), Ut.data_ptr(), nu, Vt.data_ptr(), t[1].data_ptr(),
                                       t[2].data_ptr(), -1024.0, t[3].data_ptr(), t[4].data_ptr(), pos.data_ptr(),
                                       bad.data_ptr(), _lib.stream_ptr(torch.device("cuda"))))
    assert int(bad.item()) == 3
    pos = pos.cpu().numpy().reshape(nu, 3)
    for b in (2, 4, 6):
        assert (pos[b] == -1).all()
    good = np.setdiff1d(np.arange(nu), [2, 4, 6])
    gm = R.take_rows(mp, mc, good)
    gt = R.take_rows(tp, tc, good)
    want = P.positions(P.masked_scores32(U, V, good, gm), gt[0], gt[1])
    assert np.array_equal(pos[good].ravel(), want)

    tgt = torch.zeros(nu, 2, dtype=torch.int32, device="cuda")
    tgt[3, 1] = I
    with pytest.raises(RuntimeError, match="out of range"):
        gdd.rank_positions(Ut, Vt, tgt)
    with pytest.raises(RuntimeError, match="out of range"):
        gdd.rank_positions(Ut, Vt, np.zeros((nu, 2), np.int64), exclude=(mp, mc))


def test_no_score_matrix_is_allocated():
    """B = 2,000, I = 5,000, d = 16 (a score matrix would be 40 MB): over the call the peak of the
    allocator rises by less than the output, the device copies of mask and targets and 64 KB (the
    kernel declares no workspace)."""
    import gdd
    rng = np.random.RandomState(6)
    B, I, d, T = 2000, 5000, 16, 10
    U, V = dev(rng.randn(B, d).astype(np.float32)), dev(rng.randn(I, d).astype(np.float32))
    mask = R.csr_of(rng.randint(0, B, 20000), rng.randint(0, I, 20000), B)
    tg = rng.randint(0, I, (B, T))
    gdd.rank_positions(U[:16], V, tg[:16])  # the library is loaded, the kernel's code is resident
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    pos = gdd.rank_positions(U, V, tg, exclude=mask)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    allowed = 4 * B * T + 4 * (B + 1 + len(mask[1])) + 4 * (B + 1 + B * T) + 64 * 1024
    print(f"peak rise {rise} bytes, allowed {allowed}, a score matrix {4 * B * I}")
    assert rise < allowed < 4 * B * I // 50
    lists = gdd.recommend(U, V, 256, exclude=mask).cpu().numpy()
    pos = pos.cpu().numpy()
    b, j = np.nonzero(pos < 256)
    assert len(b) > 0 and np.array_equal(lists[b, pos[b, j]], tg[b, j])
