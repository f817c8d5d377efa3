"""The bf16 labels pass (gdd_kmeans_assign_bf16) against the exact-product model of
tests/bf16_model.py — needs a gfx950 GPU.

Every label must be the nearest centre under exact bf16-rounded products with the fp32 norms, up to
the derived fp32 accumulation slack (zero violations of 2 E); the model itself must be decisive
(undecided share <= 0.02); sq_dist must equal the oracle's _euclidean_dense_dense
(oracle.labels_sqdist, _k_means_common.pyx:26-48) bit for bit; on integer lattices the label must be
a true nearest centre with no tolerance at all. Each case asserts gdd_kmeans_assign_path, so a
planning change cannot silently move it to another kernel.

Case -> instantiation, from pick_per (gdd_bf16.hip; PER = float4 loads per lane per tile, 8 dim / 64
rounded up to 1, 2, 4, 6, 8; NST = ceil(dim / 16); VEC4 = dim % 4 == 0; W waves, D tiles in flight)
and assign_bf16p (gdd_kmeans.hip; PER the first of 1, 2, 4, 6, 8, 12, 16 >= ceil(dim / 8)):

  k_assign_bf16q<PER, NST, VEC4, W, D, WPE[, DIM]>             sweep (a)        lattice (d)   (f)
    <1, 1, F, 4, 2, 1>        dims 1-3, 5-7                     bf16q/w4         1, 7          7
    <1, 1, T, 4, 2, 1>        dims 4, 8                         bf16q/w4         8
    <2, 1, F, 4, 2, 1>        dims 9-11, 13-15                  bf16q/w4         9, 15
    <2, 1, T, 4, 2, 1>        dim 12                            bf16q/w4         12            12
    <4, 2, F, 4, 2, 1>        dims 17-31 off multiples of 4     bf16q/w4         17, 23, 31
    <4, 2, T, 4, 2, 1>        dims 20, 24, 28                   bf16q/w4         24            20
    <6, 3, F, 4, 2, 1>        dims 33-47 off 4, not 41, 47      bf16q/w4         33, 45
    <6, 3, F, 4, 2, 1, 41>    dim 41 (also forced bf16_w4)      bf16q/w4         41            41
    <6, 3, F, 4, 2, 1, 47>    dim 47 (also forced bf16_w4)      bf16q/w4         47
    <6, 3, T, 4, 2, 1>        dims 36, 44                       bf16q/w4         44
    <6, 3, T, 4, 2, 1, 40>    dim 40                            bf16q/w4         40
    <6, 3, F, 8, 1, 4>        dims 42, 43, 45, 46, bf16_w8      bf16q/w8         45
    <6, 3, F, 8, 1, 4, 41>    dim 41, bf16_w8                   bf16q/w8         41            41
    <6, 3, F, 8, 1, 4, 47>    dim 47, bf16_w8                   bf16q/w8         47
    <8, 4, F, 4, 2, 1>        dims 49-63 off multiples of 4     bf16q/w4         49, 57, 63    57
    <8, 4, T, 4, 2, 1>        dims 52, 56, 60                   bf16q/w4         56
  k_bf16_frags + k_assign_bf16p<PER>                           sweep (b)
    <1>    dim 5, bf16_v1                                       bf16p/per1       5
    <2>    dim 12, bf16_v1; dim 16                              bf16p/per2       16
    <4>    dim 23, bf16_v1; dim 32                              bf16p/per3, 4    23, 32
    <6>    dim 45, bf16_v1; dim 48                              bf16p/per6       48
    <8>    dim 64                                               bf16p/per8       64            64
    <12>   dims 70, 80, 96                                      bf16p/per9-12    96
    <16>   dims 100, 112, 127, 128                              bf16p/per13-16   128
  k_assign_bf16<4 | 2> + k_assign_finalize                     (c): n < 32, a row list, X unaligned,
    bf16_tiles/<cch>x<gy>/prefill                               dims 129, 200, 496, 497, 512, k = 3000 at
                                                                dim 40; lattice 129, 512 (two waves per
                                                                block from 497), and every lattice shape
                                                                whose fragments exceed the workspace
(The other PER x NST pairs of the template are not reachable: 8 dim / 64 and dim / 16 move together.)

The persistent kernels need their centre fragments to fit the labels pass's workspace (8 n bytes):
at n = 2013 the widest shapes of (b) (dim >= 96 at k = 96, dim >= 127 at k = 33) take the tiles
form, which is asserted, and run again at n = 4013 where the r03 kernel takes them.
"""
import numpy as np
import pytest
import torch

import bf16_model as M
from gpu_util import bf16_check, force
from oracle import oracle as O

pytestmark = pytest.mark.gpu

from gdd import _lib  # noqa: E402
from gdd.kmeans import _Ops  # noqa: E402

N = 2000 + 13  # 62 full tiles and a partial one
KS = (1, 33, 96)  # one, two and three centre tiles: the pair loop's tail, its body, both
BF16, ROWS, X_UNALIGNED = 8, 1, 2  # GDD_ASSIGN_* (gdd.h)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def path_of(n, dim, k, flags=0):
    return _lib.device_lib().gdd_kmeans_assign_path(n, dim, k, BF16 | flags).decode()


def assign_bf16(X, C, rows=None, Xd=None, sq=True):
    """Labels and sq_dist of _Ops.assign(precision='bf16') with the workspace of exactly this n."""
    dim, k = C.shape[1], C.shape[0]
    Xd = torch.from_numpy(X).cuda() if Xd is None else Xd
    Cd = torch.from_numpy(C).cuda()
    rd = None if rows is None else torch.from_numpy(rows).cuda()
    n = Xd.shape[0] if rows is None else rows.shape[0]
    ops = _Ops("cuda", n, k, dim)
    lab = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    sqd = torch.full((n,), -1.0, dtype=torch.float32, device="cuda") if sq else None
    ops.assign(Xd, Cd, rows=rd, labels=lab, sq=sqd, precision="bf16")
    return lab.cpu().numpy(), (sqd.cpu().numpy() if sq else None)


def check_case(X, C, path, rows=None, Xd=None, tag=""):
    """One call: zero violations, the model decisive, sq_dist exact. X: the rows as the pass sees
    them (already gathered when a row list is given through Xd / rows)."""
    lab, sq = assign_bf16(X, C, rows=rows, Xd=Xd)
    viol, und, worst = bf16_check(X, C, lab, path)
    print(f"bf16-model {tag} n={X.shape[0]} dim={X.shape[1]} k={C.shape[0]} path={path} "
          f"violations={viol} undecided={und:.4f} worst_ratio={worst:.3f}")
    assert viol == 0, (path, viol, worst)
    assert und <= 0.02, (path, und)
    assert np.array_equal(bits(sq), bits(O.labels_sqdist(X, C, lab)))
    return lab


# ---- (a) the r06 kernel: every dim it takes -------------------------------------------------------
@pytest.mark.parametrize("dim", [d for d in range(1, 64) if d % 16])
def test_r06_dim_sweep(dim, monkeypatch):
    force(monkeypatch)
    for k in KS:
        path = path_of(N, dim, k)
        assert path == "bf16q/w4"
        X, C = M.points(N, dim, k, seed=1000 * dim + k)
        check_case(X, C, path, tag="a")


@pytest.mark.parametrize("form,waves", [("bf16_w8", 8), ("bf16_w4", 4)])
@pytest.mark.parametrize("dim", [41, 42, 43, 45, 46, 47])
def test_r06_forced_block_forms(dim, form, waves, monkeypatch):
    force(monkeypatch, form)
    for k in KS:
        path = path_of(N, dim, k)
        assert path == f"bf16q/w{waves}"
        X, C = M.points(N, dim, k, seed=1000 * dim + k + waves)
        check_case(X, C, path, tag="a/" + form)


# ---- (b) the r03 kernel: every PER of assign_bf16p -----------------------------------------------
def frags_fit(n, dim, k):
    """bf16_frag_bytes <= gdd_kmeans_assign_ws_bytes(n) (assign_plan): the persistent kernels' gate."""
    kt, nst = (k + 31) // 32, (dim + 15) // 16
    return kt * (nst * 1024 + 128) <= (8 * n + 255) // 256 * 256


def r03_expect(n, dim, k):
    return f"bf16p/per{(dim + 7) // 8}" if frags_fit(n, dim, k) else "bf16_tiles/"


@pytest.mark.parametrize("n,dim", [(N, d) for d in (16, 32, 48, 64, 70, 80, 96, 100, 112, 127, 128)] +
                         [(2 * 2000 + 13, d) for d in (96, 100, 112, 127, 128)])
def test_r03_dim_sweep(n, dim, monkeypatch):
    force(monkeypatch)
    tiles = {(d, k) for d in (96, 100, 112, 127, 128) for k in (96,)} | {(127, 33), (128, 33)}
    for k in KS:
        path = path_of(n, dim, k)
        assert path.startswith(r03_expect(n, dim, k))
        assert path.startswith("bf16_tiles/") == (n == N and (dim, k) in tiles), path  # as listed above
        X, C = M.points(n, dim, k, seed=1000 * dim + k)
        check_case(X, C, path, tag="b")


@pytest.mark.parametrize("dim", [5, 12, 23, 45])
def test_r03_forced_at_r06_dims(dim, monkeypatch):
    force(monkeypatch, "bf16_v1")
    for k in KS:
        path = path_of(N, dim, k)
        assert path == f"bf16p/per{(dim + 7) // 8}"
        X, C = M.points(N, dim, k, seed=1000 * dim + k + 1)
        check_case(X, C, path, tag="b/bf16_v1")


# ---- (c) the tiles form ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,dim", [(1, 41), (1, 64), (31, 41), (31, 47), (31, 64)])
def test_tiles_fewer_rows_than_a_tile(n, dim, monkeypatch):
    """n < 32: below the r06 kernel's floor and the fragments' workspace. The rows are the first of
    a larger sample the centres are drawn from; the seeds are ones at which the model decides every
    one of these few rows (one undecided row of 31 is already 3 %)."""
    force(monkeypatch)
    for k in KS:
        path = path_of(n, dim, k)
        assert path.startswith("bf16_tiles/"), path
        X, C = M.points(N, dim, k, seed=3 + k)
        check_case(np.ascontiguousarray(X[:n]), C, path, tag="c/n<32")


@pytest.mark.parametrize("dim", [41, 64])
def test_tiles_row_list_shuffled_with_repeats(dim, monkeypatch):
    force(monkeypatch)
    rng = np.random.default_rng(7)
    rows = np.concatenate([rng.permutation(N), rng.integers(0, N, 500), [N - 1, N - 1, 0, 0]]).astype(np.int64)
    for k in KS:
        X, C = M.points(N, dim, k, seed=dim + k)
        path = path_of(rows.shape[0], dim, k, ROWS)
        assert path.startswith("bf16_tiles/"), path
        check_case(np.ascontiguousarray(X[rows]), C, path, rows=rows, Xd=torch.from_numpy(X).cuda(), tag="c/rows")


def test_tiles_unaligned_x_dim41(monkeypatch):
    force(monkeypatch)
    dim = 41
    for k in KS:
        X, C = M.points(N + 1, dim, k, seed=41 + k)
        Xd = torch.from_numpy(X).cuda()[1:]  # 164 bytes into the allocation
        assert Xd.data_ptr() % 16 != 0
        path = path_of(N, dim, k, X_UNALIGNED)
        assert path.startswith("bf16_tiles/"), path
        check_case(np.ascontiguousarray(X[1:]), C, path, Xd=Xd, tag="c/unaligned")


@pytest.mark.parametrize("dim", [129, 200, 496, 497, 512])
def test_tiles_wide_dims(dim, monkeypatch):
    """496 | 497: the last dim whose four-wave block fits a CU's LDS, the first that runs two waves."""
    force(monkeypatch)
    for k in KS:
        path = path_of(N, dim, k)
        assert path.startswith("bf16_tiles/"), path
        X, C = M.points(N, dim, k, seed=1000 * dim + k)
        check_case(X, C, path, tag="c/wide")


def test_tiles_centres_do_not_fit(monkeypatch):
    """k = 3000 at dim 40: 94 centre tiles of three k-steps are 289 KB of fragments, so neither
    persistent kernel holds them; several centre chunks merge through the keys."""
    force(monkeypatch)
    n, dim, k = 2 * 2000 + 13, 40, 3000
    path = path_of(n, dim, k)
    assert path.startswith("bf16_tiles/") and int(path.split("/")[1].split("x")[1]) > 1, path
    X, C = M.points(n, dim, k, seed=40)
    check_case(X, C, path, tag="c/k3000")


# ---- (d) integer lattices: no tolerance -----------------------------------------------------------
LATTICE_NS = (32, 33, 63, 64, 65, 1000, N)  # N: where the widest fragments of each class still fit
LATTICE_KS = (1, 31, 32, 33, 64, 65)

# (dim, GDD_FORCE token, the path the class is meant to run). The small n take the tiles form (their
# workspace holds no fragments); the class's own kernel runs at n = 1000 with one centre tile (not
# dim 128) and at n = N with two (dim 128: one), the r06 kernel with one, two and three
LATTICE = ([(d, "", "bf16q/w4") for d in (1, 7, 8, 9, 12, 15, 17, 23, 24, 31, 33, 40, 41, 44, 45, 47, 49, 56,
                                          57, 63)] +
           [(d, "bf16_w8", "bf16q/w8") for d in (41, 45, 47)] +
           [(5, "bf16_v1", "bf16p/per1"), (23, "bf16_v1", "bf16p/per3"), (16, "", "bf16p/per2"),
            (32, "", "bf16p/per4"), (48, "", "bf16p/per6"), (64, "", "bf16p/per8"),
            (96, "", "bf16p/per12"), (128, "", "bf16p/per16"), (129, "", "bf16_tiles/"), (512, "", "bf16_tiles/")])


@pytest.mark.parametrize("dim,token,meant", LATTICE)
def test_lattice_exact_nearest(dim, token, meant, monkeypatch):
    """Every form returns a true nearest centre (int64 distances); the r03 and tiles forms the first
    such index, the r06 form any of the tied ones (gdd_bf16.hip header)."""
    force(monkeypatch, *([token] if token else []))
    assert path_of(1000, dim, 32).startswith(meant) or dim == 128  # 8 k-steps: 8,320 bytes of 8,192
    assert path_of(N, dim, 32 if dim == 128 else 64).startswith(meant)
    if meant.startswith("bf16q"):
        assert {path_of(N, dim, k) for k in LATTICE_KS} == {meant}
    for n in LATTICE_NS:
        for k in LATTICE_KS:
            path = path_of(n, dim, k)
            X, C = M.lattice(n, dim, k, seed=dim * 100000 + n * 100 + k)
            lab, _ = assign_bf16(X, C, sq=False)
            d, dmin = M.nearest_exact(X, C)
            assert lab.min() >= 0 and lab.max() < k
            assert np.array_equal(d[np.arange(n), lab], dmin), (path, n, k)
            if M.form_of(path) != "r06":
                assert np.array_equal(lab, d.argmin(1)), (path, n, k)


# ---- (e) the norms given ---------------------------------------------------------------------------
def call_bf16(Xd, Cd, cn2d, n, dim, k):
    lib = _lib.device_lib()
    lab = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    ws = _lib.workspace(lib.gdd_kmeans_assign_ws_bytes(n), "cuda")
    _lib.check(lib.gdd_kmeans_assign_bf16(n, dim, Xd.data_ptr(), None, k, Cd.data_ptr(), _lib.ptr(cn2d),
                                          lab.data_ptr(), None, ws.data_ptr(), ws.numel(),
                                          _lib.stream_ptr("cuda")))
    return lab.cpu().numpy()


@pytest.mark.parametrize("dim,k,token,path", [(23, 96, "", "bf16q/w4"), (45, 96, "bf16_w8", "bf16q/w8"),
                                              (64, 96, "", "bf16p/per8"), (3, 225, "", "bf16q/w4")])
def test_given_norms(dim, k, token, path, monkeypatch):
    """c_norm2 from gdd_row_norms, and NULL: zero violations both ways, the same labels on lattice
    data (where every norm is exact whoever sums it). With NULL the r06 kernel sums the norms itself,
    except at dim 3 with k = 225: 8 centre tiles are past bf16q_norms_fit, so the entry point's
    temporary norms run; the r03 kernel always reads them."""
    force(monkeypatch, *([token] if token else []))
    assert path_of(N, dim, k) == path
    assert M.norms_fit(dim, k) == (dim != 3)
    lib = _lib.device_lib()
    for data in ("points", "lattice"):
        X, C = (M.points if data == "points" else M.lattice)(N, dim, k, seed=dim + k)
        Xd, Cd = torch.from_numpy(X).cuda(), torch.from_numpy(C).cuda()
        cn2d = torch.empty(k, dtype=torch.float32, device="cuda")
        _lib.check(lib.gdd_row_norms(k, dim, Cd.data_ptr(), cn2d.data_ptr(), _lib.stream_ptr("cuda")))
        given = call_bf16(Xd, Cd, cn2d, N, dim, k)
        null = call_bf16(Xd, Cd, None, N, dim, k)
        if data == "lattice":
            assert np.array_equal(given, null)
            d, dmin = M.nearest_exact(X, C)
            assert np.array_equal(d[np.arange(N), given], dmin)
            continue
        for name, lab, cn2 in (("given", given, cn2d.cpu().numpy()), ("null", null, None)):
            viol, und, worst = bf16_check(X, C, lab, path, cn2=cn2)
            print(f"bf16-model e/{name} dim={dim} k={k} path={path} violations={viol} "
                  f"undecided={und:.4f} worst_ratio={worst:.3f}")
            assert viol == 0 and und <= 0.02, (name, viol, und, worst)


# ---- (f) several tiles per wave ---------------------------------------------------------------------
@pytest.mark.parametrize("dim,token,path", [(7, "", "bf16q/w4"), (12, "", "bf16q/w4"), (20, "", "bf16q/w4"),
                                            (41, "", "bf16q/w4"), (57, "", "bf16q/w4"),
                                            (41, "bf16_w8", "bf16q/w8"), (64, "", "bf16p/per8")])
def test_three_tiles_per_wave(dim, token, path, monkeypatch):
    """n = 3 * 262,144 + 17: 24,577 tiles over at most 256 CUs x 32 resident waves, so some wave
    takes three tiles or more: both register sets of the persistent loops are refilled and the
    D = 1 loop of the 8-wave form wraps. The last 17 rows (the partial tile) are checked apart."""
    force(monkeypatch, *([token] if token else []))
    n, k = 3 * 262144 + 17, 40
    assert path_of(n, dim, k) == path
    rng = np.random.default_rng(dim)
    X = rng.standard_normal((n, dim), dtype=np.float32) + rng.integers(0, 5, (n, 1)).astype(np.float32)
    C = X[rng.choice(n, k, replace=False)] + rng.standard_normal((k, dim)).astype(np.float32) * 0.1
    lab, _ = assign_bf16(X, C, sq=False)
    viol, und, worst = bf16_check(X, C, lab, path)
    print(f"bf16-model f{'/' + token if token else ''} n={n} dim={dim} k={k} path={path} violations={viol} "
          f"undecided={und:.4f} worst_ratio={worst:.3f}")
    assert viol == 0 and und <= 0.02, (viol, und, worst)
    assert bf16_check(X[-17:], C, lab[-17:], path)[0] == 0
    assert bf16_check(X[:32], C, lab[:32], path)[0] == 0
