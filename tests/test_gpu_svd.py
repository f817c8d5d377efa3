"""Device truncated SVD (gdd/svd.py, csrc/gdd_svd.hip) on the MI355X: the kernels against numpy fp64,
truncated_svd against np.linalg.svd on the small cases of tests/test_svd_host.py, svd_embeddings
against the reference's captured Ali-Display embeddings, determinism, and the driver's
--svd_backend device.

Bounds. spmm: bit-equal to the ordered numpy loop. gram / tsmm: the dot-product forward bound
|err_ij| <= 2 n 2^-53 sum_r |a_ri| |b_rj| with n the summed index's length. CholeskyQR2:
||VᵀV - I||_max <= 1e-12 for cond(Z) <= 1e3. truncated_svd (tol = 1e-10): |σ̂² - σ²| and the
recomputed residual ||RᵀR v - σ² v|| <= 2 tol σ_1², small-side orthonormality <= 1e-12. Ali-Display
(k = 64): per column |cos| >= 1 - 1e-9 and, signs aligned, max |ours - fixture| <= 5e-6: the smallest
neighbouring gap σ_j² - σ_{j+1}² is about 0.26 against a residual <= 1e-10 σ_1² ~ 1e-7, so
Davis-Kahan gives sin θ <= 4e-7 (1 - cos <= 1e-13) and an element error <= 4e-7 sqrt(σ_1) ~ 2.3e-6
plus fp32 rounding."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svd_ref  # noqa: E402
from golden_util import load  # noqa: E402
from test_svd_host import CASES, TOL  # noqa: E402

pytestmark = pytest.mark.gpu

BS = [1, 17, 96, 128]
ROWS = [1, 63, 1000, 4097]
U53 = 2.0 ** -53


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


# ---- kernel units ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def spmm_matrix():
    """300 x 700: duplicates summed, three empty rows, one completely full row."""
    R = svd_ref.interactions(300, 700, 6000, 11).tolil()
    for r in (5, 100, 299):
        R[r, :] = 0
    R[7, :] = np.random.RandomState(3).randint(1, 4, 700).astype(np.float32)
    R = sp.csr_matrix(R)
    R.eliminate_zeros()
    lens = np.diff(R.indptr)
    assert R.data.max() > 1 and (lens == 0).sum() >= 3 and lens[7] == 700
    return R


@pytest.mark.parametrize("values", [True, False])
@pytest.mark.parametrize("b", BS)
def test_spmm_f64_bit_equal(spmm_matrix, b, values):
    from gdd import svd as S
    R = spmm_matrix
    X = np.random.RandomState(b).standard_normal((700, b))
    A = S.DeviceCSR.from_scipy(R, "cuda", values=values)
    Y = S.spmm_f64(A, dev(X)).cpu().numpy()
    ref = svd_ref.spmm_ordered(R.indptr, R.indices, R.data if values else None, X)
    assert np.array_equal(Y.view(np.uint64), ref.view(np.uint64))
    assert not Y[[5, 100, 299]].any()


def test_spmm_f64_transposed_side(spmm_matrix):
    """Aᵀ from gdd_csr_transpose (entries by ascending original row) through the same kernel."""
    from gdd import svd as S
    R = spmm_matrix
    Rt = sp.csr_matrix(R.T)
    Rt.sort_indices()
    X = np.random.RandomState(0).standard_normal((300, 17))
    Y = S.spmm_f64(S.DeviceCSR.from_scipy(R, "cuda").transpose(), dev(X)).cpu().numpy()
    assert np.array_equal(Y, svd_ref.spmm_ordered(Rt.indptr, Rt.indices, Rt.data, X))


@pytest.fixture(scope="module")
def blocks():
    rs = np.random.RandomState(5)
    return {(n, b): rs.standard_normal((n, b)) for n in ROWS for b in BS}


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("n", ROWS)
def test_gram_f64(blocks, n, b, form):
    from gdd import svd as S
    W = blocks[(n, b)]
    Wd = dev(W)
    G = S.gram_f64(Wd, form).cpu().numpy()
    G2 = S.gram_f64(Wd, form).cpu().numpy()
    bound = 2 * n * U53 * (np.abs(W).T @ np.abs(W))
    err = np.abs(G - W.T @ W)
    print(f"gram n={n} b={b} form={form}: max err/bound {np.max(err / bound):.3g}")
    assert np.all(err <= bound)
    assert np.array_equal(G.view(np.uint64), G.T.view(np.uint64))
    assert np.array_equal(G.view(np.uint64), G2.view(np.uint64))


def test_gram_default_form_is_one_of_the_two(blocks):
    from gdd import svd as S
    Wd = dev(blocks[(1000, 96)])
    G = S.gram_f64(Wd).cpu().numpy()
    assert any(np.array_equal(G, S.gram_f64(Wd, f).cpu().numpy()) for f in (0, 1))


@pytest.mark.parametrize("b", BS)
@pytest.mark.parametrize("n", ROWS)
def test_tsmm_f64(blocks, n, b):
    from gdd import svd as S
    W = blocks[(n, b)]
    Q = np.random.RandomState(n + b).standard_normal((b, b))
    Wd, Qd = dev(W), dev(Q)
    out = S.tsmm_f64(Wd, Qd).cpu().numpy()
    out2 = S.tsmm_f64(Wd, Qd).cpu().numpy()
    bound = 2 * b * U53 * (np.abs(W) @ np.abs(Q))
    err = np.abs(out - W @ Q)
    print(f"tsmm n={n} b={b}: max err/bound {np.max(err / bound):.3g}")
    assert np.all(err <= bound)
    assert np.array_equal(out.view(np.uint64), out2.view(np.uint64))


def _conditioned(n, b, cond, seed):
    rs = np.random.RandomState(seed)
    q1 = np.linalg.qr(rs.standard_normal((n, b)))[0]
    q2 = np.linalg.qr(rs.standard_normal((b, b)))[0]
    return (q1 * np.logspace(0, np.log10(cond), b)) @ q2


@pytest.mark.parametrize("n,b", [(1000, 1), (63, 17), (1000, 96), (4097, 128), (128, 128)])
def test_cholqr2_orthonormal(n, b):
    from gdd import svd as S
    Z = _conditioned(n, b, 1e3 if b > 1 else 1.0, n + b)
    V, flag = S.cholqr2_f64(dev(Z))
    V = V.cpu().numpy()
    orth = np.max(np.abs(V.T @ V - np.eye(b)))
    print(f"cholqr2 n={n} b={b}: orth {orth:.3g}")
    assert int(flag.item()) == 0
    assert orth <= 1e-12
    # the same column space: projecting Z on V loses nothing
    assert np.max(np.abs(V @ (V.T @ Z) - Z)) <= 1e-10 * np.max(np.abs(Z))


@pytest.mark.parametrize("b", [17, 128])
def test_chol_inv_vs_restatement(b):
    from gdd import svd as S
    Z = _conditioned(500, b, 1e3, b)
    G = Z.T @ Z
    G = (G + G.T) / 2
    Rinv, flag = S.chol_inv_f64(dev(G))
    Rinv = Rinv.cpu().numpy()
    ref, bad = svd_ref.chol_inv(G)
    assert int(flag.item()) == 0 and not bad
    assert np.array_equal(np.triu(Rinv), Rinv)
    assert np.max(np.abs(Rinv.T @ G @ Rinv - np.eye(b))) <= 1e-9  # cond(G) = 1e6
    assert np.max(np.abs(Rinv - ref)) <= 1e-9 * np.max(np.abs(ref))


@pytest.mark.parametrize("b", [17, 128])
def test_breakdown_flag_for_equal_columns(b):
    from gdd import svd as S
    Z = np.random.RandomState(b).standard_normal((300, b))
    Z[:, b - 3] = Z[:, 2]
    Zd = dev(Z)
    V, flag = S.cholqr2_f64(Zd)
    assert int(flag.item()) == 1
    G = Z.T @ Z
    Rinv, flag = S.chol_inv_f64(dev((G + G.T) / 2))
    assert int(flag.item()) == 1 and np.array_equal(Rinv.cpu().numpy(), np.eye(b))


# ---- truncated_svd -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_truncated_svd_small_cases(name):
    from gdd import svd as S
    make, k = CASES[name]
    R = make()
    U, Sg, V, info = S.truncated_svd(R, k)
    f = svd_ref.check_factors(R, k, U, Sg, V, TOL)
    print(name, info, f)
    assert U.shape == (R.shape[0], k) and V.shape == (R.shape[1], k) and Sg.shape == (k,)
    assert info["block"] == svd_ref.block_size(R.shape, k)
    assert f["sigma2_err"] <= f["bound"]
    assert f["orth"] <= 1e-12
    assert f["residual"] <= f["bound"]
    assert info["host_qr_redone"] == (1 if name == "rank10" else 0)
    small = U if R.shape[1] > R.shape[0] else V
    assert np.all(small[np.argmax(np.abs(small), axis=0), np.arange(k)] > 0)


def test_block_limit_names_the_host_backend():
    from gdd import svd as S
    with pytest.raises(ValueError, match="host"):
        S.truncated_svd(svd_ref.interactions(400, 300, 3000, 6), 100)


# ---- real data ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alidisplay():
    z = load("golden_alidisplay.npz")
    nu, ni = z["user_emb"].shape[0], z["item_emb"].shape[0]
    R = sp.coo_matrix((np.ones(len(z["train_u"]), np.float32), (z["train_u"], z["train_i"])),
                      shape=(nu, ni)).tocsr()
    return R, z["user_emb"], z["item_emb"]


def test_alidisplay_vs_reference_embeddings(alidisplay):
    from gdd import svd as S
    R, fu, fi = alidisplay
    assert fu.shape == (17730, 64) and fi.shape == (10036, 64)
    ue, ie = S.svd_embeddings(R, 64)
    assert ue.dtype == np.float32 and ie.dtype == np.float32
    for ours, fx, side in ((ue, fu, "user"), (ie, fi, "item")):
        o, f = ours.astype(np.float64), fx.astype(np.float64)
        dots = (o * f).sum(0)
        cos = np.abs(dots) / (np.linalg.norm(o, axis=0) * np.linalg.norm(f, axis=0))
        elem = np.max(np.abs(o * np.sign(dots) - f))
        print(f"alidisplay {side}: max 1-|cos| {np.max(1 - cos):.3g}, max elem {elem:.3g}")
        assert np.all(cos >= 1 - 1e-9)
        assert elem <= 5e-6
    # the same sign flips on both sides
    assert np.array_equal(np.sign((ue.astype(np.float64) * fu).sum(0)),
                          np.sign((ie.astype(np.float64) * fi).sum(0)))


# ---- determinism -------------------------------------------------------------------------------
def test_embeddings_bit_identical_and_seed_free_sigma():
    from gdd import svd as S
    R = svd_ref.interactions(300, 200, 1500, 1)
    a, b = S.svd_embeddings(R, 16), S.svd_embeddings(R, 16)
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    _, S0, _, i0 = S.truncated_svd(R, 16, seed=42)
    _, S1, _, i1 = S.truncated_svd(R, 16, seed=7)
    assert np.max(np.abs(S0 ** 2 - S1 ** 2)) <= 2 * TOL * S0[0] ** 2


# ---- driver ------------------------------------------------------------------------------------
def test_driver_svd_backend_device(tmp_path, capsys):
    from gdd import distill_recsys as D
    rs = np.random.RandomState(0)
    nu, ni, E = 300, 200, 4000
    u, i = rs.randint(0, nu, E), rs.randint(0, ni, E)
    u[:nu], i[:ni] = np.arange(nu), np.arange(ni)  # every id occurs
    os.makedirs(tmp_path / "tiny")
    cut = {"train": slice(0, 3200), "valid": slice(3200, 3600), "test": slice(3600, E)}
    for name, s in cut.items():
        np.savetxt(tmp_path / "tiny" / f"{name}.txt", np.stack([u[s], i[s]], 1), fmt="%d")
    argv = ["--data_dir", str(tmp_path), "--dataset", "tiny", "--svd_backend", "device", "--refine_epochs", "2",
            "--svd_dim", "16", "--embed_dim", "16", "--batch_size", "256", "--seed", "42"]
    tm = {}
    D.run(D.parse_args(argv), out_root=str(tmp_path / "out"), timings=tm)
    out = capsys.readouterr().out.splitlines()
    assert "[cluster] computing SVD embeddings..." in out
    assert any(l.startswith("[refine] ep=0002") for l in out)
    d = tmp_path / "out" / "distilled_recsys" / "tiny"
    assert np.load(d / "u2cu.npy").shape == (nu,) and np.load(d / "i2ci.npy").shape == (ni,)
    assert os.path.exists(d / "condensed_graph.npz")
    assert tm["svd_s"] > 0
