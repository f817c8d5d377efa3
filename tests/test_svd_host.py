"""CPU checks of the device truncated SVD's algorithm: its numpy restatement (tests/svd_ref.py)
against np.linalg.svd on small dense-able interaction matrices, and the host-side argument checks
of gdd.svd (no GPU needed).

Bounds (tol = 1e-10, the default): |σ̂_j² - σ_j²| <= 2 tol σ_1² (Weyl's bound for the converged
residual, a factor 2 for rounding) and ||VᵀV - I||_max <= 1e-12 on the iterated (smaller) side."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import svd_ref  # noqa: E402
from gdd import svd as gsvd  # noqa: E402

TOL = 1e-10

# (name, matrix, k): shared by tests/test_gpu_svd.py
CASES = {
    "base": (lambda: svd_ref.interactions(300, 200, 1500, 1), 16),
    "wide": (lambda: svd_ref.interactions(97, 131, 700, 2), 64),      # roles swap, b clamps to 97
    "clamp": (lambda: svd_ref.interactions(40, 33, 300, 3), 32),      # b clamps to 33
    "rank10": (lambda: svd_ref.low_rank_rows(40, 33, 10, 6, 4), 16),  # rank < b: the breakdown path
}


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_vs_dense_svd(name):
    make, k = CASES[name]
    R = make()
    U, S, V, info = svd_ref.truncated_svd(R, k)
    f = svd_ref.check_factors(R, k, U, S, V, TOL)
    print(name, info, f)
    assert U.shape == (R.shape[0], k) and V.shape == (R.shape[1], k) and S.shape == (k,)
    assert np.all(np.diff(S) <= 0)
    assert f["sigma2_err"] <= f["bound"]
    assert f["orth"] <= 1e-12
    assert info["residual"] <= TOL * S[0] ** 2 * (1 + 1e-12)
    if name == "rank10":
        assert info["host_qr_redone"] == 1
        assert np.all(S[10:] <= 1e-6 * S[0])
    else:
        assert info["host_qr_redone"] == 0
    assert info["block"] == gsvd.block_size(R.shape, k)


def test_sign_convention_and_scaling():
    R = svd_ref.interactions(300, 200, 1500, 1)
    U, S, V, _ = svd_ref.truncated_svd(R, 16)
    top = np.argmax(np.abs(V), axis=0)
    assert np.all(V[top, np.arange(16)] > 0)
    ue, ve = svd_ref.svd_embeddings(R, 16)
    assert ue.dtype == np.float32 and ve.dtype == np.float32
    assert np.array_equal(ve, (V * np.sqrt(np.maximum(S, 1e-12))).astype(np.float32))
    # the factors reproduce R's best rank-16 approximation
    D = np.asarray(R.todense(), np.float64)
    u, s, vt = np.linalg.svd(D, full_matrices=False)
    assert np.max(np.abs((U * S) @ V.T - (u[:, :16] * s[:16]) @ vt[:16])) <= 1e-6


def test_seed_changes_start_not_sigma():
    R = svd_ref.interactions(300, 200, 1500, 1)
    _, S0, _, _ = svd_ref.truncated_svd(R, 16, seed=42)
    _, S1, _, _ = svd_ref.truncated_svd(R, 16, seed=7)
    assert np.max(np.abs(S0 ** 2 - S1 ** 2)) <= 2 * TOL * S0[0] ** 2


def test_chol_inv_restatement():
    rs = np.random.RandomState(0)
    Z = rs.standard_normal((200, 33))
    Rinv, bad = svd_ref.chol_inv(Z.T @ Z)
    assert not bad and np.allclose(np.triu(Rinv), Rinv)
    V = Z @ Rinv
    assert np.max(np.abs(V.T @ V - np.eye(33))) <= 1e-12
    Z[:, 5] = Z[:, 9]
    assert svd_ref.chol_inv(Z.T @ Z)[1]


def test_spmm_ordered_is_the_plain_loop():
    R = svd_ref.interactions(30, 20, 200, 5)
    X = np.random.RandomState(1).standard_normal((20, 3))
    Y = svd_ref.spmm_ordered(R.indptr, R.indices, R.data, X)
    ref = np.zeros((30, 3))
    for r in range(30):
        for p in range(R.indptr[r], R.indptr[r + 1]):
            for c in range(3):
                ref[r, c] = ref[r, c] + np.float64(R.data[p]) * X[R.indices[p], c]
    assert np.array_equal(Y, ref)


def test_device_block_limit_raises_before_touching_the_device():
    R = svd_ref.interactions(400, 300, 3000, 6)
    with pytest.raises(ValueError, match="host"):
        gsvd.truncated_svd(R, 100)  # b = 164 > 128
    with pytest.raises(ValueError):
        gsvd.truncated_svd(R, 300)  # k must be below min(shape)
    with pytest.raises(ValueError):
        gsvd.svd_embeddings(svd_ref.interactions(1, 5, 3, 0), 64)
    assert gsvd.block_size((97, 131), 64) == 97 and gsvd.block_size((17730, 10036), 64) == 128
    from gdd import _lib
    assert _lib.load().gdd_svd_max_block() == gsvd.MAX_BLOCK  # host-only query


def test_driver_flag_defaults_to_host():
    from gdd import distill_recsys as D
    assert D.parse_args([]).svd_backend == "host"
    assert D.parse_args(["--svd_backend", "device"]).svd_backend == "device"
    with pytest.raises(SystemExit):
        D.parse_args(["--svd_backend", "other"])
    with pytest.raises(ValueError):
        D.compute_svd_embeddings(svd_ref.interactions(30, 20, 100, 0), 8, 42, backend="other")
