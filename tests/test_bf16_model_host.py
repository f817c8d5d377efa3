"""The bf16 labels pass's reference (tests/bf16_model.py) tested on the CPU: the fp64 argmin of its own
scores never violates it, and it flags numpy emulations of subtly wrong kernels — among them one the
suite's earlier 2^-7 bound (kept in test_gpu_kmeans.py for what it says about the distance to the
fp32 labels) accepts on every row."""
import numpy as np
import pytest

import bf16_model as M

SHAPES = [(9000, 45, 100), (20000, 23, 200), (20000, 57, 333)]


def make(n, dim, k):
    """The generator of test_assign_bf16_within_rounding: randn + an integer offset per row, the
    centres points plus 0.1 randn."""
    rng = np.random.default_rng(n + k)
    X = (rng.standard_normal((n, dim)) + rng.integers(0, 5, (n, 1))).astype(np.float32)
    C = X[rng.choice(n, k, replace=False)] + rng.standard_normal((k, dim)).astype(np.float32) * 0.1
    return X, C


def old_bound_failures(X, C, b):
    """Rows the earlier property test rejects: label b differs from the fp64 label a and
    d[b] - d[a] > 2 2^-7 ||x|| (||c_a|| + ||c_b||) + 1e-3 (1 + d[a])."""
    X64, C64 = X.astype(np.float64), C.astype(np.float64)
    d = (X64 ** 2).sum(1)[:, None] + (C64 ** 2).sum(1)[None] - 2 * X64 @ C64.T
    a = d.argmin(1)
    i = np.arange(X.shape[0])
    xn, cn = np.linalg.norm(X64, axis=1), np.linalg.norm(C64, axis=1)
    bound = 2 * 2.0 ** -7 * xn * (cn[a] + cn[b]) + 1e-3 * (1 + d[i, a])
    return int(((a != b) & (d[i, b] - d[i, a] > bound)).sum()), float((a == b).mean())


@pytest.fixture(scope="module", params=SHAPES, ids=lambda s: "x".join(map(str, s)))
def case(request):
    X, C = make(*request.param)
    Xb, Cb = M.round_bf16(X), M.round_bf16(C)
    cn = (C.astype(np.float64) ** 2).sum(1)
    return X, C, Xb, Cb, cn


def test_round_bf16_is_nearest_even():
    a = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0,
                  257.0, 0.0], np.float32)
    want = [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0, 256.0, 0.0]  # ties to even
    got = M.round_bf16(a)
    assert got.dtype == np.float64 and got.tolist() == want


@pytest.mark.parametrize("form", M.FORMS)
def test_model_argmin_has_no_violations(case, form):
    X, C, _, _, _ = case
    lab = M.scores(X, C, None).argmin(1)
    viol, und, worst = M.check_labels(X, C, None, lab, form)
    assert viol == 0 and worst == 0.0
    assert und <= 0.02  # the generator leaves the check decisive on all but a few rows
    E = M.slack(X, C, None, form)
    assert E.shape == (X.shape[0],) and (E > 0).all()
    if form != "r06":  # r06 alone carries the shift's magnitude and the key's five bits
        assert (E < M.slack(X, C, None, "r06")).all()


def test_given_norms_are_taken_as_passed(case):
    X, C, Xb, Cb, _ = case
    cn32 = (C.astype(np.float64) ** 2).sum(1).astype(np.float32)
    s = M.scores(X, C, cn32)
    assert np.array_equal(s, cn32.astype(np.float64)[None] / 2 - Xb @ Cb.T)
    # no term for the kernel's own norm sum when the norms are given
    assert (M.slack(X, C, cn32, "r03") < M.slack(X, C, None, "r03")).all()


def _wrong_kernels(Xb, Cb, cn):
    n, k = Xb.shape[0], Cb.shape[0]
    good = cn[None] / 2 - Xb @ Cb.T
    Xw = Xb.copy()
    Xw[:, -1] = 0
    yield "last feature dropped", (cn[None] / 2 - Xw @ Cb.T).argmin(1)
    yield "last centre never considered", good[:, :k - 1].argmin(1)
    yield "norms of the bf16-rounded centres", ((Cb ** 2).sum(1)[None] / 2 - Xb @ Cb.T).argmin(1)
    lab = good.argmin(1)
    t0 = (n - 1) // 32 * 32  # the last 32-tile (partial unless n % 32 == 0) labelled from the one before
    lab[t0:] = lab[t0 - 32:t0 - 32 + (n - t0)]
    yield "row tail labelled from the previous tile", lab


def test_wrong_kernels_are_flagged(case):
    X, C, Xb, Cb, cn = case
    for name, lab in _wrong_kernels(Xb, Cb, cn):
        for form in M.FORMS:
            viol, _, worst = M.check_labels(X, C, None, lab, form)
            assert viol > 0 and worst > 2, (name, form)


def test_bf16_norms_pass_the_old_bound_and_fail_the_model(case):
    """Why the reference exists: a kernel that takes ||c||^2 from the bf16-rounded centres agrees
    with the fp32 labels on ~99 % of rows, the 2^-7 bound accepts every wrong label, the model
    flags more than 100."""
    X, C, Xb, Cb, _ = case
    lab = ((Cb ** 2).sum(1)[None] / 2 - Xb @ Cb.T).argmin(1)
    old, agree = old_bound_failures(X, C, lab)
    assert agree >= 0.95  # the old test's other condition holds too
    assert old == 0
    viol, _, _ = M.check_labels(X, C, None, lab, "r06")  # the widest slack of the three
    assert viol > 100


def test_check_labels_chunks_rows(monkeypatch):
    X, C = make(3000, 7, 70)
    lab = M.scores(X, C, None).argmin(1)
    lab[::50] = (lab[::50] + 1) % 70
    whole = M.check_labels(X, C, None, lab, "r03")
    monkeypatch.setattr(M, "_CHUNK_ELEMS", 70 * 257)
    assert M.check_labels(X, C, None, lab, "r03") == whole
    assert whole[0] > 0
