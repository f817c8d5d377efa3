"""The contrastive loss and the layer's ablation switches as dense definitions in CPU torch (fp64 by
default), the loader of tests/golden/rankformer_cl.npz (recorded from the reference by
tools/make_golden_rankformer_cl.py) and the forward error bounds the device tests use.

Definitions, for ``A``, ``Y`` of shape ``B × d`` and ``ℓ = A Yᵀ / tau``: ``loss_r = lse_r − ℓ_rr``,
``P = softmax(ℓ)`` by rows, ``R = P Y``, ``C = (G ∘ P)ᵀ A`` for a per-row ``G``.

Bounds (``u = 2⁻²⁴``; the kernels take fp32 ``A``, ``Y`` as exact). Write ``S_r = max_c Σ_f |A_rf||Y_cf|``.

* A logit is a ``d``-term fmaf chain times the fp32 ``1/tau``: ``d`` roundings of the chain, one of the
  product, one of ``1/tau`` itself: ``|ℓ̂ − ℓ| ≤ ε_r = (d + 2) u S_r / tau``.
* ``lse_r = m + log Σ_c exp(ℓ̂_rc − m)`` is exact in ``m``. Each term carries the logit's ``ε_r``, the
  subtraction's ``u |ℓ̂ − m| ≤ 2 u S_r / tau ≤ ε_r`` and ``expf``'s 2u; ``B`` positive terms add up with
  at most ``(B − 1) u`` relative error in any order, the rescaling of the running sum (at most one per
  tile of 32 columns, 3u each) at most ``0.1 B u``; ``logf`` and the two final additions add
  ``3u |lse| ≤ 3u (S_r / tau + ln B)``, of which the first part is below ``ε_r`` and the second below
  ``0.9 B u + 10u``. With the diagonal logit's own ``ε_r`` that is ``4 ε_r + 2 B u + 16 u``, and the
  final subtraction rounds once more::

      |loss err_r| ≤ rel_r + u |loss_r|,      rel_r = 2u [2 (d + 2) S_r / tau + B + 8]

* ``P̂_rc = exp(ℓ̂_rc − lsê_r)`` has relative error ``rel_r``; the ``B``-term chain that adds
  ``P̂_rc Y_cf`` (and the rescaling and the final division) adds ``2 B u`` relative to the sum of
  magnitudes: ``|R err_rf| ≤ (rel_r + 2 B u) Σ_c P_rc |Y_cf|``, and in the same way
  ``|C err_cf| ≤ Σ_r (rel_r + 2 B u) |G_r| P_rc |A_rf|``.
* The gradients ``dA_r = G_r (R_r − Y_r) / tau`` and ``dY_c = (C_c − G_c A_c) / tau`` add one
  subtraction and two products (4u of the terms' magnitudes) to the scaled bounds of ``R`` and ``C``.
* :func:`infonce` normalises in fp32 first: each element of ``x̂``, ``ŷ`` has relative error at most
  ``(d + 3) u`` (``d`` squares summed, the root, the division), which moves a logit by at most
  ``2 (d + 3) u S_r / tau``: the chain length ``d + 2`` becomes ``3d + 8`` (``chain`` below), and the
  gradient goes back through the normalisation's Jacobian ``(I − x̂ x̂ᵀ) / ‖x‖`` with ``(d + 8) u`` of
  rounding of its own.

Every bound is first order in ``u`` and has no fitted constant; the torch fp32 formula on a CPU sits
at about 0.02 of the row bound."""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN_CL = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rankformer_cl.npz")
NCE_CASES = ("nce65", "nce300")
LAYER_CASES = tuple(f"{b}_{t}" for b in ("small", "wide") for t in ("neg", "bench", "norm", "all"))
U = 2.0 ** -24


def load_cl_case(name):
    """One case of the fixture, keys without the case prefix."""
    z = np.load(GOLDEN_CL)
    return {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + ".")}


# ---- dense definitions ---------------------------------------------------------------------------
def logits(A, Y, tau):
    return (A @ Y.t()) / tau


def dense_rows(A, Y, tau):
    """The per-row losses lse_r − ℓ_rr [B]."""
    L = logits(A, Y, tau)
    return torch.logsumexp(L, 1) - torch.diagonal(L)


def dense_lse_diag(A, Y, tau):
    L = logits(A, Y, tau)
    return torch.logsumexp(L, 1), torch.diagonal(L).clone()


def dense_P(A, Y, tau):
    return torch.softmax(logits(A, Y, tau), 1)


def dense_R(A, Y, tau):
    return dense_P(A, Y, tau) @ Y


def dense_C(A, Y, tau, G):
    return (G.unsqueeze(1) * dense_P(A, Y, tau)).t() @ A


def dense_infonce(x, y, tau=0.15, b_cos=True):
    """model.py:10-24."""
    if b_cos:
        x, y = F.normalize(x), F.normalize(y)
    return dense_rows(x, y, tau).mean()


def dense_rankformer(x, M, alpha=2.0, clamp=0.0, del_neg=False, del_benchmark=False, del_omega_norm=False,
                     rows=None):
    """rankformer_ref.dense_rankformer with the three switches of rec.py:219-221 and :263-274.
    ``rows`` (a bool mask over the n + m outputs) returns those rows only, the others never divided:
    a 0/0 row (an item without users under ``del_neg`` at clamp 0, NaN in the reference as well)
    would otherwise put NaN into every gradient of a dense definition."""
    n, m = M.shape
    xh = F.normalize(x)
    xu, xi, vu, vi = xh[:n], xh[n:], x[:n], x[n:]
    N = 1 - M
    dp = M.sum(1, keepdim=True).clamp(min=1)
    dn = (m - M.sum(1, keepdim=True)).clamp(min=1)
    s = xu @ xi.t()
    bp = (M * s).sum(1, keepdim=True) / dp
    bn = (N * s).sum(1, keepdim=True) / dn
    bpz, bnz = (torch.zeros_like(bp), torch.zeros_like(bn)) if del_benchmark else (bp, bn)
    Op = M * (s - bnz + alpha) / dp
    Om = N * (s - bpz - alpha) / dn
    d1 = (bp - bnz + alpha).clamp(min=clamp)  # the first term of each user denominator keeps its b
    d2 = (bpz - bn + alpha).clamp(min=clamp)
    if del_neg:
        num_u, num_i = Op @ vi, Op.t() @ vu
        den_u, den_i = d1, Op.sum(0).clamp(min=clamp)
    else:
        num_u, num_i = (Op + Om) @ vi, (Op + Om).t() @ vu
        den_u, den_i = d1 + d2, Op.sum(0).clamp(min=clamp) + (-Om.sum(0)).clamp(min=clamp)
    num, den = torch.cat([num_u, num_i], 0), torch.cat([den_u[:, 0], den_i], 0).unsqueeze(1)
    if rows is not None:
        num, den = num[rows], den[rows]
    return num if del_omega_norm else num / den


# ---- bounds (module docstring) -------------------------------------------------------------------
def rel_factor(A, Y, tau, chain=None):
    """rel_r [B] for fp64 copies of the inputs; ``chain`` is d + 2 unless the caller's path is longer."""
    B, d = A.shape
    chain = d + 2 if chain is None else chain
    S = (A.abs() @ Y.abs().t()).max(1).values
    return 2 * U * (2 * chain * S / tau + B + 8)


def bound_rows(A, Y, tau, chain=None):
    return rel_factor(A, Y, tau, chain) + U * dense_rows(A, Y, tau).abs()


def bound_R(A, Y, tau, chain=None):
    B = A.shape[0]
    return (rel_factor(A, Y, tau, chain) + 2 * U * B).unsqueeze(1) * (dense_P(A, Y, tau) @ Y.abs())


def bound_C(A, Y, tau, G, chain=None):
    B = A.shape[0]
    w = (rel_factor(A, Y, tau, chain) + 2 * U * B) * G.abs()
    return (w.unsqueeze(1) * dense_P(A, Y, tau)).t() @ A.abs()


def bound_dA(A, Y, tau, G, chain=None):
    mag = dense_P(A, Y, tau) @ Y.abs() + Y.abs()
    return (G.abs() / tau).unsqueeze(1) * (bound_R(A, Y, tau, chain) + 4 * U * mag)


def bound_dY(A, Y, tau, G, chain=None):
    mag = (G.abs().unsqueeze(1) * dense_P(A, Y, tau)).t() @ A.abs() + G.abs().unsqueeze(1) * A.abs()
    return (bound_C(A, Y, tau, G, chain) + 4 * U * mag) / tau


def through_normalize(x, b):
    """|J| b for the Jacobian J = (I − x̂ x̂ᵀ)/‖x‖ of F.normalize at x, b ≥ 0 elementwise."""
    nrm = x.norm(dim=1, keepdim=True).clamp(min=1e-12)
    xh = (x / nrm).abs()
    return (b + xh * (xh * b).sum(1, keepdim=True)) / nrm


def bounds_infonce(x, y, tau):
    """(loss bound, bound of d loss / dx, of d loss / dy) for :func:`dense_infonce` with ``b_cos``
    against a device path that normalises in fp32."""
    B, d = x.shape
    A, Y = F.normalize(x), F.normalize(y)
    chain = 3 * d + 8
    rows = dense_rows(A, Y, tau)
    loss_b = float(bound_rows(A, Y, tau, chain).mean() + (B + 1) * U * rows.abs().mean())
    G = torch.full((B,), 1.0 / B, dtype=x.dtype)
    P = dense_P(A, Y, tau)
    gA = (G / tau).unsqueeze(1) * (P @ Y - Y)
    gY = ((G.unsqueeze(1) * P).t() @ A - G.unsqueeze(1) * A) / tau
    bA = bound_dA(A, Y, tau, G, chain) + (d + 3) * U * (G / tau).unsqueeze(1) * (P @ Y.abs() + Y.abs())
    bY = bound_dY(A, Y, tau, G, chain) + (d + 3) * U * ((G.unsqueeze(1) * P).t() @ A.abs()
                                                        + G.unsqueeze(1) * A.abs()) / tau
    bx = through_normalize(x, bA) + (d + 8) * U * through_normalize(x, gA.abs())
    by = through_normalize(y, bY) + (d + 8) * U * through_normalize(y, gY.abs())
    return loss_b, bx, by


# ---- inputs the device tests share ---------------------------------------------------------------
def unit_rows(B, d, seed):
    """(A, Y) fp32: A rows of unit norm (in fp32 rounding), Y a perturbed copy, renormalised."""
    g = torch.Generator().manual_seed(seed)
    A = F.normalize(torch.randn(B, d, generator=g, dtype=torch.float64)).float()
    Y = F.normalize(A.double() + 0.3 * torch.randn(B, d, generator=g, dtype=torch.float64) / d ** 0.5).float()
    return A, Y


def planted(B=130, d=64, late=False, seed=5):
    """The running-maximum case (tau = 0.01): for every third row r, Y[(r + 1) % B] = A[r], so the
    off-diagonal logit is 100. ``late``: the planted columns are the last 30 (Y[B − 1 − k] = A[r] for the k-th such row
    r < B − 32): at B = 130 the kernel's last, partial tile of two columns and the full tile before
    it, so the maximum rises at the very end of the stream."""
    A, Y = unit_rows(B, d, seed)[0], unit_rows(B, d, seed + 1)[0]  # independent: the diagonal is small
    rows = list(range(0, B, 3))
    if late:
        tail = [c for c in range(B - 1, B - 1 - 30, -1)]
        for r, c in zip([r for r in rows if r < B - 32], tail):
            Y[c] = A[r]
    else:
        for r in rows:
            Y[(r + 1) % B] = A[r]
    return A, Y
