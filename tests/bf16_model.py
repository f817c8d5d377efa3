"""High-precision model of the bf16 labels pass (gdd_kmeans_assign_bf16) — numpy and torch on the
CPU only: no GPU call, no oracle import.

What the kernels order by. All three kernel forms round the operands of the dot products to bf16
(nearest even), multiply exactly (two 8-bit significands: 16 bits, exact in fp32) and accumulate in
fp32. With x~ = bf16(x), c~ = bf16(c) and the fp32 norms cn2 exactly as the kernel reads them, each
form picks the centre with the smallest

    s[i, c] = cn2[c] / 2 - sum_f x~[i, f] c~[c, f]                                  (scores)

evaluated in fp32:
  * "r03" (k_assign_bf16p) and "tiles" (k_assign_bf16) compute d = fma(-2, acc, cn2[c]) = 2 s from
    an MFMA chain acc that starts at zero, first minimum;
  * "r06" (k_assign_bf16q) starts the chain at -cn2[c] / 2 and adds, in a free K slot, the per-point
    shift -(0.53125 ||x~||^2 + 2^-100) rounded to bf16, so acc = -(s + shift_i); the shift is the
    same for every centre of a point and reorders nothing. The argmin runs on acc's bits with the
    in-tile centre index in the five low significand bits.

The slack E[i] (slack), derived, not tuned. Let

    S[i] = max_c ( cn2[c] / 2 + sum_f |x~[i, f] c~[c, f]| + [r06] 0.54 ||x~[i]||^2 )

the largest sum of the magnitudes of the terms any centre's chain adds for point i (r06's shift:
0.53125 ||x~||^2 summed in fp32 and rounded to bf16, at most 0.53125 (1 + 2^-8)(1 + 2^-21) < 0.54).
  1. The chain adds m = 16 NST + 1 terms (NST = ceil(dim / 16) MFMA steps of 16 products, and the
     starting value). In whatever order or grouping the MFMA adds them, m terms take fewer than m
     additions, each rounding or truncating (2^-23 relative at most, where nearest rounding gives
     2^-24) a partial sum of magnitude at most S: the computed acc is within m 2^-23 S[i] of the
     exact value (first order; the products themselves are exact).
  2. r06: clearing five of the 24 significand bits moves a key by less than 2^-18 |acc| <= 2^-18 S.
     r03 and tiles: the final fma rounds once, 2^-24 |d| with |d| / 2 <= S.
  3. cn2 = None: the model takes the norms of the unrounded fp32 centres in fp64, the kernel sums
     them in fp32. The r06 kernel's own sum (fma chains of 8 features, then the partial sums in
     order) applies at most min(dim, 7 + ceil(dim / 8)) <= dim roundings of 2^-24 to sums below
     cn2[c]; the numpy-order sum of the other forms (mul + add, four lanes) at most
     dim / 4 + 3 <= dim (dim >= 4; dim of them below). Halved: dim 2^-24 max_c cn2[c] / 2.

    E[i] = (m 2^-23 + {r06: 2^-18, r03 and tiles: 2^-24}) S[i] + [cn2 None] dim 2^-24 max_c cn2[c] / 2

bounds the error of every centre's computed value for point i, in the units of s. A kernel that
returns label b therefore saw computed(b) <= computed(best), so s[i, b] - min_c s[i, c] <= 2 E[i];
anything larger is a wrong label (check_labels: a violation). Where the model's own best and second
best lie within 2 E[i] either may be returned: such a row is "undecided" and checks nothing beyond
that bound.
"""
import numpy as np
import torch

FORMS = ("r06", "r03", "tiles")
_CHUNK_ELEMS = 1 << 22  # rows x centres per chunk: 32 MiB of fp64 per temporary


def form_of(path):
    """The model's form name for a gdd_kmeans_assign_path string."""
    return {"bf16q": "r06", "bf16p": "r03", "bf16_tiles": "tiles"}[path.split("/")[0]]


def norms_fit(dim, k):
    """bf16q_norms_fit (gdd_bf16.hip): the r06 kernel sums ||c||^2 itself when no norms are given;
    otherwise, and for the other forms, the entry point runs the numpy-order row norms first."""
    return (k + 31) // 32 * 32 * 2 * ((dim + 15) // 16) <= 4 * (32 * dim + 16)


def points(n, dim, k, seed):
    """The suite's bf16 test data: X = randn + an integer offset per row, the centres k of the points
    plus 0.1 randn — centres sit among the points, so near-ties of every size occur.

    Two widths need another generator to keep the model decisive (undecided share <= 0.02), both
    measured with the model alone on the CPU:
      * dim 1: 96 centres on a line leave 5-10 % of random points within 2 E of a midpoint (E is
        relative to the largest centre's terms, the gaps to the centres' spacing, and rounding a
        centre to bf16 moves the midpoints by more than the spacing), so the centres are an evenly
        spaced, shuffled lattice of multiples of 1/8 (exact in bf16) and the points are jittered
        around them, at most 0.2 of the spacing;
      * dim > 128: with 16 dim + 1 accumulated terms E grows like dim^2 while the gaps between iid
        rows grow like sqrt(dim) (6-8 % undecided at 512); rows of intrinsic rank 8 (randn(n, 8) @
        randn(8, dim), the same offset) keep gaps and E in proportion (below 1.2 %)."""
    rng = np.random.default_rng(seed)
    if dim == 1:
        C0 = (rng.permutation(k) - (k - 1) / 2) * 0.25
        X = (C0[rng.integers(0, k, n)] + rng.uniform(-0.2, 0.2, n) * 0.25).astype(np.float32)[:, None]
        C = C0.astype(np.float32)[:, None]
        return X, C
    if dim > 128:
        X = rng.standard_normal((n, 8)) @ rng.standard_normal((8, dim))
    else:
        X = rng.standard_normal((n, dim))
    X = (X + rng.integers(0, 5, (n, 1))).astype(np.float32)
    C = X[rng.choice(n, k, replace=k > n)] + rng.standard_normal((k, dim)).astype(np.float32) * 0.1
    return X, C


def lattice(n, dim, k, seed):
    """Integers in [-3, 3]: bf16 rounding is exact and every partial sum is an integer or
    half-integer below 2^14 (dim <= 512), with the r06 form (dim <= 63) a multiple of 2^-5 below
    2^11 (its shift, 17/32 ||x||^2 <= 302 rounded to bf16, stays a multiple of 2^-5; the key keeps
    19 significand bits), so the fp32 accumulation is exact in any order and the nearest centres
    are known in int64. Row 0 is all zero (the r06 shift is then -2^-100, absorbed by every centre
    but the zero one, which it keeps negative); centre k // 2 is all zero; centres repeat inside a lane half (1, 2),
    across the halves (1, 4), across centre tiles (5, 32; 1, k - 1)."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-3, 4, (n, dim)).astype(np.float32)
    C = rng.integers(-3, 4, (k, dim)).astype(np.float32)
    X[0] = 0
    if k > 2:
        C[2] = C[1]
    if k > 4:
        C[4] = C[1]
    if k > 32:
        C[32] = C[5]
    if k > 1:
        C[k - 1] = C[1 if k > 2 else 0]
    C[k // 2] = 0
    return X, C


def nearest_exact(X, C):
    """(d, dmin): the int64 squared distances [n, k] of lattice data and their row minima."""
    Xi, Ci = X.astype(np.int64), C.astype(np.int64)
    d = (Xi ** 2).sum(1)[:, None] + (Ci ** 2).sum(1)[None] - 2 * Xi @ Ci.T
    return d, d.min(1)


def round_bf16(a):
    """fp32 -> bf16 (nearest even), returned as float64."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    return torch.from_numpy(a).bfloat16().double().numpy()


def _norms(C, cn2):
    if cn2 is None:
        return (np.asarray(C, np.float64) ** 2).sum(1)
    cn2 = np.asarray(cn2)
    assert cn2.dtype == np.float32 and cn2.shape == (C.shape[0],)
    return cn2.astype(np.float64)


def _coef(dim, form):
    assert form in FORMS, form
    m = 16 * ((dim + 15) // 16) + 1
    return m * 2.0 ** -23 + (2.0 ** -18 if form == "r06" else 2.0 ** -24)


def _chunks(X, C, cn2, form):
    """(i0, i1, s, E) per chunk of rows: the scores and, with a form, the slack (else None)."""
    n, dim = X.shape
    k = C.shape[0]
    cn = _norms(C, cn2)
    Cb = round_bf16(C)
    step = max(1, _CHUNK_ELEMS // k)
    for i0 in range(0, n, step):
        Xb = round_bf16(X[i0:i0 + step])
        s = cn[None, :] / 2 - Xb @ Cb.T
        E = None
        if form is not None:
            mag = cn[None, :] / 2 + np.abs(Xb) @ np.abs(Cb).T
            S = mag.max(1)
            if form == "r06":
                S = S + 0.54 * (Xb ** 2).sum(1)  # the same for every centre
            E = _coef(dim, form) * S
            if cn2 is None:
                E = E + dim * 2.0 ** -24 * cn.max() / 2
        yield i0, i0 + Xb.shape[0], s, E


def scores(X, C, cn2=None):
    """s[i, c] = cn2[c] / 2 - sum_f bf16(X[i, f]) bf16(C[c, f]) in fp64 (cn2 None: the fp64 norms of
    the unrounded C)."""
    return np.concatenate([s for _, _, s, _ in _chunks(X, C, cn2, None)], axis=0)


def slack(X, C, cn2, form):
    """E[i] of the module docstring for the kernel form ('r06', 'r03' or 'tiles')."""
    return np.concatenate([E for _, _, _, E in _chunks(X, C, cn2, form)])


def check_labels(X, C, cn2, labels, form):
    """(violations, undecided_share, worst_ratio): the rows whose label's score exceeds the best
    by more than 2 E[i]; the share of rows whose model best and second best lie within 2 E[i]; the
    largest (s[i, label] - min_c s[i, c]) / E[i]."""
    labels = np.asarray(labels).astype(np.int64)
    n, k = X.shape[0], C.shape[0]
    assert labels.shape == (n,) and labels.min() >= 0 and labels.max() < k
    violations, undecided, worst = 0, 0, 0.0
    for i0, i1, s, E in _chunks(X, C, cn2, form):
        lab = labels[i0:i1]
        if k > 1:
            two = np.partition(s, 1, axis=1)[:, :2]
            best, gap = two[:, 0], two[:, 1] - two[:, 0]
            undecided += int((gap <= 2 * E).sum())
        else:
            best = s[:, 0]
        over = s[np.arange(i1 - i0), lab] - best
        violations += int((over > 2 * E).sum())
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(over > 0, over / E, 0.0)
        worst = max(worst, float(ratio.max()))
    return violations, undecided / n, worst
