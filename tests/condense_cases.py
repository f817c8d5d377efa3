"""Deterministic inputs for the condensation edge tests, shared by the host file
(test_condense_cases_host.py, which asserts from the oracle alone that the inputs have the
properties the device cases rest on) and the device file (test_gpu_condense_forms.py).

numpy only: nothing here touches a device. Every builder is cached and its arrays are read, never
written, by the tests."""
import functools

import numpy as np
import scipy.sparse as sp

from gdd import synth
from oracle import oracle as OO

BLK = 4096  # top-k compaction block of csrc/gdd_condense.hip (kTkBlk), also its row-sum chunk

# row -> length: both sides of the whole-workgroup threshold (512) and of the 4096-value chunk,
# two and three chunks, several long rows in the first 64-row workgroup and some in later ones
LONG_ROWS = {0: 511, 1: 512, 2: 513, 3: 4095, 10: 4096, 63: 4097, 64: 8192, 65: 8197, 200: 12291}
LONG_N = 12300

TOPK_NNZ = 3 * BLK + 17          # four blocks, the last one of 17 edges
TOPK_NNZ_BIG = 256 * BLK + BLK + 5  # 258 blocks: two per scan lane, the last lanes idle


def topk_ms(nnz):
    """The cut-offs of the one-set tie cases: the issue's seven and 3 * nnz // 4, which puts the
    threshold of "mixed" on a finite negative value."""
    return (1, BLK - 1, BLK, BLK + 1, nnz // 2, 3 * nnz // 4, nnz - 1, nnz)


def topk_ms_big(nnz):
    return (nnz // 10, nnz - 3)


@functools.lru_cache(maxsize=None)
def long_row_graph(seed=11):
    """(rowptr, col, val, n): not symmetric, rows of LONG_ROWS' lengths and 1..11 entries elsewhere,
    columns distinct and ascending, values (U[0,1) + 0.1) * 2^j with j in -6..6 so that the order of
    a row's sum shows in its bits. The binary variant is the same pattern with val = None."""
    rng = np.random.default_rng(seed)
    n = LONG_N
    length = rng.integers(1, 12, n)
    for r, L in LONG_ROWS.items():
        length[r] = L
    # short rows: ascending columns from positive gaps (11 * (n // 12) < n keeps them in range)
    short = np.cumsum(rng.integers(1, n // 12, (n, 11)), axis=1) - 1
    cols = []
    for r in range(n):
        if r in LONG_ROWS:
            cols.append(np.sort(rng.choice(n, LONG_ROWS[r], replace=False)))
        else:
            cols.append(short[r, : length[r]])
    col = np.concatenate(cols).astype(np.int32)
    rowptr = np.zeros(n + 1, np.int32)
    rowptr[1:] = np.cumsum(length)
    nnz = len(col)
    val = ((rng.random(nnz) + 0.1) * np.exp2(rng.integers(-6, 7, nnz))).astype(np.float32)
    return rowptr, col, val, n


@functools.lru_cache(maxsize=None)
def small_graph(seed=75):
    """(rowptr, col, val, n) of the normalised chung_lu(600, 8, seed) (the oracle's normalisation,
    which the device's equals bit for bit); the binary variant is the same pattern with val = None."""
    A = sp.csr_matrix(synth.chung_lu(600, 8.0, seed))
    rowptr, col, val = OO.normalize_csr(A.indptr, A.indices, None, -1)
    return rowptr, col, val, A.shape[0]


ZERO_ROWS = (5, 17, 333)


@functools.lru_cache(maxsize=None)
def embeddings(n, C, seed=0):
    """n x C normal logits (scale 2) with the rows ZERO_ROWS all zero: the norm clamp gives them zero
    cosines, their reweighted rows sum to 0 and their ER is NaN, which top-k ranks largest."""
    e = (np.random.default_rng(1000 * C + seed).standard_normal((n, C)) * 2).astype(np.float32)
    for r in ZERO_ROWS:
        if r < n:
            e[r] = 0.0
    return e


@functools.lru_cache(maxsize=None)
def tie_weights(nnz, kind, seed=21):
    rng = np.random.default_rng(seed + nnz % 1000)
    if kind == "ints":
        return rng.integers(0, 5, nnz).astype(np.float32)
    if kind == "equal":
        return np.full(nnz, 2.5, np.float32)
    if kind == "ints1000":
        return rng.integers(0, 1000, nnz).astype(np.float32)
    if kind == "mixed":
        w = rng.integers(-3, 4, nnz).astype(np.float32)
        den = np.float32(1e-40)  # a denormal: its key differs from zero's only in the low bits
        specials = [np.nan, np.inf, -np.inf, -0.0, 0.0, den, -den]
        for q, s in enumerate(specials):  # each about 50 times, in every block
            w[7 + 3 * q:: 251 + 2 * q] = s
        return w
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def complete_graph(n):
    """(rowptr, rows, col) of the complete graph with self-loops, n * n entries."""
    rowptr = (np.arange(n + 1, dtype=np.int64) * n).astype(np.int32)
    rows = np.repeat(np.arange(n, dtype=np.int32), n)
    col = np.tile(np.arange(n, dtype=np.int32), n)
    return rowptr, rows, col


@functools.lru_cache(maxsize=None)
def complete_weights(n, nsets, seed=31):
    """(probs [n, nsets], er [n * n]) from {0.25, 0.5, 1.0} and {0.5, 1, 2}: every per-class product
    is an exact power of two, so each class has a handful of distinct weights and thousands of ties."""
    rng = np.random.default_rng(seed + n + nsets)
    probs = rng.choice(np.array([0.25, 0.5, 1.0], np.float32), (n, nsets))
    er = rng.choice(np.array([0.5, 1.0, 2.0], np.float32), n * n)
    return np.ascontiguousarray(probs), er


def tie_split(w, m):
    """How the oracle's rule splits the ties at the cut: (threshold value, ids of the ties taken,
    ids of the ties left). NaNs tie with each other, -0 with +0."""
    from oracle import condense as O
    sel = O.topk_edges(w, m)
    taken = np.zeros(len(w), bool)
    taken[sel] = True
    key = np.where(np.isnan(w), np.inf, w).astype(np.float64)
    rank = np.where(np.isnan(w), 2.0, 0.0)  # NaN above +inf
    order = np.lexsort((np.arange(len(w)), -key, -rank))
    last = order[m - 1]
    thr = w[last]
    tie = np.isnan(w) if np.isnan(thr) else (w == thr)
    return thr, np.flatnonzero(tie & taken), np.flatnonzero(tie & ~taken)
