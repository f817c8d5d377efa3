"""Graphs built for the edges of the graph kernels (gdd_normalize.hip, gdd_propagate.hip) and
references of normalisation and SpMM that share no code with the kernels or with oracle/.

The graphs put row lengths, diagonal positions and empty-row runs exactly at the sizes where the
kernels change path (16-lane chunks, the 8-entry unroll, 32/64-lane groups, GDD_PROP_SEG = 256
segments, 256-entry fill blocks, 512 staged row starts), instead of leaving them to the chance of a
random graph. Every builder is deterministic and returns a canonical scipy CSR (fp32 values, sorted
columns, no duplicates); the module-level caches hand out shared objects, which callers must not
modify.
"""
import functools

import numpy as np
import scipy.sparse as sp

SEG = 256  # GDD_PROP_SEG

# row lengths around every boundary of k_hop (8-entry unroll, 16/32/64-lane groups), the segment
# cut (256: one item; 257+: split rows with 2, 3 and 4 segments) and a full row
LADDER_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257,
                  258, 511, 512, 513, 767, 768)

# the expected forms, read from the dispatch: (d, align) -> form. A threshold moved on purpose has
# to edit this table.
HOP_FORMS = [
    # align 16, d % 4 == 0: float4 lanes
    (64, 16, "v4/g16/s1"), (100, 16, "v4/g32/s1"), (112, 16, "v4/g32/s1"), (116, 16, "v4/g16/s2"),
    (128, 16, "v4/g16/s2"), (132, 16, "v4/g64/s1"), (256, 16, "v4/g64/s1"), (260, 16, "v4/g64/s2"),
    (512, 16, "v4/g64/s2"), (516, 16, "v4/g64/s0"), (1024, 16, "v4/g64/s4"), (1028, 16, "v4/g64/s0"),
    (2048, 16, "v4/g64/s8"),
    # align 16, d % 4 == 2: float2 lanes
    (30, 16, "v2/g16/s1"), (34, 16, "v2/g32/s1"), (62, 16, "v2/g32/s1"), (66, 16, "v2/g64/s1"),
    (130, 16, "v2/g64/s2"), (258, 16, "v2/g64/s0"), (450, 16, "v2/g64/s4"), (602, 16, "v2/g64/s0"),
    (1022, 16, "v2/g64/s8"),
    # odd d: scalar lanes
    (7, 16, "v1/g16/s1"), (17, 16, "v1/g32/s1"), (31, 16, "v1/g32/s1"), (33, 16, "v1/g64/s1"),
    (65, 16, "v1/g64/s2"), (127, 16, "v1/g64/s2"), (129, 16, "v1/g64/s0"), (255, 16, "v1/g64/s4"),
    (257, 16, "v1/g64/s0"), (511, 16, "v1/g64/s8"),
    # the fall-backs for buffers that are only 8- or 4-byte aligned
    (128, 8, "v2/g64/s1"), (128, 4, "v1/g64/s2"),
]


def ladder_rows(n=768):
    """Row ids that carry LADDER_LENGTHS, in that order (spread over the rows, all four row-id
    residues mod 4)."""
    step = (n - 8) // len(LADDER_LENGTHS)
    return [5 + step * k for k in range(len(LADDER_LENGTHS))]


def _csr(n, lengths, cols, vals):
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(lengths, out=rowptr[1:])
    A = sp.csr_matrix((np.asarray(vals, np.float32), np.asarray(cols, np.int32),
                       rowptr.astype(np.int32)), shape=(n, n))
    assert A.has_canonical_format
    return A


@functools.lru_cache(maxsize=None)
def ladder_graph(n=768, seed=0, weighted=False, signed=False):
    """LADDER_LENGTHS at ladder_rows(n), every other row 0..11 entries; columns a sorted random
    subset; values 1, or uniform in [0.1, 3] (weighted), with a random sign each (signed: for SpMM
    only, never for normalisation)."""
    assert n >= max(LADDER_LENGTHS)
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 12, n)
    for r, L in zip(ladder_rows(n), LADDER_LENGTHS):
        lengths[r] = L
    cols = np.concatenate([np.sort(rng.choice(n, size=L, replace=False)) for L in lengths] or [[]])
    nnz = int(lengths.sum())
    vals = rng.uniform(0.1, 3.0, nnz).astype(np.float32) if weighted else np.ones(nnz, np.float32)
    if signed:
        vals = vals * rng.choice(np.float32([-1.0, 1.0]), nnz)
    return _csr(n, lengths, cols, vals)


# (stored columns below the row id, stored columns above it, diagonal stored as this entry or None)
DIAG_CASES = (
    # diagonal absent, inserted before the first larger column: lane 0, lanes 15/16 of the first
    # 16-lane chunk, lane 0 of the second chunk and lane 1 of it, lane 0 of the third
    (0, 5, None), (15, 5, None), (16, 5, None), (17, 5, None), (32, 5, None),
    # diagonal absent and every column below the row id: appended after 1, 2 and 3 chunks
    (1, 0, None), (16, 0, None), (17, 0, None), (40, 0, None),
    # diagonal stored as the 1st, 16th, 17th and 33rd entry of its row
    (0, 5, 1), (15, 5, 16), (16, 5, 17), (32, 5, 33),
)
DIAG_FIRST_ROW = 64


def diag_case_rows():
    """[(row id, case)] of diag_cases_graph: every case once per residue of the row id mod 4 (the
    four 16-lane groups of a wave in k_rows_emit)."""
    return [(DIAG_FIRST_ROW + 4 * c + g, case) for c, case in enumerate(DIAG_CASES) for g in range(4)]


@functools.lru_cache(maxsize=None)
def diag_cases_graph(seed=1):
    """Weighted graph (n = 192) whose rows DIAG_FIRST_ROW.. hold DIAG_CASES; the other rows have
    0..3 entries (some stay empty: without I their r is 0 and entries pointing at them are dropped)."""
    n = 192
    rng = np.random.default_rng(seed)
    cases = dict(diag_case_rows())
    lengths, cols = [], []
    for i in range(n):
        if i in cases:
            below, above, stored = cases[i]
            c = list(np.sort(rng.choice(i, size=below, replace=False)))
            if stored is not None:
                assert stored == below + 1
                c.append(i)
            c += list(np.sort(rng.choice(np.arange(i + 1, n), size=above, replace=False)))
        else:
            c = list(np.sort(rng.choice(n, size=rng.integers(0, 4), replace=False)))
        lengths.append(len(c))
        cols += c
    vals = rng.uniform(0.1, 3.0, len(cols)).astype(np.float32)
    return _csr(n, lengths, cols, vals)


SPARSE_HUB_ROW = 5
SPARSE_HUB_LEN = 1000
SPARSE_RUN = 1100   # empty rows in the middle: more than the 512 row starts a fill block stages
SPARSE_TAIL = 600   # empty rows at the end: the last fill block's range exceeds 512 rows too


@functools.lru_cache(maxsize=None)
def sparse_runs_graph(exact_multiple, seed=2):
    """Binary graph: row 0 empty; rows 1..4 of 4 entries; the hub (row 5, 1000 entries, diagonal
    stored; it starts at entry 16, so the fill blocks of entries 256..767 lie wholly inside it);
    short rows (the first with its diagonal stored) up to 1280 = 5 * 256 entries, or 1280 + 37;
    SPARSE_RUN empty rows; 100 rows of 5 entries; SPARSE_TAIL empty rows."""
    rng = np.random.default_rng(seed)
    head = [0, 4, 4, 4, 4, SPARSE_HUB_LEN] + [4] * 66  # 16 + 1000 + 264 = 1280
    if not exact_multiple:
        head.append(37)
    lengths = head + [0] * SPARSE_RUN + [5] * 100 + [0] * SPARSE_TAIL
    n = len(lengths)
    cols = []
    for i, L in enumerate(lengths):
        if i in (SPARSE_HUB_ROW, SPARSE_HUB_ROW + 1):  # stored diagonals: the hub and a short row
            others = rng.choice(np.delete(np.arange(n), i), size=L - 1, replace=False)
            c = np.sort(np.append(others, i))
        else:
            c = np.sort(rng.choice(n, size=L, replace=False))
        cols += list(c)
    A = _csr(n, lengths, cols, np.ones(len(cols), np.float32))
    before_run = int(A.indptr[len(head)])
    assert (before_run % SEG == 0) == bool(exact_multiple)
    return A


def fill_block_ranges(rowptr, blk=256):
    """For every blk-entry block of the CSR entry stream: (row of its first entry, row of its last
    entry, rows in its search range). The search range is what k_fast_fill is given: from the row of
    the block's first entry up to and including the row of the next block's first entry (the last
    block: up to the last row), so a run of empty rows after a block's last entry counts."""
    rowptr = np.asarray(rowptr, np.int64)
    n, nnz = len(rowptr) - 1, int(rowptr[-1])
    start = np.arange(0, nnz, blk)
    row_of = lambda p: np.searchsorted(rowptr, p, side="right") - 1
    first, last = row_of(start), row_of(np.minimum(start + blk, nnz) - 1)
    hi = np.append(first[1:] + 1, n)
    return first, last, hi - first


# ---- normalisation --------------------------------------------------------------------------------
def normalize_ref(A, add_identity):
    """Â = D^-1/2 (A [+ I]) D^-1/2 from the formula in gdd_normalize.hip's header -> (rowptr, col,
    val fp32), canonical CSR.

    With I: scipy in float64 (sp.eye promotes), rounded to fp32 once. Without I: fp32 throughout,
    elementwise numpy. Two limits, found by checking this against the oracle:
    * scipy's own fp32 route (np.power(rowsum, -0.5) on an fp32 array) differs from the project's
      r = fp32(fp64 rsqrt) by a few ulp on about a quarter of the entries, so the fp32 path is
      written out here instead of calling scipy;
    * with a negative row sum r is NaN, and scipy's products drop NaN * 0 entries that the project
      keeps. Adjacencies are non-negative: this reference is for positive weights only.
    """
    A = sp.csr_matrix(A)
    assert A.has_canonical_format and A.dtype == np.float32 and (A.data > 0).all()
    n = A.shape[0]
    if add_identity:
        M = A.astype(np.float64) + sp.eye(n, dtype=np.float64, format="csr")
        rowsum = np.asarray(M.sum(1)).ravel()
        with np.errstate(divide="ignore"):
            r = np.power(rowsum, -0.5)
        r[np.isinf(r)] = 0.0
        out = (sp.diags(r) @ M @ sp.diags(r)).tocsr()
        out.sort_indices()
        out = out.astype(np.float32)
        return out.indptr.astype(np.int32), out.indices.astype(np.int32), out.data
    rp, col, a = A.indptr, A.indices, A.data
    r = np.zeros(n, np.float32)
    for i in range(n):
        s = np.float32(0.0)
        for v in a[rp[i]:rp[i + 1]]:  # sequential fp32 sum in column order
            s = np.float32(s + v)
        with np.errstate(divide="ignore"):
            ri = np.float32(1.0 / np.sqrt(np.float64(s)))
        r[i] = np.float32(0.0) if np.isinf(ri) else ri
    rows = np.repeat(np.arange(n), np.diff(rp))
    t = r[rows] * a      # fp32
    u = t * r[col]       # fp32
    keep = (t != 0) & (u != 0)
    rowptr = np.zeros(n + 1, np.int32)
    np.cumsum(np.bincount(rows[keep], minlength=n), out=rowptr[1:])
    return rowptr, col[keep].astype(np.int32), u[keep].astype(np.float32)


def adds_identity(A, self_loops):
    """The reference's rule: I is added iff A[0,0] == 0, unless self_loops (0 / 1) forces it."""
    return bool(self_loops) if self_loops >= 0 else A[0, 0] == 0


# ---- SpMM -----------------------------------------------------------------------------------------
U32 = 2.0 ** -24  # fp32 unit roundoff


def spmm_ref64(A, x, scale):
    """y = (scale * A) @ x in fp64 with the stored values scaled in fp32 first (fp32(scale) * v, one
    rounding, as the kernel and the reference's `alpha * adj_norm` do) -> (y fp64, bound fp64).

    bound[i, f] = gamma_k * sum_j |a_ij| |x_jf|, gamma_k = k u / (1 - k u), u = 2^-24: the standard
    bound of a length-k fp32 sum of products in any order. For a row of L entries k = L +
    ceil(L / 256) + 1: L fused multiply-adds, the additions of the 256-entry segment partials, and
    one of slack for the first. A correct fp32 SpMM of any summation order lies within it."""
    A = sp.csr_matrix(A)
    As = A.copy()
    As.data = (np.float32(scale) * A.data.astype(np.float32)).astype(np.float32)
    A64 = As.astype(np.float64)
    x64 = np.asarray(x, np.float64)
    y = A64 @ x64
    L = np.diff(A.indptr).astype(np.float64)
    k = L + np.ceil(L / SEG) + 1
    gamma = k * U32 / (1 - k * U32)
    return y, gamma[:, None] * (abs(A64) @ np.abs(x64))


def csr_arrays(A):
    A = sp.csr_matrix(A)
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
