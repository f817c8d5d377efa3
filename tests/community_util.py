"""Host model of the community node order (gdd_community_order, DESIGN §4 "Community order") and the
graphs its tests share. numpy only: the model pins the device path bit for bit.

The definition: CAP = 256, deg[v] = rowptr[v+1] - rowptr[v], labels start as lab[v] = v. A sweep is
synchronous. Row r collects one vote for lab[r] itself and one for lab[c] of each of its first
min(deg[r], CAP) stored entries c with c != r and deg[c] <= CAP; its new label is the one with the
most votes, among equals the smallest. After the sweeps, order = the nodes sorted by (label, id) and
rho[order[j]] = j."""
import functools

import numpy as np

CAP = 256


def lpa_sweep(rowptr, col, lab, cap=CAP):            # int64 arrays
    n = lab.shape[0]; deg = np.diff(rowptr); lens = np.minimum(deg, cap)
    rows = np.repeat(np.arange(n), lens)
    off = np.arange(lens.sum()) - np.repeat(np.cumsum(lens) - lens, lens)
    nb = col[np.repeat(rowptr[:-1], lens) + off]
    keep = (nb != rows) & (deg[nb] <= cap)
    rows = np.r_[rows[keep], np.arange(n)]; nb = np.r_[nb[keep], np.arange(n)]
    uk, cnt = np.unique(rows * n + lab[nb], return_counts=True)
    r, l = uk // n, uk % n
    o = np.lexsort((l, -cnt, r)); first = np.r_[True, r[o][1:] != r[o][:-1]]
    new = lab.copy(); new[r[o][first]] = l[o][first]; return new


def community_order(rowptr, col, sweeps, cap=CAP):
    """(rho, labels, changed): `sweeps` sweeps of lpa_sweep from lab = arange(n); changed[s] = labels
    sweep s changed; rho from order = the nodes sorted by (label, id)."""
    rowptr = np.asarray(rowptr, np.int64)
    col = np.asarray(col, np.int64)
    n = rowptr.shape[0] - 1
    lab = np.arange(n, dtype=np.int64)
    changed = np.zeros(sweeps, np.int64)
    for s in range(sweeps):
        new = lpa_sweep(rowptr, col, lab, cap) if n else lab
        changed[s] = int((new != lab).sum())
        lab = new
    order = np.lexsort((np.arange(n), lab))
    rho = np.empty(n, np.int64)
    rho[order] = np.arange(n)
    return rho, lab, changed


def csr_from_pairs(n, u, v, diag=False):
    """Canonical CSR structure (rowptr, col: int64) of the symmetrised, deduplicated pairs without
    self pairs; diag=True stores every diagonal entry as well."""
    keep = u != v
    u, v = u[keep], v[keep]
    a = np.r_[u, v]
    b = np.r_[v, u]
    if diag:
        a = np.r_[a, np.arange(n)]
        b = np.r_[b, np.arange(n)]
    key = np.unique(a.astype(np.int64) * n + b)
    rows, col = key // n, key % n
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=rowptr[1:])
    return rowptr, col


def sbm_pairs(seed, n=8192, block=256, avg_deg=20, p_in=0.9, shuffle=True):
    """The stochastic block model of the tests: m = n * avg_deg / 2 draws, 90 % inside the block of
    u; ids shuffled by a permutation (shuffle=False: the true block order, blocks contiguous)."""
    rng = np.random.default_rng(seed)
    m = n * avg_deg // 2
    u = rng.integers(0, n, m)
    inside = rng.random(m) < p_in
    v = np.where(inside, (u // block) * block + rng.integers(0, block, m), rng.integers(0, n, m))
    perm = rng.permutation(n)
    if shuffle:
        u, v = perm[u], perm[v]
    return u, v


@functools.lru_cache(maxsize=None)
def sbm(seed, n=8192, diag=False, shuffle=True, hubs=0):
    """(rowptr, col) of the SBM; hubs > 0 adds that many hub rows (ids 0 .. hubs-1) of 1,500 draws
    each, far above CAP. Cached and shared: callers must not write into the arrays."""
    u, v = sbm_pairs(seed, n=n, shuffle=shuffle)
    if hubs:
        rng = np.random.default_rng(1000 + seed)
        hu = np.repeat(np.arange(hubs), 1500)
        u, v = np.r_[u, hu], np.r_[v, rng.integers(0, n, hu.shape[0])]
    rowptr, col = csr_from_pairs(n, u, v, diag)
    rowptr.setflags(write=False)
    col.setflags(write=False)
    return rowptr, col


@functools.lru_cache(maxsize=None)
def model(kind, seed, sweeps, **kw):
    """community_order of a cached graph, computed once and shared."""
    rowptr, col = {"sbm": sbm}[kind](seed, **kw)
    out = community_order(rowptr, col, sweeps)
    for a in out:
        a.setflags(write=False)
    return out


def near_fraction(rowptr, col, rho, window=1024):
    """Fraction of the stored entries (r, c) with |rho[r] - rho[c]| < window."""
    rows = np.repeat(np.arange(rowptr.shape[0] - 1), np.diff(rowptr))
    return float((np.abs(rho[rows] - rho[col]) < window).mean())


def rows_graph(lens, n, block=50):
    """A hand-built structure: a small block model (blocks of `block` nodes, ids in block order) whose
    first len(lens) rows are replaced by rows of exactly lens[i] distinct sorted columns drawn from all
    nodes, so that after a sweep or two the long rows count block labels with multiplicities and ties.
    Not symmetric: the definition does not need it."""
    rng = np.random.default_rng(7)
    m = n * 4
    u = rng.integers(0, n, m)
    v = np.minimum((u // block) * block + rng.integers(0, block, m), n - 1)
    rowptr, col = csr_from_pairs(n, u, v)
    cols = [np.sort(rng.choice(n, k, replace=False)) for k in lens]
    cols += [col[rowptr[i]:rowptr[i + 1]] for i in range(len(lens), n)]
    rowptr = np.zeros(n + 1, np.int64)
    np.cumsum([c.shape[0] for c in cols], out=rowptr[1:])
    return rowptr, np.concatenate(cols).astype(np.int64)


def ring(n):
    i = np.arange(n)
    return csr_from_pairs(n, i, (i + 1) % n)


def grid(h, w):
    i = np.arange(h * w).reshape(h, w)
    u = np.r_[i[:, :-1].ravel(), i[:-1, :].ravel()]
    v = np.r_[i[:, 1:].ravel(), i[1:, :].ravel()]
    return csr_from_pairs(h * w, u, v)


def path(n):
    i = np.arange(n - 1)
    return csr_from_pairs(n, i, i + 1)
