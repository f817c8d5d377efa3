"""The plain numpy definition of gdd.rankeval, for the tests: fp64 scores, a stable sort by
(-score, item), and the metric formulas (precision = hits / k, recall = hits / min(n, k),
ndcg = dcg / idcg with 1 / log2(rank + 2) weights), everything in fp64.

Also the fixture's generator (``fixture_inputs``: a pure function of its seed, shared by
tools/make_golden_rankeval.py and the tests) and its loader."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_rankeval.npz")
FIXTURE_TOPKS = (1, 5, 20, 50)


def grid(rng, n, d):
    """An n x d fp32 table with entries in {-2, .., 2} / 2: every product is a multiple of 1/4 and
    every partial sum of at most 256 of them is below 2^10, so dot products are exact in fp32 in any
    order (and ties abound)."""
    return (rng.randint(-2, 3, size=(n, d)) / 2.0).astype(np.float32)


def csr_of(rows, cols, n_rows):
    """Sorted distinct (row, col) pairs as (ptr int32 [n_rows + 1], col int32)."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    if rows.size:
        pairs = np.unique(np.stack([rows, cols], 1), axis=0)
    else:
        pairs = np.zeros((0, 2), np.int64)
    ptr = np.searchsorted(pairs[:, 0], np.arange(n_rows + 1))
    return ptr.astype(np.int32), pairs[:, 1].astype(np.int32)


def take_rows(ptr, col, users):
    """The CSR rows ``users`` in that order."""
    ptr, col = np.asarray(ptr, np.int64), np.asarray(col)
    out = np.zeros(len(users) + 1, np.int64)
    parts = []
    for b, u in enumerate(users):
        parts.append(col[ptr[u]:ptr[u + 1]])
        out[b + 1] = out[b] + parts[-1].shape[0]
    c = np.concatenate(parts) if parts else np.zeros(0, np.int32)
    return out.astype(np.int32), c.astype(np.int32)


def scores64(U, V, users=None, mask=None, mask_value=-1024.0):
    """fp64 scores [B, I]; ``mask`` = (ptr, col) with one row per selected user."""
    U, V = np.asarray(U, np.float64), np.asarray(V, np.float64)
    S = (U if users is None else U[np.asarray(users)]) @ V.T
    if mask is not None:
        ptr, col = mask
        for b in range(S.shape[0]):
            S[b, col[ptr[b]:ptr[b + 1]]] = np.float64(np.float32(mask_value))
    return S


def ranked(S, k):
    """(items int32 [B, k], scores fp64 [B, k]): descending score, equal scores by ascending item."""
    order = np.argsort(-S, axis=1, kind="stable")[:, :k]
    return order.astype(np.int32), np.take_along_axis(S, order, 1)


def metrics(lists, te_ptr, te_col, deg, topks):
    """(per_user [B, 3, nk], sums [3, nk], count) from ranked lists; ``deg`` None: the row length."""
    lists = np.asarray(lists)
    B, K = lists.shape
    nk = len(topks)
    inv = 1.0 / np.log2(np.arange(K, dtype=np.float64) + 2.0)
    per = np.zeros((B, 3, nk))
    count = 0
    for b in range(B):
        row = te_col[te_ptr[b]:te_ptr[b + 1]]
        n = int(deg[b]) if deg is not None else int(row.shape[0])
        if n <= 0:
            continue
        count += 1
        hit = np.isin(lists[b], row)
        for j, k in enumerate(topks):
            cut = min(n, k)
            hits = int(hit[:k].sum())
            dcg = 0.0
            for r in range(k):
                if hit[r]:
                    dcg += inv[r]
            idcg = 0.0
            for r in range(cut):
                idcg += inv[r]
            per[b, :, j] = (hits / k, hits / cut, dcg / idcg)
    return per, per.sum(0), count


def fixture_inputs(seed=20):
    """300 users x 500 items, d = 16, grid embeddings; train and valid lines with repeats; users
    0..9 have no valid line, users 10..14 more than 50 distinct valid items."""
    rng = np.random.RandomState(seed)
    n, m, d = 300, 500, 16
    U, V = grid(rng, n, d), grid(rng, m, d)
    tu = rng.randint(0, n, 4000)
    ti = rng.randint(0, m, 4000)
    rep = rng.randint(0, 4000, 300)
    train_u, train_i = np.concatenate([tu, tu[rep]]), np.concatenate([ti, ti[rep]])
    vu = rng.randint(10, n, 2500)
    vi = rng.randint(0, m, 2500)
    big_u = np.repeat(np.arange(10, 15), 70)
    big_i = np.concatenate([rng.permutation(m)[:70] for _ in range(5)])
    vu, vi = np.concatenate([vu, big_u]), np.concatenate([vi, big_i])
    rep = rng.randint(0, vu.shape[0], 200)
    valid_u, valid_i = np.concatenate([vu, vu[rep]]), np.concatenate([vi, vi[rep]])
    # a valid line that is also a training pair is masked and can never be hit: keep some
    return dict(n=n, m=m, U=U, V=V, train_u=train_u.astype(np.int64), train_i=train_i.astype(np.int64),
                valid_u=valid_u.astype(np.int64), valid_i=valid_i.astype(np.int64))


def fixture_reference_run(c, topks=FIXTURE_TOPKS, mask_value=-1024.0):
    """What RankingEvaluator computes on the fixture, by the plain definition: evaluated users (the
    sorted distinct valid users), their lists, per-user metrics, means and count."""
    n, m = int(c["n"]), int(c["m"])
    users = np.unique(c["valid_u"])
    tr = take_rows(*csr_of(c["train_u"], c["train_i"], n), users)
    te = take_rows(*csr_of(c["valid_u"], c["valid_i"], n), users)
    deg = np.bincount(c["valid_u"], minlength=n)[users]
    lists, _ = ranked(scores64(c["U"], c["V"], users, tr, mask_value), max(topks))
    per, sums, count = metrics(lists, te[0], te[1], deg, topks)
    return dict(users=users, lists=lists, te=te, deg=deg, per=per, means=sums / max(count, 1), count=count)


def load_fixture():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}
