"""Deterministic inputs for the refinement epoch's edge tests, shared by the host file
(test_refine_cases_host.py, which asserts from the fp64 reference alone that the inputs have the
properties the device cases rest on) and the device file (test_gpu_refine_forms.py).

numpy only: nothing here touches a device. Every builder is cached and its arrays are read, never
written, by the tests. A case is a dict: ``params`` (the five fp32 parameters), ``edge_index`` (CSR
order), ``u`` / ``pos_i`` / ``neg_i``, ``teacher`` (two tables or None), ``num_layers``, ``reg_lambda``,
``kd_lambda``."""
import functools

import numpy as np

# The device must stay within F times a case's yardstick (refine_ref.references): the smallest power
# of two that is at least twice the largest ratio measured over every case below.
F = 16.0

CHUNK = 64  # entries a wave of k_spmm / k_seed / k_degrees / k_degrad resolves per turn
GATHER = 16  # k_spmm: entries whose gathers are issued together

LADDER = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 200)  # row r of the ladder graph has LADDER[r] entries
LADDER_ITEMS = 200
LADDER_ROWS = 16  # four more rows of 3..9 entries

GROUPS = (0, 1, 63, 64, 65, 128, 129, 193)  # user r is drawn GROUPS[r] times
ITEM_GROUPS = (0, 1, 63, 64, 65, 128, 129, 193, 643)  # item c fills ITEM_GROUPS[c] of the 2 B entries

WIDTHS = (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256)
LAYERS = (0, 1, 2, 4, 8)
FOLD_B = 4117  # 258 blocks of 16 triplets, the last of 5: two turns of k_final's 256-thread fold
LOGITS = (-100.0, -30.0, -20.0, 0.0, 19.999, 20.0, 20.001, 30.0, 80.0)
DRIVER_SCALES = ((1e-4, 0.01, True), (1e-4, 0.01, False))  # (reg_lambda, kd_lambda, teacher) of the driver


def _f32(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def _params(rng, nu, ni, d, n_edges, delta=0.05, logits=None):
    if logits is None:
        logits = 1.5 * _f32(rng, n_edges) + 0.5
    return {"user_emb.weight": 0.1 * _f32(rng, nu, d), "item_emb.weight": 0.1 * _f32(rng, ni, d),
            "user_delta": np.float32(delta) * _f32(rng, nu, d), "item_delta": np.float32(delta) * _f32(rng, ni, d),
            "edge_logit": np.asarray(logits, np.float32)}


def _case(rng, dense, d, num_layers, trip, reg=1.0, kd=1.0, teacher=True, **kw):
    nu, ni = dense.shape
    cu, ci = np.nonzero(dense)  # row-major: CSR order
    params = _params(rng, nu, ni, d, cu.shape[0], **kw)
    t = (0.1 * _f32(rng, nu, d), 0.1 * _f32(rng, ni, d))
    u, pos_i, neg_i = (np.asarray(a, np.int64) for a in trip)
    return {"params": params, "edge_index": np.stack([cu, ci]).astype(np.int64), "u": u, "pos_i": pos_i,
            "neg_i": neg_i, "teacher": t if teacher else None, "num_layers": int(num_layers),
            "reg_lambda": float(reg), "kd_lambda": float(kd)}


def _uniform_triplets(rng, nu, ni, b):
    return rng.integers(0, nu, b), rng.integers(0, ni, b), rng.integers(0, ni, b)


def _random_dense(rng, nu, ni, density):
    """Every row and every column holds an edge, so no gradient of the case is identically zero."""
    dense = rng.random((nu, ni)) < density
    dense[np.arange(nu), rng.integers(0, ni, nu)] = True
    dense[rng.integers(0, nu, ni), np.arange(ni)] = True
    return dense


# ---- 1. row ladders ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ladder_dense():
    """16 x 200: row r has LADDER[r] entries (rows 5, 6, 7 / 8..11 with 63, 64, 65 / 127..200 entries sit
    in waves 1, 2, 3 / 0..3 of their four-node blocks), the last four rows 3..9."""
    rng = np.random.default_rng(101)
    dense = np.zeros((LADDER_ROWS, LADDER_ITEMS), bool)
    lengths = list(LADDER) + list(rng.integers(3, 10, LADDER_ROWS - len(LADDER)))
    for r, n in enumerate(lengths):
        dense[r, rng.choice(LADDER_ITEMS, n, replace=False)] = True
    return dense


@functools.lru_cache(maxsize=None)
def row_ladder(transposed, d):
    rng = np.random.default_rng(110 + d + (1000 if transposed else 0))
    dense = ladder_dense().T if transposed else ladder_dense()
    return _case(rng, dense, d, 2, _uniform_triplets(rng, *dense.shape, 300))


# ---- 2. group ladders ----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_ladder():
    """643 triplets over 8 users and 9 items: user r drawn GROUPS[r] times, item c in ITEM_GROUPS[c] of
    the 1286 (triplet, sign) entries, both shuffled, so that the large items are positive and negative in
    interleaved triplets, some triplets have ``pos == neg`` and some are repeated."""
    rng = np.random.default_rng(202)
    u = rng.permutation(np.repeat(np.arange(len(GROUPS)), GROUPS))
    b = u.shape[0]
    assert sum(ITEM_GROUPS) == 2 * b
    ent = rng.permutation(np.repeat(np.arange(len(ITEM_GROUPS)), ITEM_GROUPS))
    dense = _random_dense(rng, len(GROUPS), len(ITEM_GROUPS), 0.4)
    return _case(rng, dense, 5, 1, (u, ent[0::2], ent[1::2]))


# ---- 3. widths, 4. layers ------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def width(d):
    rng = np.random.default_rng(300 + d)
    return _case(rng, _random_dense(rng, 9, 7, 0.3), d, 2, _uniform_triplets(rng, 9, 7, 40))


@functools.lru_cache(maxsize=None)
def layers(num_layers, no_edges=False):
    rng = np.random.default_rng(400 + num_layers + (50 if no_edges else 0))
    dense = np.zeros((9, 7), bool) if no_edges else _random_dense(rng, 9, 7, 0.3)
    return _case(rng, dense, 6, num_layers, _uniform_triplets(rng, 9, 7, 40))


# ---- 5. terms ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def terms(scale=None):
    """The designated input of every ``drop=`` variant: deltas as large as the embeddings' sum and
    logits in 5..30, so that each regulariser is a visible share of the loss and of the gradients it
    enters. ``scale``: None for reg_lambda = kd_lambda = 1, or an entry of DRIVER_SCALES."""
    rng = np.random.default_rng(500)
    dense = _random_dense(rng, 9, 7, 0.3)
    n_edges = int(dense.sum())
    logits = rng.uniform(5.0, 30.0, n_edges)
    reg, kd, teacher = (1.0, 1.0, True) if scale is None else scale
    return _case(rng, dense, 8, 2, _uniform_triplets(rng, 9, 7, 40), reg=reg, kd=kd, teacher=teacher,
                 delta=1.0, logits=logits)


# ---- 6. loss fold --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def loss_fold():
    rng = np.random.default_rng(600)
    nu, ni = 300, 41
    return _case(rng, _random_dense(rng, nu, ni, 0.03), 4, 1, _uniform_triplets(rng, nu, ni, FOLD_B))


# ---- 7. logits -----------------------------------------------------------------------------------------
LOGIT_ROW, LOGIT_COL = 3, 5  # the user row and the item column whose logits are all -100


@functools.lru_cache(maxsize=None)
def logits():
    """12 x 10 at 60 %: the edges take LOGITS in turn along the CSR order (so every row mixes them);
    user row LOGIT_ROW and item column LOGIT_COL are all -100: rows of vanishing weights."""
    rng = np.random.default_rng(700)
    dense = _random_dense(rng, 12, 10, 0.6)
    cu, ci = np.nonzero(dense)
    lg = np.asarray(LOGITS, np.float32)[np.arange(cu.shape[0]) % len(LOGITS)]
    lg[(cu == LOGIT_ROW) | (ci == LOGIT_COL)] = -100.0
    return _case(rng, dense, 5, 2, _uniform_triplets(rng, 12, 10, 60), logits=lg)


@functools.lru_cache(maxsize=None)
def logits_above_10():
    """L = 0, every logit in (10, 10.25]: the edge gradient is the weight regulariser's 2e-6 w sigmoid(x)
    alone, and w = log1p(exp(x)) still lies exp(-x) = 4.5e-5 above x, 4.4e-6 of w: a softplus that
    returned x here would show."""
    rng = np.random.default_rng(710)
    dense = _random_dense(rng, 9, 7, 0.3)
    lg = 10.25 - 0.25 * rng.random(int(dense.sum()))
    return _case(rng, dense, 5, 0, _uniform_triplets(rng, 9, 7, 40), logits=lg)


# ---- 8 and 9. Adam, the loop ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adam(no_edges=False):
    rng = np.random.default_rng(800 + (1 if no_edges else 0))
    dense = np.zeros((9, 7), bool) if no_edges else _random_dense(rng, 9, 7, 0.3)
    return _case(rng, dense, 6, 0 if no_edges else 2, _uniform_triplets(rng, 9, 7, 40))


# ---- the table the tests walk --------------------------------------------------------------------------
FAMILIES = {
    "rows": {f"rows-{'t' if t else 'n'}-d{d}": functools.partial(row_ladder, t, d)
             for t in (False, True) for d in (5, 8)},
    "groups": {"groups": group_ladder},
    "widths": {f"width-{d}": functools.partial(width, d) for d in WIDTHS},
    "layers": {**{f"layers-{n}": functools.partial(layers, n) for n in LAYERS},
               "layers-2-no-edges": functools.partial(layers, 2, True)},
    "terms": {"terms": terms, "terms-driver-kd": functools.partial(terms, DRIVER_SCALES[0]),
              "terms-driver": functools.partial(terms, DRIVER_SCALES[1])},
    "fold": {"fold": loss_fold},
    "logits": {"logits": logits, "logits-above-10": logits_above_10},
}
CASES = {name: build for fam in FAMILIES.values() for name, build in fam.items()}
FAMILY_OF = {name: fam for fam, members in FAMILIES.items() for name in members}
TERMS_CASE = "terms"  # the designated case of every drop= variant


def case(name):
    return CASES[name]()
