"""Loading helpers for the golden fixtures (tests/golden/, produced by tools/make_golden.py)."""
import glob
import io
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# Propagation parity against the reference's torch-CPU SpMM: its summation order is not the
# canonical one (nor cuSPARSE's), so fp32 results agree to rounding, not bit for bit.
PROP_RTOL, PROP_ATOL = 1e-5, 1e-6
# Cluster means: the reference reduces with torch.mean (fp32 tree); ours is fp64 then rounded.
MEAN_RTOL, MEAN_ATOL = 1e-5, 1e-6


PART_BYTES = 900_000  # a committed file stays under 1 MiB


def load(name):
    """A fixture's arrays by name. One too large for a single committed file is stored as
    <stem>.partNN.npz (:func:`save_parts`): whole arrays, and row blocks "<key>@<i>" of an array that
    is itself too large ("<key>@T<i>": of its transpose, for a column-major one), joined here in order."""
    path = os.path.join(GOLDEN, name)
    if os.path.exists(path):
        return np.load(path, allow_pickle=False)
    parts = sorted(glob.glob(os.path.join(GOLDEN, os.path.splitext(name)[0] + ".part[0-9][0-9].npz")))
    if not parts:
        raise FileNotFoundError(path)
    out, blocks = {}, {}
    for p in parts:
        with np.load(p, allow_pickle=False) as z:
            for key in z.files:
                base, at, i = key.partition("@")
                if at:
                    blocks.setdefault((base, i[0] == "T"), {})[int(i.lstrip("T"))] = z[key]
                else:
                    out[key] = z[key]
    for (base, transposed), b in blocks.items():
        a = np.concatenate([b[i] for i in range(len(b))])
        out[base] = a.T if transposed else a
    return out


def _packed(a):
    buf = io.BytesIO()
    np.savez_compressed(buf, a=a)
    return buf.tell()


def save_parts(name, arrays, limit=PART_BYTES):
    """Writes `arrays` as <stem>.partNN.npz files of at most about `limit` bytes each, for
    :func:`load`: arrays in order, a part closed when the next would overflow it; an array over the
    limit on its own goes in as row blocks "<key>@<i>"."""
    items = []
    for key, a in arrays.items():
        a = np.asarray(a)
        pieces = 1 if a.ndim == 0 else -(-_packed(a) // limit)
        if pieces == 1:
            items.append((key, a))
        elif a.ndim == 2 and a.flags.f_contiguous and not a.flags.c_contiguous:
            # column-major: blocks of the transpose, so that load() returns the same layout
            items += [(f"{key}@T{i}", blk) for i, blk in enumerate(np.array_split(a.T, pieces + 1))]
        else:
            items += [(f"{key}@{i}", blk) for i, blk in enumerate(np.array_split(a, pieces + 1))]
    stem = os.path.join(GOLDEN, os.path.splitext(name)[0])
    for old in glob.glob(stem + ".part[0-9][0-9].npz"):
        os.remove(old)
    parts, size = [{}], 0
    for key, a in items:
        n = _packed(a)
        if parts[-1] and size + n > limit:
            parts.append({})
            size = 0
        parts[-1][key] = a
        size += n
    for i, part in enumerate(parts):
        np.savez_compressed(f"{stem}.part{i:02d}.npz", **part)


def load_json(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def graph_names():
    return ["binary", "selfloop0", "weighted", "isolated"]


def rng_from_fixture(z):
    """The numpy global-RNG state captured right before the reference's sklearn call."""
    rs = np.random.RandomState()
    rs.set_state(("MT19937", z["rng_key"], int(z["rng_pos"]), int(z["rng_has_gauss"]),
                  float(z["rng_cached_gauss"])))
    return rs


def csr_to_sorted_coo(rowptr, col, val):
    rows = np.repeat(np.arange(len(rowptr) - 1, dtype=np.int32), np.diff(rowptr))
    return rows, np.asarray(col, np.int32), np.asarray(val, np.float32)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
