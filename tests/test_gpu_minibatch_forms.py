"""MiniBatchKMeans.fit once per form of the step's assignment launch (k_mb_assign<W, vec>: 4, 2 or 1
waves per block by the LDS a dim needs, 16-byte or scalar loads) and once on the reassignment's chain
form, each against the CPU oracle bit for bit — needs a gfx950 GPU. The form is asserted by name first
(gdd_minibatch_step_path, gdd_minibatch_fit_path), so a shape that slips onto another form fails here
although every form returns the same bits."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

import gdd  # noqa: E402
from gdd import _lib, synth  # noqa: E402


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def fit_equals_oracle(n, dim, k, bs, seed=7, **kw):
    """Blobs with k // 3 centres leave clusters empty, so reassignments fire. n_steps_, labels, centre
    bits, inertia and the generator's final state."""
    X = synth.blobs(n, dim, max(2, k // 3), seed=n + dim + k)
    rs_ref = np.random.RandomState(seed)
    ref = O.minibatch_kmeans(X, k, random_state=rs_ref, batch_size=bs, **kw)
    s_ref = rs_ref.get_state()
    rs = np.random.RandomState(seed)
    m = gdd.MiniBatchKMeans(n_clusters=k, random_state=rs, batch_size=bs, **kw).fit(X)
    assert m.n_steps_ == ref["n_steps_"]
    assert np.array_equal(m.labels_, ref["labels_"])
    assert np.array_equal(bits(m.cluster_centers_), bits(ref["cluster_centers_"]))
    assert m.inertia_ == ref["inertia_"]
    s = rs.get_state()
    assert np.array_equal(s[1], s_ref[1]) and s[2] == s_ref[2]


# (dim, k, the step's form at b = 256: P = 8 point groups)
STEP_FORMS = [
    (40, 70, "w4/vec/g1xp8"),
    (41, 300, "w4/scalar/g3xp8"),
    (150, 70, "w4/scalar/g1xp8"),  # the last dim on four waves (150 % 4 != 0)
    (152, 70, "w2/vec/g2xp8"),
    (151, 40, "w2/scalar/g1xp8"),
    (424, 70, "w1/vec/g3xp8"),
    (423, 33, "w1/scalar/g2xp8"),
    (512, 20, "w1/vec/g1xp8"),  # the widest dim
]


@pytest.mark.parametrize("dim,k,form", STEP_FORMS)
def test_minibatch_step_forms(dim, k, form):
    n, bs = 1500, 256
    lib = _lib.device_lib()
    assert lib.gdd_minibatch_step_path(bs, dim, k, 0).decode() == form
    assert lib.gdd_minibatch_fit_path(n, dim, k, bs).decode() == "dev/par"
    fit_equals_oracle(n, dim, k, bs)


def test_minibatch_reassign_chain_form():
    """The smallest shape on the reassignment's chain form (one dependent copy chain per reassigned
    cluster): the whole-batch limit b = 13312 and k from 1933, where the parallel copies' index tables
    no longer fit the LDS beside the swap table. The seeding draws from 2,000 points (init_size), which
    keeps the oracle's k-means++ to half a second."""
    n, dim, k, bs = 13312, 2, 1933, 13312
    lib = _lib.device_lib()
    assert lib.gdd_minibatch_fit_path(n, dim, k - 1, bs).decode() == "dev/par"
    assert lib.gdd_minibatch_fit_path(n, dim, k, bs).decode() == "dev/chain"
    fit_equals_oracle(n, dim, k, bs, init_size=2000)
