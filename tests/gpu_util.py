"""Helpers shared by the GPU test modules."""
import bf16_model
from oracle import oracle as O


def force(monkeypatch, *tokens):
    """GDD_FORCE (gdd_common.hpp): force the listed paths for the next calls (none: the defaults)."""
    if tokens:
        monkeypatch.setenv("GDD_FORCE", ",".join(tokens))
    else:
        monkeypatch.delenv("GDD_FORCE", raising=False)


def bf16_check(X, C, labels, path, cn2=None):
    """bf16_model.check_labels for a gdd_kmeans_assign_bf16 call that took `path`
    (gdd_kmeans_assign_path): (violations, undecided_share, worst_ratio). cn2: the c_norm2 the call
    was given; None: NULL — the r06 kernel then sums the norms itself where they fit its LDS, every
    other case reads the numpy-order fp32 row norms (bit for bit the oracle's, test_assign_bitexact)."""
    form = bf16_model.form_of(path)
    if cn2 is None and not (form == "r06" and bf16_model.norms_fit(X.shape[1], C.shape[0])):
        cn2 = O.row_norms(C)
    return bf16_model.check_labels(X, C, cn2, labels, form)
