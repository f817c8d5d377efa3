"""Record tests/golden/golden_rankeval.npz from the reference Rankformer code (CPU, data only).

    python tools/make_golden_rankeval.py --reference <checkout>/Rankformer/code

Imports the reference's ``model.py`` (its ``parse.py`` reads ``sys.argv`` at import, so argv is set
first: ``--device -1 --topks "[1, 5, 20, 50]"``) and calls its ``test(pred, test, recall_n)``
(model.py:27-53) the way ``evaluate`` does (:321-329): ``pred`` are the ranked lists of all 300
users as edge ids ``user * num_items + item``, ``test`` the validation lines as edge ids, ``recall_n``
the users' validation line counts, repeated lines included (dataloader.py:65-70). The lists come
from tests/rankeval_ref.py (fp64 scores, training items at -1024, stable sort) on
``rankeval_ref.fixture_inputs()``: the scores are exact on the fixture's grid embeddings, so they
are the lists ``torch.topk`` would give up to its order among equal scores.

Stored: the inputs (``n``, ``m``, ``U``, ``V``, ``train_u``, ``train_i``, ``valid_u``, ``valid_i``),
``topks``, the reference's ``ref_precision`` / ``ref_recall`` / ``ref_ndcg`` (its fp32 sums divided
by its count, as evaluate does, :338-340), ``ref_count``, and ``self_generated`` = 0.
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rankeval_ref as R  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference's Rankformer/code directory")
    ap.add_argument("--out", default=R.GOLDEN)
    a = ap.parse_args()
    topks = list(R.FIXTURE_TOPKS)
    sys.argv = [sys.argv[0], "--device", "-1", "--topks", str(topks)]
    sys.path.insert(0, os.path.abspath(a.reference))
    import torch
    import model as ref_model  # noqa: E402  (the reference's)

    assert list(ref_model.args.topks) == topks
    c = R.fixture_inputs()
    n, m = c["n"], c["m"]
    users = np.arange(n)
    tr = R.csr_of(c["train_u"], c["train_i"], n)
    lists, _ = R.ranked(R.scores64(c["U"], c["V"], users, tr, -1024.0), max(topks))
    pred = torch.from_numpy(users[:, None] * m + lists.astype(np.int64)).to(ref_model.args.device)
    truth = torch.from_numpy(c["valid_u"] * m + c["valid_i"]).to(ref_model.args.device)
    deg = torch.from_numpy(np.bincount(c["valid_u"], minlength=n)).long().to(ref_model.args.device)
    cnt, pre, rec, ndcg = ref_model.test(pred, truth, deg)
    pre, rec, ndcg = (x.to(torch.float32) / cnt for x in (pre, rec, ndcg))
    out = dict(c, topks=np.asarray(topks, np.int32), ref_count=np.int64(cnt),
               ref_precision=pre.numpy().astype(np.float64), ref_recall=rec.numpy().astype(np.float64),
               ref_ndcg=ndcg.numpy().astype(np.float64), self_generated=np.int32(0))
    out["n"], out["m"] = np.int64(n), np.int64(m)
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes; count {cnt}")
    for i, k in enumerate(topks):
        print(f"ndcg@{k} = {float(ndcg[i]):f}, recall@{k} = {float(rec[i]):f}, pre@{k} = {float(pre[i]):f}")


if __name__ == "__main__":
    main()
