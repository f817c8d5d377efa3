"""Top-K lists from a saved distilled recommender, at the condensed model's own cost.

    python -m gdd.recommend_distilled --artifacts ClustGDD/distilled_recsys/Ali-Display --k 20 \\
        --exclude Rankformer/data/Ali-Display/train.txt --out lists.npy

``--artifacts`` is the directory :func:`gdd.recsys.save_distilled` writes; ``--users`` an ``.npy`` of
original user ids (default: every user, in order); ``--exclude`` a file of "user item" lines (the
Rankformer ``train.txt``) whose pairs score ``--mask_value`` instead of their model score; ``--out``
receives the int32 ``[B, k]`` item ids, best first. A thin command line over
:meth:`gdd.condrank.CondensedRecommender.load`.
"""
from __future__ import annotations

import argparse
import sys

import numpy as np


def parse_args(argv=None):
    p = argparse.ArgumentParser(description="ranked top-K lists from a distilled recommender's artefact")
    p.add_argument("--artifacts", type=str, required=True, help="directory written by gdd.recsys.save_distilled")
    p.add_argument("--k", type=int, default=20)
    p.add_argument("--users", type=str, default=None, help=".npy of user ids (default: every user)")
    p.add_argument("--exclude", type=str, default=None, help='"user item" lines to mask, e.g. train.txt')
    p.add_argument("--mask_value", type=float, default=-1024.0)
    p.add_argument("--lgn_layers", type=int, default=2, help="propagation layers of the distillation run")
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--out", type=str, required=True, help=".npy that receives the lists")
    return p.parse_args(argv)


def run(args) -> np.ndarray:
    import scipy.sparse as sp

    from .condrank import CondensedRecommender
    from .distill_recsys import _read_pairs
    rec = CondensedRecommender.load(args.artifacts, device=args.device, num_layers=args.lgn_layers)
    users = None if args.users is None else np.load(args.users)
    exclude = None
    if args.exclude is not None:
        u, i = _read_pairs(args.exclude)
        if u.size and (u.min() < 0 or u.max() >= rec.num_users or i.min() < 0 or i.max() >= rec.num_items):
            raise ValueError(f"{args.exclude}: a pair outside the model's {rec.num_users} users x "
                             f"{rec.num_items} items")
        exclude = sp.coo_matrix((np.ones(u.shape[0], np.float32), (u, i)),
                                shape=(rec.num_users, rec.num_items)).tocsr()
    lists = rec.recommend(args.k, users=users, exclude=exclude, mask_value=args.mask_value).cpu().numpy()
    np.save(args.out, lists)
    info = rec.last_info
    print(f"[recommend] {lists.shape[0]} users x top-{lists.shape[1]} from {info['ranked_clusters']} user clusters "
          f"x {info['list_len']} item clusters, {info['fallback_users']} recomputed; saved to: {args.out}")
    return lists


def main(argv=None):
    run(parse_args(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
