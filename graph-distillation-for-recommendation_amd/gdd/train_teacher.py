"""Train the Rankformer teacher on the MI355X and write the file that
``gdd.distill_recsys --teacher_path`` loads (Rankformer/code/main.py with parse.py's flags).

    python -m gdd.train_teacher --data_dir Rankformer/data --dataset Ali-Display --out teacher.pt
    python -m gdd.distill_recsys --data_dir Rankformer/data --dataset Ali-Display --teacher_path teacher.pt

Flags keep the reference's names and defaults where the reference has them (``--hidden_dim``,
``--use_gcn``, ``--gcn_layers``, ``--gcn_left``, ``--gcn_right``, ``--gcn_mean``,
``--rankformer_layers``, ``--rankformer_tau``, ``--rankformer_alpha``, ``--rankformer_clamp_value``,
``--use_cl``, ``--cl_layer``, ``--cl_lambda``, ``--cl_eps``, ``--cl_tau``, ``--del_neg``,
``--del_benchmark``, ``--del_omega_norm``, ``--learning_rate``, ``--reg_lambda``, ``--loss_batch_size``, ``--max_epochs``, ``--valid_interval``,
``--stopping_step``, ``--seed``). The Rankformer layers are on unless ``--no_rankformer`` is given
(``--use_rankformer`` is accepted and changes nothing); ``--data_dir`` / ``--dataset`` are
``gdd.distill_recsys``'s. Repeated lines of ``train.txt`` are dropped with a note (the layer is
defined over distinct pairs). ``--select_by ndcg --topks "[20]"`` is the reference's model selection
(main.py:100-120): precision, recall and NDCG at every cut-off of ``--topks`` per validation, the epoch
with the best validation NDCG@max(topks) is kept, and the test split is reported at each new best.
The default, ``--select_by recall``, selects on Recall@``--eval_topk``. See :mod:`gdd.rankformer` for
what is not offered.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import torch

from .distill_recsys import load_rankformer_dataset
from .rankeval import format_metrics, parse_topks
from .rankformer import save_teacher, train_teacher


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--data_dir", type=str, default=os.path.join("Rankformer", "data"))
    p.add_argument("--dataset", type=str, default="Ali-Display")
    p.add_argument("--out", type=str, default="teacher_rankformer.pt")
    p.add_argument("--seed", type=int, default=12345)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--hidden_dim", type=int, default=64)
    p.add_argument("--use_gcn", action="store_true")
    p.add_argument("--gcn_layers", type=int, default=1)
    p.add_argument("--gcn_left", type=float, default=1.0)
    p.add_argument("--gcn_right", type=float, default=0.0)
    p.add_argument("--gcn_mean", action="store_true")
    p.add_argument("--use_rankformer", action="store_true", help="accepted; the layers are on by default")
    p.add_argument("--no_rankformer", action="store_true")
    p.add_argument("--rankformer_layers", type=int, default=1)
    p.add_argument("--rankformer_tau", type=float, default=0.5)
    p.add_argument("--rankformer_alpha", type=float, default=2.0)
    p.add_argument("--rankformer_clamp_value", type=float, default=0.0)
    p.add_argument("--use_cl", action="store_true", help="add the contrastive (InfoNCE) loss")
    p.add_argument("--cl_layer", type=int, default=1, help="the GCN layer (1-based) whose output is the view")
    p.add_argument("--cl_lambda", type=float, default=0.05)
    p.add_argument("--cl_eps", type=float, default=0.1, help="norm of the noise added after each GCN layer")
    p.add_argument("--cl_tau", type=float, default=0.15)
    p.add_argument("--del_neg", action="store_true", help="ablation: no negative pairs in the layer")
    p.add_argument("--del_benchmark", action="store_true", help="ablation: no benchmark terms in the layer")
    p.add_argument("--del_omega_norm", action="store_true", help="ablation: the layer's numerator, undivided")
    p.add_argument("--learning_rate", type=float, default=1e-1)
    p.add_argument("--reg_lambda", type=float, default=1e-4)
    p.add_argument("--loss_batch_size", type=int, default=0, help="0: full batch")
    p.add_argument("--max_epochs", type=int, default=2000)
    p.add_argument("--valid_interval", type=int, default=20)
    p.add_argument("--stopping_step", type=int, default=10)
    p.add_argument("--eval_topk", type=int, default=20)
    p.add_argument("--select_by", type=str, default="recall", choices=("recall", "ndcg"),
                   help="recall: Recall@eval_topk; ndcg: the reference's NDCG@max(topks) with the test split "
                        "reported at each new best")
    p.add_argument("--topks", type=str, default="[20]", help="cut-offs of --select_by ndcg, e.g. \"[20, 50]\"")
    args = p.parse_args(argv)
    try:
        args.topks = list(parse_topks(args.topks))
    except (ValueError, SyntaxError) as e:
        p.error(f"--topks: {e}")
    return args


def run(args):
    """Train, restore the best validation epoch, write ``args.out``. Returns (model, history)."""
    if not torch.cuda.is_available():
        raise RuntimeError("gdd.train_teacher: no HIP device visible (the MI355X path has no CPU fallback)")
    device = torch.device(args.device if args.device.startswith("cuda") else "cuda")
    print(f"[env] device={device}")
    ds = load_rankformer_dataset(args.data_dir, args.dataset)
    t0 = time.perf_counter()
    model, hist = train_teacher(
        ds.num_users, ds.num_items, ds.train_u, ds.train_i, ds.valid_u, ds.valid_i,
        hidden_dim=args.hidden_dim, learning_rate=args.learning_rate, reg_lambda=args.reg_lambda,
        loss_batch_size=args.loss_batch_size, max_epochs=args.max_epochs, valid_interval=args.valid_interval,
        stopping_step=args.stopping_step, topk=args.eval_topk, seed=args.seed, device=device, log=print,
        drop_repeats=True, select_by=args.select_by, topks=args.topks if args.select_by == "ndcg" else None,
        test_u=ds.test_u if args.select_by == "ndcg" else None,
        test_i=ds.test_i if args.select_by == "ndcg" else None,
        use_gcn=args.use_gcn, gcn_layers=args.gcn_layers, gcn_left=args.gcn_left, gcn_right=args.gcn_right,
        gcn_mean=args.gcn_mean, use_rankformer=not args.no_rankformer, rankformer_layers=args.rankformer_layers,
        rankformer_tau=args.rankformer_tau, rankformer_alpha=args.rankformer_alpha,
        rankformer_clamp_value=args.rankformer_clamp_value, use_cl=args.use_cl, cl_layer=args.cl_layer,
        cl_lambda=args.cl_lambda, cl_eps=args.cl_eps, cl_tau=args.cl_tau, del_neg=args.del_neg,
        del_benchmark=args.del_benchmark, del_omega_norm=args.del_omega_norm)
    torch.cuda.synchronize()
    if args.select_by == "ndcg":
        print(f"[teacher] {len(hist['loss'])} epochs in {time.perf_counter() - t0:.1f} s; best epoch "
              f"{hist['best_epoch']} ndcg@{args.topks[-1]}={hist['best_ndcg']:.6f}")
        if hist["test"] is not None:
            print(f"[teacher] ===== test result (at {hist['best_epoch']} epoch) =====")
            for line in format_metrics(args.topks, hist["test"]):
                print(f"[teacher] {line}")
    else:
        print(f"[teacher] {len(hist['loss'])} epochs in {time.perf_counter() - t0:.1f} s; best epoch "
              f"{hist['best_epoch']} Recall@{args.eval_topk}={hist['best_recall']:.6f}")
    out_dir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(out_dir, exist_ok=True)
    save_teacher(args.out, model)
    print(f"[save] teacher embeddings saved to: {args.out}")
    return model, hist


def main(argv=None):
    run(parse_args(argv))


if __name__ == "__main__":
    main(sys.argv[1:])
