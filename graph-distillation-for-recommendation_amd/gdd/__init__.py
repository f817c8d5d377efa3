"""gdd — MI355X-native hot path of ClustGDD graph distillation.

Drop-in replacements for the reference's hot-path call sites (see include/gdd.h for the C ABI and
the reference file:line each entry point replaces):

* :func:`gdd.graph.to_csr`, :func:`gdd.graph.normalize_adj_tensor`, :func:`gdd.graph.propagate`
* :class:`gdd.kmeans.KMeans`, :class:`gdd.kmeans.MiniBatchKMeans`
* :func:`gdd.cluster.cluster_mean`, :func:`gdd.cluster.argmax_rows`
* :mod:`gdd.pipeline` — ``pretrained_clustering_hot_path`` (the ClustGDD stage end to end),
  ``kmeans_cluster`` / ``teacher_means`` / ``standard_scaler`` (distill_recsys)
* :mod:`gdd.condense` — ``graph_sparse`` / ``graph_compress`` / ``ER_estimator`` /
  ``attaw_ER_estimator`` (ClustGDD's sparsification and cluster-level graph)
* :class:`gdd.sharded.ShardedKMeans` — Lloyd on several ranks: the E-step partitioned by rows, the
  M-step by clusters, all-gathers of the labels and the cluster slices (bit-identical to one GPU);
  ``mstep="reduce"`` (opt-in) sums each rank's rows as int64 fixed point and all-reduces the
  k x (dim + 1) + 1 words once per iteration instead (bit-identical across world sizes and row
  splits; its own arithmetic, not scikit-learn's ordered sums)
* :func:`gdd.svd.truncated_svd`, :func:`gdd.svd.svd_embeddings` — the recommender's clustering
  embeddings as a deterministic fp64 block subspace iteration on the device (opt-in:
  ``distill_recsys --svd_backend device``)
* :mod:`gdd.rankformer` — the Rankformer teacher: :class:`RankformerLayer` / :class:`GCNLayer` as
  fused row passes without float atomics, :class:`RankformerTeacher`, ``rankformer.train_teacher``
  and :func:`save_teacher` (the file ``distill_recsys --teacher_path`` loads); the command line is
  :mod:`gdd.train_teacher` (``--select_by ndcg``: the reference's selection on validation NDCG)
* :mod:`gdd.rankeval` — :func:`recommend` (ranked top-K lists from a fused score + top-K kernel that
  never writes a score), :func:`rank_metrics` and :class:`RankingEvaluator` (precision, recall and
  NDCG@K as the reference teacher computes them)
* :mod:`gdd.condrank` — :func:`recommend_condensed` / :class:`CondensedRecommender`: the same lists
  from a condensed recommender's cluster tables and maps without expanding them (clusters ranked
  once per user cluster, expanded per user); ``python -m gdd.recommend_distilled`` serves the saved
  artefact
* :mod:`gdd.rankpos` — :func:`rank_positions` / :func:`rank_positions_condensed`: how many items rank
  above given items, for every cut-off, MRR and the mean rank (:class:`PositionEvaluator`,
  :func:`metrics_from_positions`) and for teacher / student :func:`ranking_fidelity`
* :mod:`gdd.agent` / :mod:`gdd.agent_induct` — the transductive and inductive ClustGDD agents;
  :mod:`gdd.train_clustgdd_transduct` / :mod:`gdd.train_clustgdd_induct` /
  :mod:`gdd.distill_recsys` — the drop-in command lines
"""
from . import _lib  # noqa: F401  (imports torch first, see _lib docstring)
from . import gcn, pipeline, rankeval, rankformer, recsys  # noqa: F401
from .cluster import argmax_rows, cluster_mean, group_by_label
from .condrank import CondensedRecommender, recommend_condensed
from .condense import ER_estimator, attaw_ER_estimator, graph_compress, graph_sparse
from .graph import (CSRGraph, induced_subgraph, normalize_adj, normalize_adj_tensor, propagate, spmm,
                    to_csr)
from .kmeans import KMeans, MiniBatchKMeans
from .rankeval import RankingEvaluator, rank_metrics, recommend
from .rankpos import (PositionEvaluator, fidelity, metrics_from_positions, rank_positions,
                      rank_positions_condensed, ranking_fidelity)
from .rankformer import GCNLayer, InteractionGraph, RankformerLayer, RankformerTeacher, save_teacher
from .sharded import ShardedKMeans, shard_rows
from .svd import svd_embeddings, truncated_svd

__all__ = [
    "CSRGraph", "to_csr", "normalize_adj", "normalize_adj_tensor", "propagate", "spmm",
    "KMeans", "MiniBatchKMeans", "ShardedKMeans", "shard_rows", "cluster_mean", "argmax_rows",
    "induced_subgraph", "group_by_label", "graph_sparse", "graph_compress", "ER_estimator", "attaw_ER_estimator",
    "truncated_svd", "svd_embeddings",
    "InteractionGraph", "RankformerLayer", "GCNLayer", "RankformerTeacher", "save_teacher",
    "recommend", "rank_metrics", "RankingEvaluator", "recommend_condensed", "CondensedRecommender",
    "rank_positions", "rank_positions_condensed", "metrics_from_positions", "PositionEvaluator", "fidelity",
    "ranking_fidelity",
]
