from .graph_op import degree_norm, edge_softmax, graph_pool, graph_norm
from .loss import cross_entropy
from ...embedding_ops import (SparseState, bpr_loss, bpr_step, kge_filter, kge_loss, kge_metrics, kge_ranks, kge_scores, kge_step, skip_gram_loss,
                              skip_gram_step, sparse_step, topk_scores)

__all__ = ["degree_norm", "edge_softmax", "graph_pool", "graph_norm", "cross_entropy", "skip_gram_loss", "bpr_loss", "kge_loss", "kge_scores",
           "topk_scores", "SparseState", "sparse_step", "skip_gram_step", "bpr_step", "kge_step", "kge_ranks", "kge_filter", "kge_metrics"]
