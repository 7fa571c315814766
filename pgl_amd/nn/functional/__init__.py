from .graph_op import degree_norm, edge_softmax, graph_pool, graph_norm
from .loss import cross_entropy
from ...embedding_ops import bpr_loss, kge_loss, kge_scores, skip_gram_loss, topk_scores

__all__ = ["degree_norm", "edge_softmax", "graph_pool", "graph_norm", "cross_entropy", "skip_gram_loss", "bpr_loss", "kge_loss", "kge_scores",
           "topk_scores"]
