"""Front end of the pair-loss kernel (csrc/pair_loss.hip; pglamd_pair_loss, include/pgl_amd.h): the skip-gram loss of DeepWalk /
metapath2vec (examples/deepwalk/model.py:101-127) and the BPR loss of LightGCN (examples/lightgcn/model.py:158-170) over two embedding
tables, loss and both gradients, without a [P, d] or [P, K, d] tensor in either direction.  A sibling of pgl_amd.attention_ops and
pgl_amd.readout_ops, whose launch helpers (pgl_amd.ops) it shares.  The op never falls back to torch.

    z[p, j] = <emb[src[p]], ctx[tgt[p, j]]>,   tgt [P, 1 + K]: the positive, then K negatives
    "skipgram"   loss = sum_p ( w_pos softplus(-z[p, 0]) + w_neg sum_{j >= 1} softplus(z[p, j]) )       K >= 0
    "bpr"        loss = w_neg sum_p sum_{j >= 1} softplus(z[p, j] - z[p, 0])                            K >= 1

One call: a pglamd_csr_build over the P sources (one sort of P keys), then the walk, which leaves the loss, g = d loss / d z
[P, 1 + K] and d emb.  d ctx is formed in the backward, and only when ctx needs it: ops.aggregate(emb, index by target, y = g,
message_op="mul") over the P (1 + K) entries.  An entry whose target or source is outside its table carries g = 0; in that index it is
POINTED AT ROW 0 WITH WEIGHT 0 rather than dropped (dropping would need the count on the host), so it adds 0 * emb[0] -- exactly 0 for
finite tables.

The step after the loss: sparse_step (csrc/sparse_step.hip; pglamd_sparse_step) sums gradient rows by id and applies SGD, Adagrad,
row-wise Adagrad or lazy Adam to the touched rows alone, at a cost that follows the number of entries, not the table height (the index
build aside); skip_gram_step / bpr_step / kge_step run a fused loss and that step without a table-sized gradient.  Their definition
stands in the comment block above them, at the end of this file.

Out of scope: 16-bit tables; d > 256 for the pair loss; per-pair weights; weight decay; a sort that needs no [N + 1] array; gradients
arriving through autograd hooks.

Further down: the knowledge-graph-embedding scores and loss over chunked negatives (kge_scores / kge_loss, csrc/kge_score.hip), with
their definition in the comment block above them; the filtered link-prediction ranks of their evaluation (kge_ranks, the same unit;
kge_filter builds the filter index from the known triples, kge_metrics turns the counts into MRR / MR / HITS@k); then the masked
top-k retrieval over a table (topk_scores, csrc/topk_scores.hip), likewise.

Host reads: none (kge_*: one for check_range; kge_filter is a setup path and reads two sizes back; kge_metrics reads its result).  LAUNCHES counts the calls that reached the library, per op."""
import collections

import torch
from torch.autograd.function import once_differentiable

from . import _ffi, ops
from .ops import _aligned, _launch, _ptr, _scratch, _ws_hot

PAIR_CHUNK = 32              # kPairChunk: sorted pairs per lane group; a source with more pairs than this is split over chunks
PAIR_MAX_D = 256
MODES = {"skipgram": 0, "bpr": 1}        # PGLAMD_PAIR_SKIPGRAM / PGLAMD_PAIR_BPR
LAUNCHES = collections.Counter()


def pair_loss_supported(d):
    """True when tables with rows of d floats are taken by the kernel: a multiple of 4 up to 256."""
    return 4 <= int(d) <= PAIR_MAX_D and int(d) % 4 == 0


def _operands(emb, ctx, src, tgt, mode):
    """-> (emb, ctx, src, tgt, mode code) as the library takes them; TypeError / ValueError for what it does not."""
    for what, t in (("emb", emb), ("ctx", ctx)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError("pgl_amd pair_loss: %s must be a float32 tensor, got %s" % (what, getattr(t, "dtype", type(t))))
    for what, t in (("src", src), ("tgt", tgt)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
            raise TypeError("pgl_amd pair_loss: %s must be an int64 tensor, got %s" % (what, getattr(t, "dtype", type(t))))
    if mode not in MODES:
        raise ValueError("pgl_amd pair_loss: mode must be one of %s, got %r" % (sorted(MODES), mode))
    if emb.dim() != 2 or ctx.dim() != 2 or emb.shape[1] != ctx.shape[1] or emb.shape[0] < 1 or ctx.shape[0] < 1:
        raise ValueError("pgl_amd pair_loss: emb must be [Nu, d] and ctx [Nv, d], got %s and %s" % (tuple(emb.shape), tuple(ctx.shape)))
    if not pair_loss_supported(emb.shape[1]):
        raise ValueError("pgl_amd pair_loss: d = %d must be a multiple of 4 up to %d" % (emb.shape[1], PAIR_MAX_D))
    if src.dim() != 1 or tgt.dim() != 2 or tgt.shape[0] != src.shape[0] or tgt.shape[1] < 1:
        raise ValueError("pgl_amd pair_loss: src must be [P] and tgt [P, 1 + K], got %s and %s" % (tuple(src.shape), tuple(tgt.shape)))
    if mode == "bpr" and tgt.shape[1] < 2:
        raise ValueError("pgl_amd pair_loss: the BPR loss needs at least one negative (tgt [P, 1 + K], K >= 1)")
    if not (emb.is_cuda and ctx.is_cuda and src.is_cuda and tgt.is_cuda):
        raise ValueError("pgl_amd pair_loss: emb, ctx, src and tgt must be on the GPU (there is no host path)")
    if any(t.device != emb.device for t in (ctx, src, tgt)):
        raise ValueError("pgl_amd pair_loss: emb, ctx, src and tgt must be on one device")
    return _aligned(emb), _aligned(ctx), src.contiguous(), tgt.contiguous(), MODES[mode]


def pair_loss_forward(emb, ctx, src, tgt, mode, w_pos, w_neg, need_grad=True, dense_emb=True):
    """-> (loss [], g [P, 1 + K] or None, d emb [Nu, d] or None).  Operands as _operands makes them, P >= 1 (no checks).
    dense_emb=False: g without the [Nu, d] gradient (the sparse step sums the rows from g)."""
    Nu, d, Nv = int(emb.shape[0]), int(emb.shape[1]), int(ctx.shape[0])
    P, T = int(tgt.shape[0]), int(tgt.shape[1])
    # the pairs in source order; a source outside its table is filed under the extra row Nu, which the walk reads nothing for
    key = torch.where((src >= 0) & (src < Nu), src, torch.full_like(src, Nu))
    index = ops.csr_build(key, key, Nu + 1, want_i64=False, check_range=False)
    loss = torch.empty((), dtype=torch.float32, device=emb.device)
    g = torch.empty((P, T), dtype=torch.float32, device=emb.device) if need_grad else None
    demb = torch.empty_like(emb) if need_grad and dense_emb else None
    ws = _scratch(_ws_hot, "pair_loss", emb, P, d)
    _launch("pair_loss", emb, _ptr(emb), Nu, _ptr(ctx), Nv, d, _ptr(tgt), P, T - 1, _ptr(index.row32), _ptr(index.eid32), _ptr(index.indptr),
            mode, float(w_pos), float(w_neg), _ptr(loss), _ptr(g), _ptr(demb), _ptr(ws), ws.numel())
    LAUNCHES["pair_loss"] += 1
    return loss, g, demb


def pair_loss_backward_ctx(g, emb, src, tgt, num_ctx):
    """d ctx [Nv, d] = sum over the entries (p, j) with tgt[p, j] = t of g[p, j] emb[src[p]]: the engine's edge-weighted sum over an index of
    the P (1 + K) entries by target.  An entry outside a table has g = 0 and is pointed at row 0."""
    Nu, T = int(emb.shape[0]), int(tgt.shape[1])
    key = torch.where((tgt >= 0) & (tgt < num_ctx), tgt, torch.zeros_like(tgt)).reshape(-1)
    col = torch.where((src >= 0) & (src < Nu), src, torch.zeros_like(src)).repeat_interleave(T)
    index = ops.csr_build(key, col, num_ctx, want_i64=False, check_range=False)
    LAUNCHES["pair_loss_backward_ctx"] += 1
    return ops.aggregate(emb, index, "sum", out_size=num_ctx, y=g.reshape(-1, 1), message_op="mul")


class _PairLoss(torch.autograd.Function):
    """Saves g, the unscaled d emb, the ids and emb (the rows d ctx sums); the backward scales by the incoming gradient."""

    @staticmethod
    def forward(fctx, emb, ctx, src, tgt, mode, w_pos, w_neg):
        fctx.num_ctx = int(ctx.shape[0])
        if src.shape[0] == 0:                   # no pair: nothing is launched, the loss and both gradients are zeros
            fctx.save_for_backward(emb)
            return torch.zeros((), dtype=torch.float32, device=emb.device)
        loss, g, demb = pair_loss_forward(emb, ctx, src, tgt, mode, w_pos, w_neg)
        fctx.save_for_backward(emb, src, tgt, g, demb)
        return loss

    @staticmethod
    @once_differentiable
    def backward(fctx, grad):
        if len(fctx.saved_tensors) == 1:
            emb = fctx.saved_tensors[0]
            return (torch.zeros_like(emb) if fctx.needs_input_grad[0] else None,
                    emb.new_zeros((fctx.num_ctx, emb.shape[1])) if fctx.needs_input_grad[1] else None, None, None, None, None, None)
        emb, src, tgt, g, demb = fctx.saved_tensors
        d_emb = demb * grad if fctx.needs_input_grad[0] else None
        d_ctx = pair_loss_backward_ctx(g * grad, emb, src, tgt, fctx.num_ctx) if fctx.needs_input_grad[1] else None
        return d_emb, d_ctx, None, None, None, None, None


def pair_loss(emb, ctx, src, tgt, mode="skipgram", w_pos=None, w_neg=None):
    """The scalar loss of `mode` ("skipgram" | "bpr", see the module text) over emb [Nu, d] and ctx [Nv, d] (fp32, GPU, d a multiple of
    4 up to 256; nn.Embedding weights or any non-leaf tensor), src [P] and tgt [P, 1 + K] int64.  w_pos / w_neg: the caller's weights,
    not renormalised; None: 1 / P ("bpr" reads w_neg only).  Differentiable in emb and ctx; the same tensor may be passed as both and
    autograd adds the two gradients.
    An id outside its table (< 0, >= Nu for src, >= Nv for tgt) is not read: such a negative adds nothing to the loss or to any
    gradient (pad ragged negatives with -1); a pair whose source or positive is outside adds nothing at all.
    P = 0 gives a zero loss with zero gradients.  TypeError for another dtype, ValueError for CPU tensors, d not a multiple of 4 or
    above 256, tgt not [P, 1 + K] or K = 0 in "bpr" mode, all before any launch.
    Without gradients (torch.no_grad(), or neither table requiring one) the walk stores no g and no d emb; the loss has the same bits.
    Bit reproducible: no floating-point atomic in either direction."""
    emb_a, ctx_a, src, tgt, code = _operands(emb, ctx, src, tgt, mode)
    P = int(src.shape[0])
    w_pos = 1.0 / max(P, 1) if w_pos is None else float(w_pos)
    w_neg = 1.0 / max(P, 1) if w_neg is None else float(w_neg)
    if torch.is_grad_enabled() and (emb_a.requires_grad or ctx_a.requires_grad):
        return _PairLoss.apply(emb_a, ctx_a, src, tgt, code, w_pos, w_neg)
    if P == 0:
        return torch.zeros((), dtype=torch.float32, device=emb.device)
    return pair_loss_forward(emb_a, ctx_a, src, tgt, code, w_pos, w_neg, need_grad=False)[0]


def skip_gram_loss(emb, ctx, src, dst, neg, reduction="pair_mean"):
    """The skip-gram loss with negative sampling over src [P], dst [P] and neg [P, K] (K >= 0) as one fused call (pair_loss).
    reduction "pair_mean": -(log sigma(pos) + sum_k log sigma(-neg_k)).mean() over the pairs; "reference":
    (BCEWithLogits(pos, 1) + BCEWithLogits(neg, 0)) / 2 with each term a mean over its own elements (examples/deepwalk/model.py:101-127)."""
    P, K = int(src.shape[0]), int(neg.shape[1]) if neg.dim() == 2 else -1
    if dst.dim() != 1 or neg.dim() != 2 or dst.shape[0] != P or neg.shape[0] != P:
        raise ValueError("pgl_amd skip_gram_loss: src, dst must be [P] and neg [P, K], got %s, %s, %s" % (tuple(src.shape), tuple(dst.shape), tuple(neg.shape)))
    if reduction == "pair_mean":
        w_pos = w_neg = 1.0 / max(P, 1)
    elif reduction == "reference":
        w_pos, w_neg = 0.5 / max(P, 1), 0.5 / max(P * K, 1)
    else:
        raise ValueError("pgl_amd skip_gram_loss: reduction must be 'pair_mean' or 'reference', got %r" % (reduction,))
    return pair_loss(emb, ctx, src, torch.cat([dst.unsqueeze(1), neg], 1), "skipgram", w_pos, w_neg)


def bpr_loss(user_emb, item_emb, users, pos, neg):
    """softplus(<u, n> - <u, p>) averaged over the triples (examples/lightgcn/model.py:158-170) as one fused call (pair_loss): users, pos [P]
    and neg [P] or [P, K] (the mean then runs over all P K differences).  user_emb and item_emb may be one tensor."""
    if neg.dim() == 1:
        neg = neg.unsqueeze(1)
    if pos.dim() != 1 or neg.dim() != 2 or pos.shape[0] != users.shape[0] or neg.shape[0] != users.shape[0]:
        raise ValueError("pgl_amd bpr_loss: users, pos must be [P] and neg [P] or [P, K], got %s, %s, %s" % (tuple(users.shape), tuple(pos.shape), tuple(neg.shape)))
    return pair_loss(user_emb, item_emb, users, torch.cat([pos.unsqueeze(1), neg], 1), "bpr", w_neg=1.0 / max(int(neg.numel()), 1))


# ------------------------------------------------------------------------------------------------
# Knowledge-graph-embedding scores and loss over chunked negatives (csrc/kge_score.hip; pglamd_kge_scores / pglamd_kge_loss /
# pglamd_kge_loss_backward, include/pgl_amd.h): apps/Graph4KG/models/score_funcs.py:76-257 and loss_func.py:70-103.
#
#   ent [Ne, d], rel [Nr, dr] fp32 on the GPU (dr = d; "rotate": d / 2); h, r, t int64 [P], P = C cs (positive i of chunk c is
#   p = c cs + i); neg int64 [C, neg]; neg_head: the negatives replace the head (else the tail).  a = the query of a positive (its kept
#   end combined with the relation), b = an entity row; pos[p] = phi(a_p, other end of p), s[c, i, j] = phi(a_{c,i}, ent[neg[c, j]]):
#     "transe"    a = h + r | t - r                 phi = gamma - sqrt(max(sum_k (a_k - b_k)^2, 1e-30))
#     "distmult"  a = h o r | t o r                 phi = sum_k a_k b_k
#     "complex"   a = h r | t conj(r)  (complex)    phi = sum_k a_k b_k           (all d floats: re and im halves)
#     "rotate"    a = h e^{i th} | t e^{-i th}      phi = gamma - sum_{k < d/2} sqrt((a_re,k - b_re,k)^2 + (a_im,k - b_im,k)^2 + 1e-12)
#                 th = rel / ((gamma + 2) / (d / 2) / pi)        (embed_epsilon = 2.0)
#   re = the first half of a row, im = the second.  TransE takes the difference directly, not the |a|^2 + |b|^2 - 2ab expansion of the
#   reference, which cancels in fp32.  Loss ("Logsigmoid", not pairwise, weights = None):
#     loss = (mean_p softplus(-pos_p) + mean_p sum_j w[p, j] softplus(s[p, j])) / 2
#     w[p, :] = softmax_j(adv_temp s[p, :]) with no gradient through it; adv_temp = 0: the plain mean over j
#   Training stores no score: the forward leaves pos [P] and the softmax state (m, Z) [P, 2]; the backward recomputes the scores tile by
#   tile and leaves ROW gradients (kept end, other end, relation, negatives), which the engine's sum-by-id (ops.aggregate over an index
#   of the ids) adds into d ent and d rel -- no atomics anywhere, bit reproducible.
# ------------------------------------------------------------------------------------------------
KGE_MODELS = {"transe": 0, "distmult": 1, "complex": 2, "rotate": 3}     # PGLAMD_KGE_*
KGE_MAX_D = 1024


def kge_supported(model, d):
    """True when `model` over entity rows of d floats is taken by the kernel: a known model, d a multiple of 8 from 8 to 1024."""
    return model in KGE_MODELS and 8 <= int(d) <= KGE_MAX_D and int(d) % 8 == 0


def _kge_operands(ent, rel, h, r, t, neg, model, check_range):
    """-> (ent, rel, h, r, t, neg, model code, C, cs) as the library takes them; TypeError / ValueError for what it does not."""
    if model not in KGE_MODELS:
        raise ValueError("pgl_amd kge: model must be one of %s, got %r" % (sorted(KGE_MODELS), model))
    for what, x in (("ent", ent), ("rel", rel)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
            raise ValueError("pgl_amd kge: %s must be a float32 tensor, got %s" % (what, getattr(x, "dtype", type(x))))
    for what, x in (("h", h), ("r", r), ("t", t), ("neg", neg)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.int64:
            raise ValueError("pgl_amd kge: %s must be an int64 tensor, got %s" % (what, getattr(x, "dtype", type(x))))
    if ent.dim() != 2 or rel.dim() != 2 or ent.shape[0] < 1 or rel.shape[0] < 1:
        raise ValueError("pgl_amd kge: ent must be [Ne, d] and rel [Nr, dr], got %s and %s" % (tuple(ent.shape), tuple(rel.shape)))
    d = int(ent.shape[1])
    if not kge_supported(model, d):
        raise ValueError("pgl_amd kge: d = %d must be a multiple of 8 from 8 to %d" % (d, KGE_MAX_D))
    dr = d // 2 if model == "rotate" else d
    if int(rel.shape[1]) != dr:
        raise ValueError("pgl_amd kge: model %r with d = %d takes rel of width %d, got %d" % (model, d, dr, rel.shape[1]))
    if h.dim() != 1 or r.shape != h.shape or t.shape != h.shape or neg.dim() != 2 or h.shape[0] < 1 or neg.shape[0] < 1 or neg.shape[1] < 1:
        raise ValueError("pgl_amd kge: h, r, t must be [P] (P >= 1) and neg [C, neg], got %s, %s, %s, %s"
                         % (tuple(h.shape), tuple(r.shape), tuple(t.shape), tuple(neg.shape)))
    P, C = int(h.shape[0]), int(neg.shape[0])
    if P % C:
        raise ValueError("pgl_amd kge: P = %d positives do not divide into the C = %d chunks of neg" % (P, C))
    if not all(x.is_cuda and x.device == ent.device for x in (ent, rel, h, r, t, neg)):
        raise ValueError("pgl_amd kge: every operand must be on one GPU (there is no host path)")
    if check_range and (ops._ids_out_of_range(torch.cat([h, t, neg.reshape(-1)]), int(ent.shape[0])) or ops._ids_out_of_range(r, int(rel.shape[0]))):
        raise ValueError("pgl_amd kge: an id outside its table (h, t, neg in [0, %d), r in [0, %d))" % (ent.shape[0], rel.shape[0]))
    return _aligned(ent), _aligned(rel), h.contiguous(), r.contiguous(), t.contiguous(), neg.contiguous(), KGE_MODELS[model], C, P // C


def _kge_head(ent, rel, h, r, t, neg, code, C, cs, neg_head, gamma):
    """The arguments every kge entry point starts with."""
    return (_ptr(ent), int(ent.shape[0]), _ptr(rel), int(rel.shape[0]), int(ent.shape[1]), _ptr(h), _ptr(r), _ptr(t), _ptr(neg), C, cs,
            int(neg.shape[1]), code, int(bool(neg_head)), float(gamma))


def kge_scores(ent, rel, h, r, t, neg, model, gamma=12.0, neg_head=False, check_range=True):
    """-> (pos [P], s [C, cs, neg]): the scores of the positives and of every positive against its chunk's negatives (the module text
    above; apps/Graph4KG/models/score_funcs.py:76-257), cs = P / C.  For ranking evaluation; no gradient flows through it -- kge_loss
    is the training path.  ValueError before any launch for another dtype, d not a multiple of 8 in 8 .. 1024, rel of the wrong width, P
    not divisible by C, an unknown model, or (check_range: one host read) an id outside its table."""
    ent, rel, h, r, t, neg, code, C, cs = _kge_operands(ent, rel, h, r, t, neg, model, check_range)
    pos = torch.empty(C * cs, dtype=torch.float32, device=ent.device)
    s = torch.empty((C, cs, int(neg.shape[1])), dtype=torch.float32, device=ent.device)
    _launch("kge_scores", ent, *_kge_head(ent, rel, h, r, t, neg, code, C, cs, neg_head, gamma), _ptr(pos), _ptr(s))
    LAUNCHES["kge_scores"] += 1
    return pos, s


def kge_loss_forward(ent, rel, h, r, t, neg, code, C, cs, neg_head, gamma, adv_temp):
    """-> (loss [], pos [P], mz [P, 2]).  Operands as _kge_operands makes them (no checks)."""
    P = C * cs
    loss = torch.empty((), dtype=torch.float32, device=ent.device)
    pos = torch.empty(P, dtype=torch.float32, device=ent.device)
    mz = torch.empty((P, 2), dtype=torch.float32, device=ent.device)
    ws = _scratch(_ws_hot, "kge", ent, P, int(neg.shape[1]))
    _launch("kge_loss", ent, *_kge_head(ent, rel, h, r, t, neg, code, C, cs, neg_head, gamma), float(adv_temp), _ptr(pos), _ptr(mz), _ptr(loss),
            _ptr(ws), ws.numel())
    LAUNCHES["kge_loss"] += 1
    return loss, pos, mz


def kge_row_grads(ent, rel, h, r, t, neg, code, C, cs, neg_head, gamma, adv_temp, pos, mz):
    """-> (ids [2P + n], rows [2P + n, d], g_rel [P, dr]) of the unscaled loss: one gradient row per (positive's kept end, positive's
    other end, negative) with the entity each belongs to, and one per relation use (that of r[p])."""
    P, d, dr, n = C * cs, int(ent.shape[1]), int(rel.shape[1]), int(neg.numel())
    rows = torch.empty((2 * P + n, d), dtype=torch.float32, device=ent.device)         # kept ends, other ends, negatives
    g_rel = torch.empty((P, dr), dtype=torch.float32, device=ent.device)
    _launch("kge_loss_backward", ent, *_kge_head(ent, rel, h, r, t, neg, code, C, cs, neg_head, gamma), float(adv_temp), _ptr(pos), _ptr(mz),
            _ptr(rows), _ptr(rows[P:]), _ptr(g_rel), _ptr(rows[2 * P:]))
    LAUNCHES["kge_loss_backward"] += 1
    return torch.cat([t, h, neg.reshape(-1)] if neg_head else [h, t, neg.reshape(-1)]), rows, g_rel


def kge_loss_backward(ent, rel, h, r, t, neg, code, C, cs, neg_head, gamma, adv_temp, pos, mz, need_ent=True, need_rel=True):
    """-> (d ent [Ne, d] or None, d rel [Nr, dr] or None) of the unscaled loss: the two backward passes leave one gradient row per
    (positive's kept end, positive's other end, negative) and per relation use; the engine's aggregation sums them by id."""
    P = C * cs
    ids, rows, g_rel = kge_row_grads(ent, rel, h, r, t, neg, code, C, cs, neg_head, gamma, adv_temp, pos, mz)
    d_ent = d_rel = None
    if need_ent:
        index = ops.csr_build(ids, torch.arange(ids.shape[0], device=ids.device), int(ent.shape[0]), want_i64=False, check_range=False)
        d_ent = ops.aggregate(rows, index, "sum", out_size=int(ent.shape[0]))
    if need_rel:
        index = ops.csr_build(r, torch.arange(P, device=r.device), int(rel.shape[0]), want_i64=False, check_range=False)
        d_rel = ops.aggregate(g_rel, index, "sum", out_size=int(rel.shape[0]))
    return d_ent, d_rel


class _KgeLoss(torch.autograd.Function):
    """Saves the inputs, pos and (m, Z); the backward recomputes the scores and scales by the incoming gradient."""

    @staticmethod
    def forward(fctx, ent, rel, h, r, t, neg, code, C, cs, neg_head, gamma, adv_temp):
        loss, pos, mz = kge_loss_forward(ent, rel, h, r, t, neg, code, C, cs, neg_head, gamma, adv_temp)
        fctx.save_for_backward(ent, rel, h, r, t, neg, pos, mz)
        fctx.conf = (code, C, cs, neg_head, gamma, adv_temp)
        return loss

    @staticmethod
    @once_differentiable
    def backward(fctx, grad):
        ent, rel, h, r, t, neg, pos, mz = fctx.saved_tensors
        d_ent, d_rel = kge_loss_backward(ent, rel, h, r, t, neg, *fctx.conf, pos, mz, fctx.needs_input_grad[0], fctx.needs_input_grad[1])
        return (None if d_ent is None else d_ent * grad, None if d_rel is None else d_rel * grad) + (None,) * 10


def kge_loss(ent, rel, h, r, t, neg, model, gamma=12.0, neg_head=False, adv_temp=0.0, check_range=True):
    """The Logsigmoid loss of Graph4KG (apps/Graph4KG/models/loss_func.py:70-103; the module text above) over C chunks of cs = P / C
    positives, each chunk scored against its own row of neg [C, neg]; adv_temp > 0: self-adversarial weights softmax_j(adv_temp s), which
    carry no gradient.  Differentiable in ent and rel; no [C, cs, neg] tensor exists in either direction.  The reference's `weights`
    argument (subsampling weights), the pairwise / hinge / BCE losses and 16-bit tables are out of scope.
    Two calls give the same bits (no atomics).  ValueError before any launch as for kge_scores.
    When to use it (profiles/kge/README.md, P = 1024, neg = 256 / 1024, d = 200 / 400 / 800, end-to-end call times): RotatE training
    (1.6-2.4x ahead of the tiled torch recipe at a tenth to a fortieth of its peak memory), and loss-only / ranking passes (RotatE 4.6-17x;
    the other models 1.1-3.9x, level with bmm at d = 800, neg = 1024).  Forward + backward of TransE, DistMult and ComplEx is BEHIND the
    bmm composition in most rows -- DistMult in all, TransE at neg = 1024 and at d = 800, ComplEx in all but neg = 256, d = 200 -- by up to
    6.5x: the backward passes are VALU code on few workgroups."""
    ent, rel, h, r, t, neg, code, C, cs = _kge_operands(ent, rel, h, r, t, neg, model, check_range)
    if not float(adv_temp) >= 0.0:
        raise ValueError("pgl_amd kge_loss: adv_temp must be >= 0, got %r" % (adv_temp,))
    if torch.is_grad_enabled() and (ent.requires_grad or rel.requires_grad):
        return _KgeLoss.apply(ent, rel, h, r, t, neg, code, C, cs, bool(neg_head), float(gamma), float(adv_temp))
    return kge_loss_forward(ent, rel, h, r, t, neg, code, C, cs, bool(neg_head), float(gamma), float(adv_temp))[0]


# ------------------------------------------------------------------------------------------------
# Filtered link-prediction ranks (csrc/kge_score.hip; pglamd_kge_rank, include/pgl_amd.h): the evaluate / calculate_metrics loop of
# apps/Graph4KG/utils.py:116-134, 205-229 -- every test triple against ALL entities, the known true ones masked out -- without a
# [Q, Ne] score tensor.
#
#   ent, rel, h, r, t [Q], model, gamma, neg_head, a_q and phi as above: neg_head=False ranks tails (h, r -> t), True heads
#   (t, r -> h); other_q = the end being ranked.  Candidates: the entity ids j in [lo, hi) within [0, Ne).
#   Filter: an index of device tensors (indptr int64 [R + 1], col32 int32, every row ascending -- the operand form of topk_scores'
#   exclude; kge_filter builds one) and filter_rows int64 [Q]: candidate j is skipped for query q when j is in row filter_rows[q].  A
#   filter_rows[q] outside [0, R) skips nothing; duplicate entries and entries outside [lo, hi) are harmless.
#   With ref_q = phi(a_q, ent[other_q]) and s_qj = phi(a_q, ent[j]) over the candidates j != other_q that are not skipped:
#       greater[q] = #{ s_qj > ref_q }      equal[q] = #{ s_qj == ref_q }       (IEEE comparisons: a NaN counts in neither)
#   int64 [Q].  The reference's rank is greater + 1; the tie-aware ("realistic") rank greater + equal / 2 + 1.
#   ref_q has the bits the sweep gives the pair (q, other_q) -- not those of kge_scores' pos, an fp64 sum -- and the bits of s_qj follow
#   from a_q and ent[j] alone: an entity row that is a bitwise copy of the true row lands in equal, never in greater.
#   Supported: as kge_supported; Ne < 2^31, Q >= 1, hi - lo >= 1.  No gradient flows through the op.
# ------------------------------------------------------------------------------------------------
KGE_RANK_MAX_SLICES = 32     # what a caller may force; the library's own choice goes up to kRankMaxSlices = 512


def kge_ranks(ent, rel, h, r, t, model, gamma=12.0, neg_head=False, filter=None, filter_rows=None, lo=0, hi=None, slices=None,
              check_range=True):
    """-> (greater int64 [Q], equal int64 [Q]): per test triple, how many entities of [lo, hi) other than the true one and those its
    filter row lists score above / exactly as the true one (the comment block above).  One launch that sweeps the entity table; two
    when the range is dealt to several slices -- slices=None lets the library choose from (Q, hi - lo), a number in 1 .. 32 forces it
    (tests, tuning): integer counts, every slice count gives the same result.  No [Q, Ne] tensor, no atomics, no host read beyond
    check_range's: capturable with check_range=False.
    ValueError before any launch for everything kge_scores refuses, for filter without filter_rows or the reverse, an empty or outside
    range, slices outside 1 .. 32.
    When to use it (profiles/kge_rank/README.md, Q = 64 / 1024 / 8192, Ne = 2^17 / 2^20, d = 200 / 400, end-to-end call times beside
    kge_scores against one all-entity chunk + a torch comparison, which cannot filter): whenever a filter is needed or the [Q, Ne] tensor
    is a burden (0.1 MiB against 1.6-13 GiB at Q >= 1024); TransE / DistMult / ComplEx from Q = 1024 up are 1.1-2.0x ahead, Q = 64
    against 2^20 entities 1.0-1.7x.  BEHIND the score block: Q = 64 against 2^17 entities (1.02-1.55x; a call of 0.16-1.4 ms) and RotatE
    in every row (2-13 %: the same VALU work plus the counting).  The filter costs 0-8 %."""
    neg = h.reshape(1, -1)[:, :1] if isinstance(h, torch.Tensor) and h.dim() == 1 and h.shape[0] >= 1 else h      # (a stand-in: no negatives)
    ent, rel, h, r, t, _, code, _, Q = _kge_operands(ent, rel, h, r, t, neg, model, check_range)
    Ne = int(ent.shape[0])
    lo, hi = int(lo), Ne if hi is None else int(hi)
    if Ne >= 2 ** 31 or not 0 <= lo < hi <= Ne:
        raise ValueError("pgl_amd kge_ranks: [lo, hi) = [%d, %d) must be a non-empty range of the Ne = %d < 2^31 entities" % (lo, hi, Ne))
    if (filter is None) != (filter_rows is None):
        raise ValueError("pgl_amd kge_ranks: filter (a sorted index: indptr, col32) and filter_rows ([Q] int64) go together")
    if slices is not None and not 1 <= int(slices) <= KGE_RANK_MAX_SLICES:
        raise ValueError("pgl_amd kge_ranks: slices must be in 1 .. %d, got %r" % (KGE_RANK_MAX_SLICES, slices))
    index = (None, None, 0, 0, None)
    if filter is not None:
        indptr, col = getattr(filter, "indptr", None), getattr(filter, "col32", None)
        if not isinstance(indptr, torch.Tensor) or not isinstance(col, torch.Tensor) or indptr.dtype != torch.int64 or col.dtype != torch.int32 \
                or indptr.dim() != 1 or indptr.shape[0] < 1 or col.dim() != 1:
            raise ValueError("pgl_amd kge_ranks: filter must be an index of device tensors (indptr int64 [R + 1], col32 int32; kge_filter)")
        if not isinstance(filter_rows, torch.Tensor) or filter_rows.dtype != torch.int64 or tuple(filter_rows.shape) != (Q,):
            raise ValueError("pgl_amd kge_ranks: filter_rows must be an int64 tensor [Q] = [%d]" % Q)
        if not all(x.is_cuda and x.device == ent.device for x in (indptr, col, filter_rows)):
            raise ValueError("pgl_amd kge_ranks: every operand must be on one GPU (there is no host path)")
        indptr, col, filter_rows = indptr.contiguous(), col.contiguous(), filter_rows.contiguous()
        index = (_ptr(indptr), _ptr(col), int(indptr.shape[0]) - 1, int(col.shape[0]), _ptr(filter_rows))
    ent, rel = ent.detach(), rel.detach()
    S = int(slices) if slices is not None else int(_ffi.lib().pglamd_kge_rank_slices(Q, hi - lo))
    greater = torch.empty(Q, dtype=torch.int64, device=ent.device)
    equal = torch.empty(Q, dtype=torch.int64, device=ent.device)
    ws = _scratch(_ws_hot, "kge_rank", ent, Q, S) if S > 1 else None
    _launch("kge_rank", ent, _ptr(ent), Ne, _ptr(rel), int(rel.shape[0]), int(ent.shape[1]), _ptr(h), _ptr(r), _ptr(t), Q, code,
            int(bool(neg_head)), float(gamma), *index, lo, hi, S, _ptr(greater), _ptr(equal), _ptr(ws), 0 if ws is None else ws.numel())
    LAUNCHES["kge_rank"] += 1
    return greater, equal


class KgeFilter(object):
    """The sorted filter index of kge_filter: indptr int64 [G + 1] and col32 int32 over the G unique (kept end, relation) pairs of the
    known triples, every row the ascending other ends; keys int64 [G] = kept * num_rel + relation, ascending."""
    __slots__ = ("indptr", "col32", "num_nodes", "keys", "num_rel", "neg_head")

    def __init__(self, indptr, col32, keys, num_rel, neg_head):
        self.indptr, self.col32, self.num_nodes, self.keys, self.num_rel, self.neg_head = indptr, col32, int(keys.shape[0]), keys, num_rel, neg_head

    def rows(self, h, r, t):
        """filter_rows int64 [Q] of query triples: the group of (kept end, relation), -1 where no known triple has the pair."""
        key = (t if self.neg_head else h) * self.num_rel + r
        at = torch.searchsorted(self.keys, key).clamp_(max=self.num_nodes - 1)
        return torch.where(self.keys[at] == key, at, torch.full_like(at, -1))


def kge_filter(h, r, t, num_rel, neg_head=False):
    """The filter of kge_ranks from the known triples h, r, t int64 [T] on the GPU (train + valid + test, as the reference's
    filter_dict): -> a KgeFilter whose rows are the unique (kept end, relation) pairs -- (h, r) for tail ranking, (t, r) when neg_head
    -- each listing the known other ends ascending, built on the device by two stable passes of ops.csr_build (by other end, then by
    group, as Graph._csr_succ_sorted); .rows(h, r, t) finds the rows of query triples by searchsorted.  Setup path: torch.unique reads
    the number of groups back."""
    for what, x in (("h", h), ("r", r), ("t", t)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.int64 or x.dim() != 1 or x.shape != h.shape or not x.is_cuda:
            raise ValueError("pgl_amd kge_filter: %s must be an int64 GPU tensor [T]" % what)
    if h.shape[0] < 1 or int(num_rel) < 1:
        raise ValueError("pgl_amd kge_filter: needs at least one known triple and num_rel >= 1")
    kept, other = (t, h) if neg_head else (h, t)
    if ops._ids_out_of_range(torch.cat([h, t])) or ops._ids_out_of_range(r, int(num_rel)):
        raise ValueError("pgl_amd kge_filter: a negative id, or r outside [0, %d)" % int(num_rel))
    keys, group = torch.unique(kept * int(num_rel) + r, return_inverse=True)
    by_other = ops.csr_build(other, group, int(other.max()) + 1, want_i64=False, check_range=False)
    index = ops.csr_build(by_other.col32.to(torch.int64), by_other.row32.to(torch.int64), int(keys.shape[0]), want_i64=False, check_range=False)
    return KgeFilter(index.indptr, index.col32, keys, int(num_rel), bool(neg_head))


def kge_metrics(greater, equal=None):
    """-> {"MRR", "MR", "HITS@1", "HITS@3", "HITS@10"} over the ranks greater + 1 (apps/Graph4KG/utils.py:116-134), or the tie-aware
    greater + equal / 2 + 1 when equal is given; concatenate both directions' counts for the reference's both-directions figures.  One
    host read."""
    rank = greater.double() + 1.0 if equal is None else greater.double() + equal.double() / 2 + 1.0
    vals = torch.stack([(1.0 / rank).mean(), rank.mean()] + [(rank <= k).double().mean() for k in (1, 3, 10)]).tolist()
    return dict(zip(("MRR", "MR", "HITS@1", "HITS@3", "HITS@10"), vals))


# ------------------------------------------------------------------------------------------------
# Masked top-k retrieval over an embedding table (csrc/topk_scores.hip; pglamd_topk_scores, include/pgl_amd.h): "score every candidate,
# drop what the graph already links, keep the k best" -- the evaluation loop of examples/lightgcn/train.py:93-106 and examples/ngcf
# (getUsersRating -> rating[exclude_index, exclude_items] = -(1 << 10) -> topk) without a [Q, N] score tensor and without a host read.
#
#   query fp32 [Q, d], table fp32 [N, d], bias fp32 [N] or None, candidates [lo, hi) within [0, N).  For candidate j
#       s[q, j] = (sum_c query[q, c] * table[j, c]) + bias[j]
#   the sum over c ascending as ONE fp32 accumulator chain from 0, bias added once after it: the bits of s[q, j] depend on (q, j) alone,
#   never on tile, slice or launch geometry.  bias = -|t_j|^2 / 2 gives nearest-neighbour / TransE-style retrieval; the cancellation of
#   that expansion is the caller's concern.
#   Exclusion: exclude = a successor index whose rows are sorted by dst (the operand of ops.sample_negatives(csr=...): indptr int64,
#   col32), query_ids int64 [Q]; candidate j is dropped for query q when j is a successor of query_ids[q].  Duplicate entries
#   (multi-edges) are harmless; a query_ids[q] outside [0, num_nodes) excludes nothing.
#   Result: ids int64 [Q, k], scores fp32 [Q, k]: per query the first k remaining candidates in the order of ops.segment_topk
#   (csrc/pool_core.hpp) -- score descending then id ascending, IEEE equality (-0.0 ties with +0.0), NaN above every number.  The
#   returned score is the representative of its order class: -0.0 comes back as +0.0 and any NaN as the canonical NaN.  Fewer than k
#   candidates left: the tail is ids = -1, scores = -inf.  No gradient flows through the op (as kge_scores).
#   Supported: d a multiple of 4 in 4 .. 1024, 1 <= k <= 64, hi - lo >= 1, N < 2^31.
# ------------------------------------------------------------------------------------------------
TOPK_MAX_K = 64              # PGLAMD_TOPK_MAX_K
TOPK_MAX_D = 1024
TOPK_MAX_SLICES = 32         # kTopMaxSlices


def topk_supported(d, k):
    """True when tables with rows of d floats and a result of k per query are taken by the kernel: d a multiple of 4 in 4 .. 1024,
    1 <= k <= 64."""
    return 4 <= int(d) <= TOPK_MAX_D and int(d) % 4 == 0 and 1 <= int(k) <= TOPK_MAX_K


def topk_scores(query, table, k, exclude=None, query_ids=None, lo=0, hi=None, bias=None, slices=None):
    """-> (ids int64 [Q, k], scores fp32 [Q, k]): per row of query [Q, d] the k best rows of table[lo:hi] by inner product (+ bias[j]),
    without the candidates that `exclude` lists for query_ids[q] (the module text above has the definition, the order and the tail
    convention).  One launch; two when the candidate range is dealt to several slices -- slices=None lets the library choose from
    (Q, hi - lo), a number forces it (tests, tuning): an exact top-k of a total order, every slice count gives the same bits.  No
    [Q, N] tensor, no host read, no atomics: capturable and bit reproducible.  No gradient flows through it.
    ValueError before any launch for CPU tensors, a dtype other than float32 / int64, exclude without query_ids or the reverse, d not a
    multiple of 4 in 4 .. 1024, k outside 1 .. 64, an empty or outside range, a bias of the wrong length, slices outside 1 .. 32.
    When to use it: profiles/topk_scores/README.md."""
    for what, t in (("query", query), ("table", table)) + ((("bias", bias),) if bias is not None else ()):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError("pgl_amd topk_scores: %s must be a float32 tensor, got %s" % (what, getattr(t, "dtype", type(t))))
    if query.dim() != 2 or table.dim() != 2 or query.shape[1] != table.shape[1] or query.shape[0] < 1 or table.shape[0] < 1:
        raise ValueError("pgl_amd topk_scores: query must be [Q, d] and table [N, d], got %s and %s" % (tuple(query.shape), tuple(table.shape)))
    Q, d, N = int(query.shape[0]), int(query.shape[1]), int(table.shape[0])
    if not topk_supported(d, k):
        raise ValueError("pgl_amd topk_scores: d = %d must be a multiple of 4 in 4 .. %d and k = %s in 1 .. %d" % (d, TOPK_MAX_D, k, TOPK_MAX_K))
    k, lo, hi = int(k), int(lo), N if hi is None else int(hi)
    if N >= 2 ** 31 or not 0 <= lo < hi <= N:
        raise ValueError("pgl_amd topk_scores: [lo, hi) = [%d, %d) must be a non-empty range of the N = %d < 2^31 rows" % (lo, hi, N))
    if bias is not None and tuple(bias.shape) != (N,):
        raise ValueError("pgl_amd topk_scores: bias must be [N] = [%d], got %s" % (N, tuple(bias.shape)))
    if (exclude is None) != (query_ids is None):
        raise ValueError("pgl_amd topk_scores: exclude (a sorted successor index) and query_ids ([Q] int64) go together")
    if slices is not None and not 1 <= int(slices) <= TOPK_MAX_SLICES:
        raise ValueError("pgl_amd topk_scores: slices must be in 1 .. %d, got %r" % (TOPK_MAX_SLICES, slices))
    on = [query, table] + ([bias] if bias is not None else [])
    if exclude is not None:
        if not isinstance(query_ids, torch.Tensor) or query_ids.dtype != torch.int64 or tuple(query_ids.shape) != (Q,):
            raise ValueError("pgl_amd topk_scores: query_ids must be an int64 tensor [Q] = [%d]" % Q)
        if not isinstance(getattr(exclude, "indptr", None), torch.Tensor) or not isinstance(getattr(exclude, "col32", None), torch.Tensor):
            raise ValueError("pgl_amd topk_scores: exclude must be an index of device tensors (Graph._csr_succ_sorted() of a tensor graph)")
        on += [query_ids, exclude.indptr, exclude.col32]
    if not all(t.is_cuda and t.device == query.device for t in on):
        raise ValueError("pgl_amd topk_scores: every operand must be on one GPU (there is no host path)")
    query, table = _aligned(query.detach()), _aligned(table.detach())
    bias = None if bias is None else bias.detach().contiguous()
    S = int(slices) if slices is not None else int(_ffi.lib().pglamd_topk_scores_slices(Q, hi - lo))
    ids = torch.empty((Q, k), dtype=torch.int64, device=query.device)
    scores = torch.empty((Q, k), dtype=torch.float32, device=query.device)
    ws = _scratch(_ws_hot, "topk_scores", query, Q, k, S) if S > 1 else None
    if exclude is None:
        index = (None, None, 0, 0, None)
    else:
        index = (_ptr(exclude.indptr.contiguous()), _ptr(exclude.col32.contiguous()), int(exclude.num_nodes), int(exclude.col32.shape[0]),
                 _ptr(query_ids.contiguous()))
    _launch("topk_scores", query, _ptr(query), Q, _ptr(table), N, d, _ptr(bias), *index, lo, hi, k, S, _ptr(ids), _ptr(scores), _ptr(ws),
            0 if ws is None else ws.numel())
    LAUNCHES["topk_scores"] += 1
    return ids, scores


# ------------------------------------------------------------------------------------------------
# The sparse embedding step (csrc/sparse_step.hip; pglamd_sparse_step, include/pgl_amd.h): what the reference's sparse embeddings do
# after the loss -- the row-wise Adagrad and SGD of pgl/utils/shared_embedding.py:335-348, Adam(lazy_mode=True) of its DeepWalk /
# node2vec / metapath2vec examples, the Adagrad / Adam / SGD of apps/Graph4KG/train.py:58-66.
#
#   table fp32 [N, d] on the GPU, d a multiple of 4 in 4 .. 1024, N < 2^31; M entries (ids[m], col[m], w[m]); the gradient row of entry m
#   is w[m] * rows[col[m]] -- explicit form: rows [M, d], col = None (m itself), w = None (1); gathered form: rows another table (or
#   this one), col int64 [M], w fp32 [M] or None.  An id outside [0, N) is padding: the entry does nothing.  A col outside rows adds a
#   zero row.  Per id that occurs, G = scale * (the sum of its rows), then
#     "sgd"               w -= lr G
#     "adagrad"           s += G^2;  w -= lr G / (sqrt(s) + eps)                             s [N, d]
#     "rowwise_adagrad"   s[id] += mean_k G_k^2;  w -= lr G / (sqrt(s[id]) + 1e-10)         s [N]
#     "lazy_adam"         m = b1 m + (1 - b1) G;  v = b2 v + (1 - b2) G^2;  w -= lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps)
#   Rows whose id does not occur keep their bits, in the table and in every state tensor (lazy Adam: no decay of m, v for them).
#   When rows IS the table (gathered form), other lane groups would read rows this launch rewrites: the sums are stored first
#   (STORE: unique ids, one summed row each, no host read) and applied in explicit form.
# ------------------------------------------------------------------------------------------------
STEP_KINDS = {"sgd": 0, "adagrad": 1, "rowwise_adagrad": 2, "lazy_adam": 3}     # PGLAMD_STEP_*
STEP_STORE = 4
STEP_MAX_D = 1024


class SparseState(object):
    """The optimiser of one table for sparse_step: kind ("sgd" | "adagrad" | "rowwise_adagrad" | "lazy_adam"), lr, eps (None: 1e-10
    for "adagrad", 1e-8 for "lazy_adam"; "rowwise_adagrad" always adds the reference's 1e-10), betas, the state tensors (zeros: "adagrad"
    s [N, d], "rowwise_adagrad" s [N], "lazy_adam" m and v [N, d]) and the step count t, which sparse_step advances."""

    def __init__(self, table, kind, lr, eps=None, betas=(0.9, 0.999)):
        if kind not in STEP_KINDS:
            raise ValueError("pgl_amd SparseState: kind must be one of %s, got %r" % (sorted(STEP_KINDS), kind))
        if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.dim() != 2:
            raise TypeError("pgl_amd SparseState: table must be a float32 tensor [N, d]")
        self.kind, self.lr, self.betas, self.t = kind, float(lr), (float(betas[0]), float(betas[1])), 0
        self.eps = float(eps) if eps is not None else (1e-8 if kind == "lazy_adam" else 1e-10)
        shape = {"sgd": (), "adagrad": ("s",), "rowwise_adagrad": ("s",), "lazy_adam": ("m", "v")}[kind]
        self.tensors = {k: torch.zeros(table.shape[0] if kind == "rowwise_adagrad" else tuple(table.shape), dtype=torch.float32,
                                       device=table.device) for k in shape}

    def state_dict(self):
        return dict(self.tensors, step=torch.tensor(self.t, dtype=torch.int64))

    def load_state_dict(self, sd):
        for k, v in self.tensors.items():
            v.copy_(sd[k])
        self.t = int(sd["step"])


def sparse_step_supported(d):
    """True when tables with rows of d floats are taken by the kernel: a multiple of 4 in 4 .. 1024."""
    return 4 <= int(d) <= STEP_MAX_D and int(d) % 4 == 0


def _step_launch(kind, table, N, rows, col, w, row32, eid32, scale, state=None, t=1, out=(None, None, None)):
    """t: the step this launch is (Adam's bias corrections); the caller advances state.t once the launches went through."""
    d, M = int(rows.shape[1]), int(row32.shape[0])
    hyper, s0, s1 = (0.0,) * 6, None, None
    if state is not None:
        b1, b2 = state.betas
        hyper = (state.lr, state.eps, b1, b2, 1.0 - b1 ** t, 1.0 - b2 ** t)
        s0 = state.tensors.get("s", state.tensors.get("m"))
        s1 = state.tensors.get("v")
    ws = _scratch(_ws_hot, "sparse_step", rows, M, d)
    _launch("sparse_step", rows, _ptr(table), N, d, _ptr(rows), int(rows.shape[0]), _ptr(col), _ptr(w), M, _ptr(row32), _ptr(eid32), float(scale),
            kind, *hyper, _ptr(s0), _ptr(s1), *[_ptr(o) for o in out], _ptr(ws), ws.numel())
    LAUNCHES["sparse_step"] += 1


def _step_index(ids, N):
    """(row32, eid32) of the entries sorted by id (the engine's stable sort), an id outside [0, N) filed under N."""
    key = torch.where((ids >= 0) & (ids < N), ids, torch.full_like(ids, N))
    index = ops.csr_build(key, torch.arange(ids.shape[0], device=ids.device), N + 1, want_i64=False, check_range=False)
    return index.row32, index.eid32


def sparse_sums(ids, rows, N, col=None, w=None, scale=1.0):
    """-> (out_ids int64 [min(M, N)], out_rows [min(M, N), d], count int32 [1]): the unique ids in [0, N) ascending, then -1; per id
    scale * the sum of its entries' rows (the comment block above); count = their number.  Operands as sparse_step checks them, M >= 1."""
    M, d = int(ids.shape[0]), int(rows.shape[1])
    cap = min(M, N)
    out_rows = torch.empty((cap, d), dtype=torch.float32, device=rows.device)
    out_ids = torch.empty(cap, dtype=torch.int64, device=rows.device)
    count = torch.empty(1, dtype=torch.int32, device=rows.device)
    _step_launch(STEP_STORE, None, N, rows, col, w, *_step_index(ids, N), scale, out=(out_rows, out_ids, count))
    return out_ids, out_rows, count


def _apply_sums(table, state, out_ids, out_rows):
    """The explicit-form step state.t + 1 over stored sums: the ids are unique and ascending already, so no sort.  All min(M, N) slots
    are walked, the -1 tail as padding (their number U is on the device only)."""
    N = int(table.shape[0])
    row32 = torch.where(out_ids < 0, torch.full_like(out_ids, N), out_ids).to(torch.int32)
    _step_launch(STEP_KINDS[state.kind], table, N, out_rows, None, None, row32, torch.arange(out_ids.shape[0], dtype=torch.int32, device=out_ids.device),
                 1.0, state, state.t + 1)


def _step_table(table, state):
    """table as the step updates it (a Parameter's data); TypeError / ValueError for a table or state the step does not take."""
    table = table.data if isinstance(table, torch.nn.Parameter) else table
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float32:
        raise TypeError("pgl_amd sparse_step: table must be a float32 tensor, got %s" % (getattr(table, "dtype", type(table)),))
    if not isinstance(state, SparseState):
        raise TypeError("pgl_amd sparse_step: state must be a SparseState")
    if table.dim() != 2 or table.shape[0] < 1 or table.shape[0] >= 2 ** 31 or not sparse_step_supported(table.shape[1]):
        raise ValueError("pgl_amd sparse_step: table must be [N, d], N < 2^31, d a multiple of 4 in 4 .. %d, got %s" % (STEP_MAX_D, tuple(table.shape)))
    shapes = {k: (table.shape[0],) if state.kind == "rowwise_adagrad" else tuple(table.shape) for k in state.tensors}
    if any(tuple(v.shape) != shapes[k] or v.device != table.device for k, v in state.tensors.items()):
        raise ValueError("pgl_amd sparse_step: the state was made for another table")
    if table.is_cuda and (not table.is_contiguous() or table.data_ptr() % 16):
        raise ValueError("pgl_amd sparse_step: the table is updated in place and must be contiguous at a 16-byte aligned address")
    return table


def _step_operands(table, ids, rows, col, w):
    """The entries as the library takes them -> (ids, rows, col, w); table as _step_table left it."""
    for what, t in (("rows", rows),) + ((("w", w),) if w is not None else ()):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise TypeError("pgl_amd sparse_step: %s must be a float32 tensor, got %s" % (what, getattr(t, "dtype", type(t))))
    for what, t in (("ids", ids),) + ((("col", col),) if col is not None else ()):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64:
            raise TypeError("pgl_amd sparse_step: %s must be an int64 tensor, got %s" % (what, getattr(t, "dtype", type(t))))
    if w is not None and col is None:
        raise ValueError("pgl_amd sparse_step: w goes with col (the gathered form)")
    M = ids.shape[0] if ids.dim() == 1 else -1
    if (M < 0 or rows.dim() != 2 or rows.shape[1] != table.shape[1] or rows.shape[0] < 1 - (M == 0) or (col is None and rows.shape[0] != M)
            or any(t is not None and tuple(t.shape) != (M,) for t in (col, w))):
        raise ValueError("pgl_amd sparse_step: ids, col, w must be [M] and rows [R, d = %d] (explicit form: [M, d]), got ids %s, rows %s, col %s, w %s"
                         % ((table.shape[1],) + tuple(None if t is None else tuple(t.shape) for t in (ids, rows, col, w))))
    if not all(t.is_cuda and t.device == table.device for t in (table, ids, rows, col, w) if t is not None):
        raise ValueError("pgl_amd sparse_step: every operand must be on one GPU (there is no host path)")
    return (ids.contiguous(), _aligned(rows.detach()), None if col is None else col.contiguous(), None if w is None else w.detach().contiguous())


def sparse_step(table, ids, rows, state, *, col=None, w=None, scale=1.0):
    """One optimiser step of `state` (a SparseState) on the rows ids [M] int64 of table [N, d], in place, under no_grad: per id that
    occurs, G = scale * the sum of its entries' gradient rows w[m] * rows[col[m]] (explicit form: rows [M, d] alone; gathered form: col
    int64 [M] into rows [R, d], w fp32 [M] or None), then the update of state.kind -- the comment block above has the formulas, padding
    and the route taken when rows is the table itself.  Rows whose id does not occur keep their bits, state included.  Advances
    state.t.  M = 0 launches nothing and advances nothing.  No host read; no floating-point atomic: the same inputs give the same bits.
    TypeError for another dtype or state; ValueError for CPU tensors, d not a multiple of 4 in 4 .. 1024, mismatched shapes, w without
    col, a state made for another table, a table that is not contiguous and 16-byte aligned, explicit rows inside the table's own storage --
    all before any launch."""
    table = _step_table(table, state)
    ids, rows, col, w = _step_operands(table, ids, rows, col, w)
    N = int(table.shape[0])
    if ids.shape[0] == 0:
        return
    aliased = rows.untyped_storage().data_ptr() == table.untyped_storage().data_ptr()       # any view into the table's storage
    if aliased and col is None:
        raise ValueError("pgl_amd sparse_step: explicit rows may not lie in the storage of the table being updated")
    with torch.no_grad():
        if aliased:
            out_ids, out_rows, _ = sparse_sums(ids, rows, N, col, w, scale)
            _apply_sums(table, state, out_ids, out_rows)
        else:
            _step_launch(STEP_KINDS[state.kind], table, N, rows, col, w, *_step_index(ids, N), scale, state, state.t + 1)
        state.t += 1


def _pair_step(emb, ctx, src, tgt, mode, w_pos, w_neg, state_emb, state_ctx):
    """The loss of pair_loss and one sparse step on both tables (emb and ctx may be one tensor with one state): the walk leaves g alone;
    d emb's entries are (src[p], tgt[p, j], g[p, j]) gathered from ctx, d ctx's (tgt[p, j], src[p], g[p, j]) gathered from emb, both from
    the tables as they were before the step.  An entry whose source or target is outside its table is padding."""
    _operands(emb, ctx, src, tgt, mode)
    emb = _step_table(emb, state_emb)
    shared = (ctx.data_ptr(), tuple(ctx.shape)) == (emb.data_ptr(), tuple(emb.shape))
    ctx = emb if shared else _step_table(ctx, state_ctx)
    with torch.no_grad():
        src, tgt = src.contiguous(), tgt.contiguous()
        P, T = int(tgt.shape[0]), int(tgt.shape[1])
        if P == 0:
            return torch.zeros((), dtype=torch.float32, device=emb.device)
        w_pos = 1.0 / P if w_pos is None else float(w_pos)
        w_neg = 1.0 / P if w_neg is None else float(w_neg)
        loss, g, _ = pair_loss_forward(emb, ctx, src, tgt, MODES[mode], w_pos, w_neg, dense_emb=False)
        s_e, t_e, g = src.repeat_interleave(T), tgt.reshape(-1), g.reshape(-1)
        ok = (s_e >= 0) & (s_e < emb.shape[0]) & (t_e >= 0) & (t_e < ctx.shape[0])
        s_e, t_e = torch.where(ok, s_e, torch.full_like(s_e, -1)), torch.where(ok, t_e, torch.full_like(t_e, -1))
        if shared:
            sparse_step(emb, torch.cat([s_e, t_e]), emb, state_emb, col=torch.cat([t_e, s_e]), w=torch.cat([g, g]))
        else:
            ctx_ids, ctx_rows, _ = sparse_sums(t_e, emb, int(ctx.shape[0]), s_e, g)
            sparse_step(emb, s_e, ctx, state_emb, col=t_e, w=g)
            _apply_sums(ctx, state_ctx, ctx_ids, ctx_rows)
            state_ctx.t += 1
    return loss


def skip_gram_step(emb, ctx, src, dst, neg, state_emb, state_ctx=None, reduction="pair_mean"):
    """skip_gram_loss(emb, ctx, src, dst, neg, reduction) -- the same bits -- and one sparse_step of state_emb / state_ctx on the rows
    of emb and ctx the batch touches, from the gradients of that loss at the tables as they were; no [Nu, d] or [P, 1 + K, d] tensor.
    emb and ctx may be one tensor (then state_emb alone is used, and one step is taken with the sum of both gradients)."""
    P, K = int(src.shape[0]), int(neg.shape[1]) if neg.dim() == 2 else -1
    if dst.dim() != 1 or neg.dim() != 2 or dst.shape[0] != P or neg.shape[0] != P:
        raise ValueError("pgl_amd skip_gram_step: src, dst must be [P] and neg [P, K], got %s, %s, %s" % (tuple(src.shape), tuple(dst.shape), tuple(neg.shape)))
    if reduction not in ("pair_mean", "reference"):
        raise ValueError("pgl_amd skip_gram_step: reduction must be 'pair_mean' or 'reference', got %r" % (reduction,))
    w_pos, w_neg = (1.0 / max(P, 1),) * 2 if reduction == "pair_mean" else (0.5 / max(P, 1), 0.5 / max(P * K, 1))
    return _pair_step(emb, ctx, src, torch.cat([dst.unsqueeze(1), neg], 1), "skipgram", w_pos, w_neg, state_emb, state_ctx)


def bpr_step(user_emb, item_emb, users, pos, neg, state_user, state_item=None):
    """bpr_loss(user_emb, item_emb, users, pos, neg) -- the same bits -- and one sparse_step on both tables, as skip_gram_step."""
    if neg.dim() == 1:
        neg = neg.unsqueeze(1)
    if pos.dim() != 1 or neg.dim() != 2 or pos.shape[0] != users.shape[0] or neg.shape[0] != users.shape[0]:
        raise ValueError("pgl_amd bpr_step: users, pos must be [P] and neg [P] or [P, K], got %s, %s, %s" % (tuple(users.shape), tuple(pos.shape), tuple(neg.shape)))
    return _pair_step(user_emb, item_emb, users, torch.cat([pos.unsqueeze(1), neg], 1), "bpr", None, 1.0 / max(int(neg.numel()), 1),
                      state_user, state_item)


def kge_step(ent, rel, h, r, t, neg, model, state_ent, state_rel, gamma=12.0, neg_head=False, adv_temp=0.0, check_range=True):
    """kge_loss(...) -- the same bits -- and one sparse_step of state_ent on the entity rows and of state_rel on the relation rows the
    batch touches: the row gradients of the backward launch go to the step as they are (explicit form), no [Ne, d] gradient exists."""
    if not float(adv_temp) >= 0.0:
        raise ValueError("pgl_amd kge_step: adv_temp must be >= 0, got %r" % (adv_temp,))
    _, _, h, r, t, neg, code, C, cs = _kge_operands(ent, rel, h, r, t, neg, model, check_range)
    ent, rel = _step_table(ent, state_ent), _step_table(rel, state_rel)
    with torch.no_grad():
        conf = (code, C, cs, bool(neg_head), float(gamma), float(adv_temp))
        loss, pos, mz = kge_loss_forward(ent, rel, h, r, t, neg, *conf)
        ids, rows, g_rel = kge_row_grads(ent, rel, h, r, t, neg, *conf, pos, mz)
        sparse_step(ent, ids, rows, state_ent)
        sparse_step(rel, r, g_rel, state_rel)
    return loss
