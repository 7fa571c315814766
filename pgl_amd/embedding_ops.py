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

Out of scope: sparse (row-list) gradients and an optimiser step inside the kernel; 16-bit tables; d > 256; per-pair weights.

Host reads: none.  LAUNCHES counts the calls that reached the library, per op."""
import collections

import torch
from torch.autograd.function import once_differentiable

from . import ops
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


def pair_loss_forward(emb, ctx, src, tgt, mode, w_pos, w_neg, need_grad=True):
    """-> (loss [], g [P, 1 + K] or None, d emb [Nu, d] or None).  Operands as _operands makes them, P >= 1 (no checks)."""
    Nu, d, Nv = int(emb.shape[0]), int(emb.shape[1]), int(ctx.shape[0])
    P, T = int(tgt.shape[0]), int(tgt.shape[1])
    # the pairs in source order; a source outside its table is filed under the extra row Nu, which the walk reads nothing for
    key = torch.where((src >= 0) & (src < Nu), src, torch.full_like(src, Nu))
    index = ops.csr_build(key, key, Nu + 1, want_i64=False, check_range=False)
    loss = torch.empty((), dtype=torch.float32, device=emb.device)
    g = torch.empty((P, T), dtype=torch.float32, device=emb.device) if need_grad else None
    demb = torch.empty_like(emb) if need_grad else None
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
