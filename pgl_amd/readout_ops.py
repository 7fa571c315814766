"""Front end of the attention read-out kernels (csrc/readout.hip; pglamd_attention_readout*, include/pgl_amd.h): the softmax-weighted
sum over each member graph's contiguous rows behind GlobalAttention (pgl/nn/pool.py:174-178) and Set2Set (pgl/nn/pool.py:139-142).
A module of its own beside pgl_amd.pool_ops, whose launch helpers (pgl_amd.ops) it shares.  The op never falls back to torch; the
routing (kernel or today's tensor code) is decided by the layers, pgl_amd.nn.pool.

    s_i = score[i] (gate mode) | <x[i], q[g]> (query mode);  a = softmax of s over segment g;  out[g] = sum_{i in g} a_i x[i]

Host reads: none.  readout_plan works on a HOST seg_ptr (numpy) and uploads its tables once; attention_readout and its backward
read nothing back, allocate through torch's caching allocator only and can be captured in a torch.cuda.graph.

seed_attention_readout (csrc/seed_readout.hip; pglamd_seed_readout*) is the pooling attention of GraphMultisetTransformer on the same plan:
k seeds, shared by all segments, attend over each segment's rows, the softmax taken over the seed axis.

set_attention (csrc/set_attention.hip; pglamd_set_attention*) is the dense attention of the same model's SelfAtt block (MAB.forward)
on fp32 MFMA tiles: per-set queries, sets of up to 128 rows, the softmax over the query axis; see the section at the end of this file.

LAUNCHES counts the calls that reached the library, per op: how a test of the routing tells which path ran."""
import collections

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from .ops import _launch, _ptr, _scratch, _ws_hot

READOUT_PIECE = 256          # PGLAMD_READOUT_PIECE: the most rows of one segment a wave walks
READOUT_MAX_D = 512
GATE, QUERY = 0, 1           # PGLAMD_READOUT_GATE / PGLAMD_READOUT_QUERY
LAUNCHES = collections.Counter()


def readout_supported(d):
    """True when rows of d floats are taken by the kernels."""
    return 1 <= int(d) <= READOUT_MAX_D


def host_pieces(seg_ptr, piece=READOUT_PIECE):
    """The numpy half of readout_plan.  seg_ptr int64 [S + 1], not decreasing -> (pieces int64 [P, 4], long_segs int64 [Lg, 3]):
    pieces = (segment, first row, rows <= piece, part), the segments in order and each one's rows in order, at least one piece per
    segment (an empty segment: one piece of 0 rows); part = -1 for the only piece of its segment, else the piece's number among the
    pieces of all multi-piece ("long") segments; long_segs = (segment, first part, parts)."""
    seg_ptr = np.ascontiguousarray(seg_ptr, dtype=np.int64).reshape(-1)
    if seg_ptr.shape[0] < 2:
        raise ValueError("pgl_amd host_pieces: seg_ptr must hold S + 1 >= 2 entries")
    lens = np.diff(seg_ptr)
    if seg_ptr[0] < 0 or (lens < 0).any():
        raise ValueError("pgl_amd host_pieces: seg_ptr must start at >= 0 and not decrease")
    piece = int(piece)
    count = np.maximum((lens + piece - 1) // piece, 1)
    first = np.concatenate([np.zeros(1, np.int64), np.cumsum(count)])
    seg = np.repeat(np.arange(lens.shape[0], dtype=np.int64), count)
    k = np.arange(int(first[-1]), dtype=np.int64) - first[seg]
    is_long = count > 1
    part0 = np.concatenate([np.zeros(1, np.int64), np.cumsum(np.where(is_long, count, 0))])[:-1]
    pieces = np.stack([seg, seg_ptr[seg] + k * piece, np.clip(lens[seg] - k * piece, 0, piece),
                       np.where(is_long[seg], part0[seg] + k, -1)], 1).astype(np.int64)
    longs = np.flatnonzero(is_long).astype(np.int64)
    return np.ascontiguousarray(pieces), np.ascontiguousarray(np.stack([longs, part0[longs], count[longs]], 1).astype(np.int64))


class ReadoutPlan(object):
    """What the kernels need to know about a batch's segments: the device tables (seg_ptr, pieces, long_segs) and, on the host,
    S, N, the piece count, the long-segment count, the number of parts and the longest segment."""
    __slots__ = ("device", "S", "N", "num_pieces", "num_long", "num_parts", "max_len", "seg_ptr", "pieces", "long_segs")


def readout_plan(seg_ptr_host, device):
    """Host arithmetic on a host int64 seg_ptr [S + 1] (numpy), three uploads, no device read."""
    if isinstance(seg_ptr_host, torch.Tensor):
        if seg_ptr_host.is_cuda:
            raise ValueError("pgl_amd readout_plan: seg_ptr must be a host array (reading a device tensor would be a host read)")
        seg_ptr_host = seg_ptr_host.numpy()
    seg_ptr = np.ascontiguousarray(seg_ptr_host, dtype=np.int64).reshape(-1)
    pieces, longs = host_pieces(seg_ptr)
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError("pgl_amd readout_plan: the plan's tables live on the GPU, got device %s" % device)
    p = ReadoutPlan()
    p.S, p.N = int(seg_ptr.shape[0]) - 1, int(seg_ptr[-1])
    p.num_pieces, p.num_long = int(pieces.shape[0]), int(longs.shape[0])
    p.num_parts = int(longs[:, 2].sum()) if p.num_long else 0
    p.max_len = int(np.diff(seg_ptr).max())
    up = lambda a: torch.from_numpy(a).to(device)
    p.seg_ptr, p.pieces, p.long_segs = up(seg_ptr), up(pieces), up(longs if p.num_long else np.zeros((1, 3), np.int64))
    p.device = p.seg_ptr.device          # (with its index: torch.device("cuda") is not torch.device("cuda:0"))
    return p


def _operands(x, plan, score, query):
    """-> (x, operand, mode) as the library takes them; ValueError for what it does not."""
    if (score is None) == (query is None):
        raise ValueError("pgl_amd attention_readout: exactly one of score / query must be given")
    opnd, mode, name = (score, GATE, "score") if query is None else (query, QUERY, "query")
    for what, t in (("x", x), (name, opnd)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError("pgl_amd attention_readout: %s must be a float32 tensor, got %s" % (what, getattr(t, "dtype", type(t))))
    if x.dim() != 2:
        raise ValueError("pgl_amd attention_readout: x must be [N, d], got %s" % (tuple(x.shape),))
    N, d = int(x.shape[0]), int(x.shape[1])
    if not readout_supported(d):
        raise ValueError("pgl_amd attention_readout: d = %d is outside [1, %d]" % (d, READOUT_MAX_D))
    if not (x.is_cuda and opnd.is_cuda):
        raise ValueError("pgl_amd attention_readout: x and %s must be on the GPU (there is no host path)" % name)
    if not isinstance(plan, ReadoutPlan) or plan.N != N:
        raise ValueError("pgl_amd attention_readout: the plan is for %s rows, x has %d" % (getattr(plan, "N", None), N))
    if plan.device != x.device or opnd.device != x.device:
        raise ValueError("pgl_amd attention_readout: x, %s and the plan must be on one device" % name)
    want = (N,) if mode == GATE else (plan.S, d)
    if tuple(opnd.shape) != want:
        raise ValueError("pgl_amd attention_readout: %s must be %s, got %s" % (name, want, tuple(opnd.shape)))
    # rows must be contiguous (the kernels stream them); a contiguous view at a 4-byte aligned address is read in place, one float at a time
    return x.contiguous(), opnd.contiguous(), mode


def _tables(plan):
    return (_ptr(plan.seg_ptr), plan.S, _ptr(plan.pieces), plan.num_pieces, _ptr(plan.long_segs), plan.num_long, plan.num_parts)


def _workspace(x, plan, d):
    return _scratch(_ws_hot, "attention_readout", x, plan.num_parts, d) if plan.num_long else None


def readout_forward(x, opnd, mode, plan):
    """-> (out [S, d], stats [S, 2]).  x [N, d] and opnd contiguous fp32 on the plan's device (no checks: _operands makes them)."""
    N, d = int(x.shape[0]), int(x.shape[1])
    out = torch.empty((plan.S, d), dtype=torch.float32, device=x.device)
    stats = torch.empty((plan.S, 2), dtype=torch.float32, device=x.device)
    ws = _workspace(x, plan, d)
    _launch("attention_readout", x, _ptr(x), N, d, mode, _ptr(opnd), *_tables(plan), _ptr(out), _ptr(stats),
            _ptr(ws), 0 if ws is None else ws.numel())
    LAUNCHES["attention_readout"] += 1
    return out, stats


def readout_backward(grad, x, opnd, mode, plan, out, stats, need=(True, True)):
    """-> (d x or None, d operand or None); a gradient that is not needed is neither allocated nor stored."""
    N, d = int(x.shape[0]), int(x.shape[1])
    need_x, need_o = bool(need[0]), bool(need[1])
    if not (need_x or need_o):
        return None, None
    grad = grad.contiguous()
    dx = torch.empty_like(x) if need_x else None
    do = torch.empty_like(opnd) if need_o else None
    ws = _workspace(x, plan, d)
    _launch("attention_readout_backward", x, _ptr(grad), _ptr(x), N, d, mode, _ptr(opnd), _ptr(out), _ptr(stats), *_tables(plan),
            int(need_x), int(need_o), _ptr(dx), _ptr(do), _ptr(ws), 0 if ws is None else ws.numel())
    LAUNCHES["attention_readout_backward"] += 1
    return dx, do


class _AttentionReadout(torch.autograd.Function):
    """Saves the inputs, out and the per-segment statistics [S, 2] only: the backward recomputes the weights from them."""

    @staticmethod
    def forward(ctx, x, opnd, mode, plan):
        out, stats = readout_forward(x, opnd, mode, plan)
        ctx.mode, ctx.plan = mode, plan
        ctx.save_for_backward(x, opnd, out, stats)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        x, opnd, out, stats = ctx.saved_tensors
        dx, do = readout_backward(grad, x, opnd, ctx.mode, ctx.plan, out, stats, need=ctx.needs_input_grad[:2])
        return dx, do, None, None


def attention_readout(x, plan, score=None, query=None):
    """out [S, d]: the softmax-weighted sum of each segment's rows of x [N, d] (fp32, GPU, d <= 512).  Exactly one of
    score [N] (gate mode: the weights are the segment softmax of score) and query [S, d] (query mode: of <x[i], query[g]>).  plan:
    readout_plan(seg_ptr, x.device).  An empty segment gives exactly 0.  Differentiable in x and score / query; ValueError for
    CPU tensors, another dtype, an unsupported d or a plan for another row count."""
    x, opnd, mode = _operands(x, plan, score, query)
    if torch.is_grad_enabled() and (x.requires_grad or opnd.requires_grad):
        return _AttentionReadout.apply(x, opnd, mode, plan)
    return readout_forward(x, opnd, mode, plan)[0]


# ------------------------------------------------------------------------------------------------
# seed attention (csrc/seed_readout.hip; pglamd_seed_readout*): the pooling attention of GraphMultisetTransformer
# ------------------------------------------------------------------------------------------------
SEED_MAX_K, SEED_MIN_DIM, SEED_MAX_DIM = 32, 4, 256


def seed_readout_supported(k, dim, num_heads):
    """True when the seed-attention kernels take k seeds on rows of dim floats in num_heads heads: 1 <= k <= 32, 4 <= dim <= 256,
    dim % num_heads == 0 and a head width dim / num_heads that is a power of two >= 4."""
    k, dim, h = int(k), int(dim), int(num_heads)
    if not (1 <= k <= SEED_MAX_K and SEED_MIN_DIM <= dim <= SEED_MAX_DIM and h >= 1 and dim % h == 0):
        return False
    hd = dim // h
    return hd >= 4 and hd & (hd - 1) == 0


def _aligned(t):
    """t contiguous at a 16-byte aligned address (the kernels walk rows in 16-byte lanes): a view that is not is cloned."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _seed_operands(k, v, q, plan, num_heads, key_bias):
    """-> (k, v, q, key_bias) as the library takes them; ValueError for what it does not."""
    for what, t in (("k", k), ("v", v), ("q", q)) + ((("key_bias", key_bias),) if key_bias is not None else ()):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError("pgl_amd seed_attention_readout: %s must be a float32 tensor, got %s" % (what, getattr(t, "dtype", type(t))))
    if k.dim() != 2 or q.dim() != 2 or k.shape != v.shape or q.shape[1] != k.shape[1]:
        raise ValueError("pgl_amd seed_attention_readout: k, v must be [N, dim] and q [seeds, dim], got %s, %s, %s" %
                         (tuple(k.shape), tuple(v.shape), tuple(q.shape)))
    N, dim, seeds = int(k.shape[0]), int(k.shape[1]), int(q.shape[0])
    if not seed_readout_supported(seeds, dim, num_heads):
        raise ValueError("pgl_amd seed_attention_readout: (seeds, dim, heads) = (%d, %d, %d) is outside 1 <= seeds <= %d, %d <= dim <= %d, "
                         "dim %% heads == 0, dim / heads a power of two >= 4" % (seeds, dim, int(num_heads), SEED_MAX_K, SEED_MIN_DIM, SEED_MAX_DIM))
    if not (k.is_cuda and v.is_cuda and q.is_cuda and (key_bias is None or key_bias.is_cuda)):
        raise ValueError("pgl_amd seed_attention_readout: k, v, q and key_bias must be on the GPU (there is no host path)")
    if not isinstance(plan, ReadoutPlan) or plan.N != N:
        raise ValueError("pgl_amd seed_attention_readout: the plan is for %s rows, k has %d" % (getattr(plan, "N", None), N))
    if any(t.device != plan.device for t in (k, v, q) + (() if key_bias is None else (key_bias,))):
        raise ValueError("pgl_amd seed_attention_readout: k, v, q, key_bias and the plan must be on one device")
    if key_bias is not None and tuple(key_bias.shape) != (N,):
        raise ValueError("pgl_amd seed_attention_readout: key_bias must be (%d,), got %s" % (N, tuple(key_bias.shape)))
    return _aligned(k), _aligned(v), _aligned(q), None if key_bias is None else key_bias.contiguous()


def _seed_shape(k, q, num_heads):
    return (int(k.shape[0]), int(k.shape[1]), int(q.shape[0]), int(num_heads))


def seed_readout_forward(k, v, q, bias, plan, num_heads, residual):
    """-> out [S, seeds, dim].  Operands as _seed_operands makes them (no checks)."""
    N, dim, seeds, h = _seed_shape(k, q, num_heads)
    out = torch.empty((plan.S, seeds, dim), dtype=torch.float32, device=k.device)
    ws = _scratch(_ws_hot, "seed_readout", k, plan.num_pieces, plan.num_parts, seeds, dim) if plan.num_long else None
    _launch("seed_readout", k, _ptr(k), _ptr(v), N, dim, _ptr(q), seeds, h, _ptr(bias), int(bool(residual)), *_tables(plan), _ptr(out),
            _ptr(ws), 0 if ws is None else ws.numel())
    LAUNCHES["seed_readout"] += 1
    return out


def seed_readout_backward(grad, k, v, q, bias, plan, num_heads, residual, need=(True, True, True, False)):
    """-> (d k, d v, d q, d key_bias), None where not needed: such a gradient is neither allocated nor stored."""
    N, dim, seeds, h = _seed_shape(k, q, num_heads)
    need = [bool(n) for n in need]
    need[3] = need[3] and bias is not None
    if not any(need):
        return None, None, None, None
    grad = _aligned(grad)
    dk, dv, dq = (torch.empty_like(t) if n else None for t, n in zip((k, v, q), need))
    db = torch.empty_like(bias) if need[3] else None
    ws = _scratch(_ws_hot, "seed_readout", k, plan.num_pieces, plan.num_parts, seeds, dim) if need[2] else None
    _launch("seed_readout_backward", k, _ptr(grad), _ptr(k), _ptr(v), _ptr(q), _ptr(bias), N, dim, seeds, h, int(bool(residual)),
            *_tables(plan), *(int(n) for n in need), _ptr(dk), _ptr(dv), _ptr(dq), _ptr(db), _ptr(ws), 0 if ws is None else ws.numel())
    LAUNCHES["seed_readout_backward"] += 1
    return dk, dv, dq, db


class _SeedReadout(torch.autograd.Function):
    """Saves its inputs only: a node's weights depend on that node alone, so the backward recomputes them."""

    @staticmethod
    def forward(ctx, k, v, q, bias, plan, num_heads, residual):
        ctx.plan, ctx.num_heads, ctx.residual = plan, num_heads, residual
        ctx.save_for_backward(k, v, q, bias)
        return seed_readout_forward(k, v, q, bias, plan, num_heads, residual)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        k, v, q, bias = ctx.saved_tensors
        return seed_readout_backward(grad, k, v, q, bias, ctx.plan, ctx.num_heads, ctx.residual, need=ctx.needs_input_grad[:4]) + (None, None, None)


def seed_attention_readout(k, v, q, plan, num_heads, key_bias=None, residual=True):
    """out [S, seeds, dim]: the seeds q [seeds, dim], shared by all segments, attend over each segment's rows of k / v [N, dim] (fp32, GPU)
    in num_heads heads, the softmax taken over the SEED axis as pgl/nn/gmt_pool.py:97-100 takes it:

        s[n,j,h] = key_bias[n] + <q[j, head h], k[n, head h]> / sqrt(dim);   A = softmax of s over j
        out[g,j, head h] = residual * q[j, head h] + sum_{n in g} A[n,j,h] v[n, head h]

    plan: readout_plan(seg_ptr, k.device).  An empty segment gives residual * q.  key_bias [N] is added in fp32 (-1e9 makes a row's
    weights 1 / seeds, as the reference's mask does).  Differentiable in k, v, q and key_bias; the Function saves its inputs only.
    ValueError for CPU tensors, another dtype, a shape seed_readout_supported refuses or a plan for another row count; an operand that
    is not 16-byte aligned is cloned.  No host read: capturable in a torch.cuda.graph."""
    k, v, q, bias = _seed_operands(k, v, q, plan, num_heads, key_bias)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (k, v, q, bias)):
        return _SeedReadout.apply(k, v, q, bias, plan, int(num_heads), bool(residual))
    return seed_readout_forward(k, v, q, bias, plan, num_heads, residual)


# ------------------------------------------------------------------------------------------------
# set attention (csrc/set_attention.hip; pglamd_set_attention*): the dense attention of MAB (SelfAtt of GraphMultisetTransformer)
# The Function saves its INPUTS ONLY (q, k, v, key_bias): a key column's softmax over the queries is wave-local in the kernel, so the
# backward recomputes S and A with the forward's bits; neither the [n, n] weights nor per-column statistics are kept.
# ------------------------------------------------------------------------------------------------
SET_MAX_N = 128


def set_attention_supported(nq, nk, dim, num_heads):
    """True when the set-attention kernels take nq queries and nk keys of dim floats in num_heads heads: 1 <= nq, nk <= 128 and the
    dim / head-width rule of seed_readout_supported (4 <= dim <= 256, dim % num_heads == 0, dim / num_heads a power of two >= 4)."""
    return 1 <= int(nq) <= SET_MAX_N and 1 <= int(nk) <= SET_MAX_N and seed_readout_supported(1, dim, num_heads)


def _set_operands(q, k, v, num_heads, key_bias):
    """-> (q, k, v, key_bias) as the library takes them; ValueError for what it does not."""
    for what, t in (("q", q), ("k", k), ("v", v)) + ((("key_bias", key_bias),) if key_bias is not None else ()):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
            raise ValueError("pgl_amd set_attention: %s must be a float32 tensor, got %s" % (what, getattr(t, "dtype", type(t))))
    if q.dim() != 3 or k.dim() != 3 or k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2]:
        raise ValueError("pgl_amd set_attention: q must be [B, nq, dim] and k, v [B, nk, dim], got %s, %s, %s" %
                         (tuple(q.shape), tuple(k.shape), tuple(v.shape)))
    B, nq, dim, nk = int(q.shape[0]), int(q.shape[1]), int(q.shape[2]), int(k.shape[1])
    if not set_attention_supported(nq, nk, dim, num_heads):
        raise ValueError("pgl_amd set_attention: (nq, nk, dim, heads) = (%d, %d, %d, %d) is outside 1 <= nq, nk <= %d, %d <= dim <= %d, "
                         "dim %% heads == 0, dim / heads a power of two >= 4" % (nq, nk, dim, int(num_heads), SET_MAX_N, SEED_MIN_DIM, SEED_MAX_DIM))
    if not (q.is_cuda and k.is_cuda and v.is_cuda and (key_bias is None or key_bias.is_cuda)):
        raise ValueError("pgl_amd set_attention: q, k, v and key_bias must be on the GPU (there is no host path)")
    if any(t.device != q.device for t in (k, v) + (() if key_bias is None else (key_bias,))):
        raise ValueError("pgl_amd set_attention: q, k, v and key_bias must be on one device")
    if key_bias is not None and tuple(key_bias.shape) != (B, nk):
        raise ValueError("pgl_amd set_attention: key_bias must be (%d, %d), got %s" % (B, nk, tuple(key_bias.shape)))
    return _aligned(q), _aligned(k), _aligned(v), None if key_bias is None else key_bias.contiguous()


def _set_shape(q, k, num_heads):
    return (int(q.shape[0]), int(q.shape[1]), int(k.shape[1]), int(q.shape[2]), int(num_heads))


def set_attention_forward(q, k, v, bias, num_heads, residual):
    """-> out [B, nq, dim].  Operands as _set_operands makes them (no checks)."""
    out = torch.empty_like(q)
    _launch("set_attention", q, _ptr(q), _ptr(k), _ptr(v), _ptr(bias), *_set_shape(q, k, num_heads), int(bool(residual)), _ptr(out))
    LAUNCHES["set_attention"] += 1
    return out


def set_attention_backward(grad, q, k, v, bias, num_heads, residual, need=(True, True, True)):
    """-> (d q, d k, d v), None where not needed: such a gradient is neither allocated nor computed."""
    need = [bool(n) for n in need[:3]]
    if not any(need) or q.shape[0] == 0:
        return tuple(torch.empty_like(t) if n else None for t, n in zip((q, k, v), need))
    grad = _aligned(grad)
    dq, dk, dv = (torch.empty_like(t) if n else None for t, n in zip((q, k, v), need))
    _launch("set_attention_backward", q, _ptr(grad), _ptr(q), _ptr(k), _ptr(v), _ptr(bias), *_set_shape(q, k, num_heads),
            int(bool(residual)), _ptr(dq), _ptr(dk), _ptr(dv))
    LAUNCHES["set_attention_backward"] += 1
    return dq, dk, dv


class _SetAttention(torch.autograd.Function):
    """Saves its inputs only: the backward recomputes the scores and the weights (the forward's bits) in its one launch."""

    @staticmethod
    def forward(ctx, q, k, v, bias, num_heads, residual):
        ctx.num_heads, ctx.residual = num_heads, residual
        ctx.save_for_backward(q, k, v, bias)
        return set_attention_forward(q, k, v, bias, num_heads, residual)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        q, k, v, bias = ctx.saved_tensors
        return set_attention_backward(grad, q, k, v, bias, ctx.num_heads, ctx.residual, need=ctx.needs_input_grad[:3]) + (None, None, None)


def set_attention(q, k, v, num_heads, key_bias=None, residual=True):
    """out [B, nq, dim]: the queries q [B, nq, dim] of every set attend over its keys k / values v [B, nk, dim] (fp32, GPU) in num_heads
    heads, the softmax taken over the QUERY axis as pgl/nn/gmt_pool.py:97-100 takes it (head h = columns h hd .. (h + 1) hd - 1):

        s[b,i,j,h] = key_bias[b,j] + <q[b,i, head h], k[b,j, head h]> / sqrt(dim);   A[b,:,j,h] = softmax of s[b,:,j,h] over i
        out[b,i, head h] = residual * q[b,i, head h] + sum_j A[b,i,j,h] v[b,j, head h]

    key_bias [B, nk] is added in fp32 (-1e9 makes a key's weights 1 / nq, as the reference's mask does) and gets no gradient (it is
    identically 0).  Differentiable in q, k and v; the Function saves its inputs only, never the [nq, nk] weights.  ValueError, before
    any launch, for CPU tensors, another dtype, mismatched shapes or a shape set_attention_supported refuses; an operand that is not
    contiguous or not 16-byte aligned is copied.  No host read, no atomics, no workspace: capturable in a torch.cuda.graph, and the
    results are a pure function of the arguments, bit for bit, whichever gradients are asked for."""
    q, k, v, bias = _set_operands(q, k, v, num_heads, key_bias)
    if torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v)):
        return _SetAttention.apply(q, k, v, bias, int(num_heads), bool(residual))
    return set_attention_forward(q, k, v, bias, num_heads, residual)
