"""Front end of the attention read-out kernels (csrc/readout.hip; pglamd_attention_readout*, include/pgl_amd.h): the softmax-weighted
sum over each member graph's contiguous rows behind GlobalAttention (pgl/nn/pool.py:174-178) and Set2Set (pgl/nn/pool.py:139-142).
A module of its own beside pgl_amd.pool_ops, whose launch helpers (pgl_amd.ops) it shares.  The op never falls back to torch; the
routing (kernel or today's tensor code) is decided by the layers, pgl_amd.nn.pool.

    s_i = score[i] (gate mode) | <x[i], q[g]> (query mode);  a = softmax of s over segment g;  out[g] = sum_{i in g} a_i x[i]

Host reads: none.  readout_plan works on a HOST seg_ptr (numpy) and uploads its tables once; attention_readout and its backward
read nothing back, allocate through torch's caching allocator only and can be captured in a torch.cuda.graph.

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
