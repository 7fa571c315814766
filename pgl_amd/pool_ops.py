"""Front end of the graph-pooling kernels (csrc/pool.hip; pglamd_segment_topk, pglamd_filter_edges_*, include/pgl_amd.h): the
per-graph top-k permutation behind pgl.math.segment_topk (pgl/math.py:276-364) and the edge filter behind
pgl.utils.transform.filter_adj (pgl/utils/transform.py:138-168).  A module of its own beside pgl_amd.ops, whose launch helpers
it uses.  The low-level ops here never fall back to torch; the routing (kernel or today's tensor code) is decided by their
callers: pgl_amd.math.segment_topk, pgl_amd.utils.transform.filter_adj and pgl_amd.nn.SAGPool.

Host reads, function by function (the line that reads is quoted; tests/test_pool_defs.py looks it up in the source):
    topk_supported      none (no device work)
    topk_counts         none (numpy in, numpy out)
    topk_perm           none.  Flags of a bad segment go to the caller's `status` tensor, which topk_check reads
    topk_check          `flags = int(status.item())`
    filter_edges        `kept, flags = status.tolist()`   -- between the counting launches and the fill; the only one
    host_topk_perm, host_filter_edges       host twins: numpy in, numpy out, no device

LAUNCHES counts the calls that reached the library, per op: how a test of the routing tells which path ran."""
import collections

import numpy as np
import torch

from . import _ffi
from .ops import _launch, _np_i64, _np_ptr, _ptr, _scratch, _ws

TOPK_MAX_SEG = 4096          # PGLAMD_TOPK_MAX_SEG: the longest segment one launch sorts
TOPK_FLAGS = ((1, "a segment longer than %d elements (or of negative length)" % TOPK_MAX_SEG),
              (2, "a k outside [0, segment length]"))
FILTER_FLAGS = ((1, "an id of perm or an edge end outside [0, num_nodes)"), (2, "a repeated id in perm"))
LAUNCHES = collections.Counter()
_ROUTE = True                # private switch: False keeps math.segment_topk, filter_adj and SAGPool on their tensor code (tests and
                             # scripts/bench_pool.py run both paths in one build)


class FilterFlag(ValueError):
    """filter_edges found a flag; .flags holds the bits (1: an id out of range, 2: a repeated id in perm)."""

    def __init__(self, msg, flags):
        super(FilterFlag, self).__init__(msg)
        self.flags = flags


def _name(flags, table):
    return " and ".join(w for b, w in table if flags & b)


def topk_supported(max_len):
    """True when a batch whose longest segment has max_len elements is taken by the kernel."""
    return 0 <= int(max_len) <= TOPK_MAX_SEG


def topk_counts(seg_len, ratio):
    """k per segment on the host, numpy int64: min(ratio, len) for an int ratio, else ceil(float32(ratio) * float32(len)) -- the
    value torch.ceil(ratio * seg_len.float()) has on the device."""
    seg_len = np.asarray(seg_len, dtype=np.int64)
    if isinstance(ratio, (int, np.integer)):
        return np.minimum(seg_len, np.int64(ratio))
    return np.ceil(np.float32(ratio) * seg_len.astype(np.float32)).astype(np.int64)


def topk_perm(scores, seg_ptr, out_ptr, total, status=None):
    """perm int64 [total]: perm[out_ptr[s] + j] = the global position of the j-th element of segment s (positions seg_ptr[s] ..
    seg_ptr[s+1]-1 of `scores`) in the order (score descending, position ascending), j < out_ptr[s+1] - out_ptr[s]; IEEE equality,
    NaN above every number (tests/pool_defs.py: topk_perm_restated).  scores fp32 [n]; seg_ptr, out_ptr int64 [S+1] on the same
    device; total = out_ptr[-1], known to the caller.  No host read: a segment longer than TOPK_MAX_SEG or a k outside
    [0, len] is skipped and ORs a bit into `status` (int64 [1] on the device, cleared by the caller; topk_check reads it)."""
    if not (scores.is_cuda and seg_ptr.is_cuda and out_ptr.is_cuda):
        raise ValueError("pgl_amd topk_perm: scores, seg_ptr and out_ptr must be on the GPU (host_topk_perm is the host twin)")
    if scores.dtype != torch.float32 or scores.dim() != 1:
        raise ValueError("pgl_amd topk_perm: scores must be float32 [n], got %s %s" % (scores.dtype, tuple(scores.shape)))
    for name, t in (("seg_ptr", seg_ptr), ("out_ptr", out_ptr)):
        if t.dtype != torch.int64 or t.dim() != 1 or t.device != scores.device:
            raise ValueError("pgl_amd topk_perm: %s must be int64 [S + 1] on %s" % (name, scores.device))
    if seg_ptr.shape != out_ptr.shape or int(seg_ptr.shape[0]) < 1:
        raise ValueError("pgl_amd topk_perm: seg_ptr and out_ptr must both hold S + 1 entries")
    if status is None:
        status = torch.zeros(1, dtype=torch.int64, device=scores.device)
    elif status.dtype != torch.int64 or int(status.numel()) != 1 or status.device != scores.device:
        raise ValueError("pgl_amd topk_perm: status must be int64 [1] on %s" % scores.device)
    scores, seg_ptr, out_ptr = scores.contiguous(), seg_ptr.contiguous(), out_ptr.contiguous()
    perm = torch.empty(int(total), dtype=torch.int64, device=scores.device)
    S = int(seg_ptr.shape[0]) - 1
    if S:
        _launch("segment_topk", scores, _ptr(scores), _ptr(seg_ptr), _ptr(out_ptr), S, _ptr(perm), _ptr(status))
        LAUNCHES["topk_perm"] += 1
    return perm


def topk_check(status):
    """Reads the status of topk_perm calls (one host read); ValueError that names the flag."""
    flags = int(status.item())
    if flags:
        raise ValueError("pgl_amd topk_perm: %s (status %d)" % (_name(flags, TOPK_FLAGS), flags))


def filter_edges(edges, perm, num_nodes):
    """-> (out_edges int64 [kept, 2], out_pos int64 [kept]).  With new_id[perm[i]] = i and -1 elsewhere, the edges whose two ends
    have new_id >= 0, relabelled, and their positions in `edges`, both in input order (tests/pool_defs.py:
    filter_edges_restated).  edges int64 [E, 2] (a row-strided view is read in place), perm int64 [m] of distinct ids in
    [0, num_nodes).  Exactly one host read, of the status pair between count and fill; FilterFlag (a ValueError) that names the
    flag for an id out of range -- never dereferenced -- or a repeated id in perm."""
    if not (edges.is_cuda and perm.is_cuda):
        raise ValueError("pgl_amd filter_edges: edges and perm must be on the GPU (host_filter_edges is the host twin)")
    if edges.dtype != torch.int64 or edges.dim() != 2 or int(edges.shape[1]) != 2:
        raise ValueError("pgl_amd filter_edges: edges must be int64 [E, 2], got %s %s" % (edges.dtype, tuple(edges.shape)))
    if perm.dtype != torch.int64 or perm.dim() != 1 or perm.device != edges.device:
        raise ValueError("pgl_amd filter_edges: perm must be int64 [m] on %s" % edges.device)
    E, m, n, dev = int(edges.shape[0]), int(perm.shape[0]), int(num_nodes), edges.device
    if E > 1 and (edges.stride(1) != 1 or edges.stride(0) < 2):
        edges = edges.contiguous()
    stride = int(edges.stride(0)) if E > 1 else 2
    perm = perm.contiguous()
    status = torch.empty(2, dtype=torch.int64, device=dev)
    ws = _scratch(_ws, "filter_edges", edges, n, E)
    _launch("filter_edges_count", edges, _ptr(edges), stride, E, _ptr(perm), m, n, _ptr(status), _ptr(ws), ws.numel())
    LAUNCHES["filter_edges"] += 1
    kept, flags = status.tolist()
    if flags:
        raise FilterFlag("pgl_amd filter_edges: %s (num_nodes = %d)" % (_name(flags, FILTER_FLAGS), n), flags)
    out_edges = torch.empty((kept, 2), dtype=torch.int64, device=dev)
    out_pos = torch.empty(kept, dtype=torch.int64, device=dev)
    if kept:
        _launch("filter_edges_fill", edges, _ptr(edges), stride, E, n, _ptr(out_edges), _ptr(out_pos), _ptr(ws), ws.numel())
    return out_edges, out_pos


def host_topk_perm(scores, seg_ptr, out_ptr):
    """Host twin of topk_perm (pglamd_segment_topk_host): numpy in -> (perm int64 [out_ptr[-1]], status int).  Entries of a
    skipped segment (status != 0) are -1."""
    scores = np.ascontiguousarray(scores, dtype=np.float32).reshape(-1)
    seg_ptr, out_ptr = _np_i64(seg_ptr).reshape(-1), _np_i64(out_ptr).reshape(-1)
    if seg_ptr.shape != out_ptr.shape or seg_ptr.shape[0] < 1:
        raise ValueError("pgl_amd host_topk_perm: seg_ptr and out_ptr must both hold S + 1 entries")
    if seg_ptr.min() < 0 or seg_ptr.max() > scores.shape[0] or out_ptr[0] != 0 or (np.diff(out_ptr) < 0).any():
        raise ValueError("pgl_amd host_topk_perm: seg_ptr must lie inside the scores and out_ptr start at 0 and not decrease")
    perm = np.full(int(out_ptr[-1]), -1, np.int64)
    status = np.zeros(1, np.int64)
    _ffi.check(_ffi.lib().pglamd_segment_topk_host(_np_ptr(scores), _np_ptr(seg_ptr), _np_ptr(out_ptr), int(seg_ptr.shape[0]) - 1,
                                                   _np_ptr(perm), _np_ptr(status)), "segment_topk_host")
    return perm, int(status[0])


def host_filter_edges(edges, perm, num_nodes):
    """Host twin of filter_edges (pglamd_filter_edges_host): numpy in -> (out_edges [kept, 2], out_pos [kept], flags int).  A flag
    is returned, not raised."""
    edges = np.asarray(edges)
    if edges.ndim != 2 or edges.shape[1] != 2:
        raise ValueError("pgl_amd host_filter_edges: edges must be [E, 2]")
    edges, perm = _np_i64(edges), _np_i64(perm).reshape(-1)
    E = int(edges.shape[0])
    out_edges, out_pos = np.empty((E, 2), np.int64), np.empty(E, np.int64)
    status = np.zeros(2, np.int64)
    _ffi.check(_ffi.lib().pglamd_filter_edges_host(_np_ptr(edges), 2, E, _np_ptr(perm), int(perm.shape[0]), int(num_nodes),
                                                   _np_ptr(out_edges), _np_ptr(out_pos), _np_ptr(status)), "filter_edges_host")
    kept = int(status[0])
    return out_edges[:kept].copy(), out_pos[:kept].copy(), int(status[1])
