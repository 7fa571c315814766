"""pgl_amd.ops -- thin Python front end over the C ABI (include/pgl_amd.h).

torch tensors are only the device-memory container (data_ptr + current HIP stream); every op
here is one call into libpglamd.so.  GPU ops refuse CPU tensors: there is no eager / CPU fallback
on the message-passing path.  The host_* functions are the CPU-side helpers of the same library
(numpy in, numpy out) used by numpy-mode graphs and by the partitioner.

Each function names the reference call site it stands in for (reference = PaddlePaddle/PGL 2.2.6).
"""
import collections
import ctypes
import math
import threading

import numpy as np
import os

import torch

from . import _ffi

REDUCE = {"sum": 0, "mean": 1, "max": 2, "min": 3}
MSG = {"add": 0, "sub": 1, "mul": 2, "div": 3}
_DTYPE = {torch.float16: 0, torch.float32: 1, torch.float64: 2, torch.int32: 3, torch.int64: 4, torch.bfloat16: 5}


def _need_cuda(*ts):
    for t in ts:
        if t is not None and type(t).__name__ == "EdgeTensor":
            raise TypeError("pgl_amd.ops: an EdgeTensor (rows in the engine's destination-sorted order, pgl_amd/edge_tensor.py) cannot be "
                            "handed to a kernel as it is -- call .materialize() for the original edge order")
        if t is not None and not t.is_cuda:
            raise RuntimeError("pgl_amd: this op runs only on an MI355X (got a %s tensor); there is no CPU "
                               "fallback for the message-passing path" % t.device)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream(t):
    return ctypes.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ws(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


_WS_HOT = collections.OrderedDict()      # (device, stream, thread) -> buffer, least recently used first
_WS_HOT_MAX = 1 << 29                    # largest request held (512 MiB: the aggregate scratch at |E| = 100 M, d = 128 fp32 is 400 MB)
_WS_HOT_TOTAL = 1 << 30                  # bytes held over all entries; the least recently used ones are dropped beyond it
_WS_HOT_ENTRIES = 16


def set_option(name, value):
    """pglamd_set_option: process-wide TUNING options of the library ("csr_onesweep": tests / experiments).  Launch choices a
    caller makes per graph are per-call arguments (aggregate(deal_chunks=...))."""
    _ffi.check(_ffi.lib().pglamd_set_option(name.encode(), int(value)), "set_option")


def release_workspaces():
    """Drops every cached scratch buffer (they return to torch's caching allocator; torch.cuda.empty_cache() then gives the
    memory back to the device).  Safe at any point: a buffer in use by queued kernels stays alive through the allocator's
    stream ordering."""
    _WS_HOT.clear()


def _ws_hot(nbytes, device):
    """Scratch of the per-step ops (aggregate, segment ops, the GAT kernels): one grow-only buffer per (device, stream, thread)
    instead of an allocator round trip per call.  A kernel's scratch is consumed inside the call that filled it, so calls
    queued on ONE stream can share it; another stream gets its own.  Bounded: requests above 512 MiB are not held,
    at most 16 entries / 1 GiB in total are kept (least recently used dropped first, so entries of finished threads and
    streams age out), nothing is cached while the stream is being captured into a graph (the buffer would escape the
    capture's private pool), and `release_workspaces()` empties the cache."""
    nbytes = max(int(nbytes), 256)
    if nbytes > _WS_HOT_MAX or torch.cuda.is_current_stream_capturing():
        return _ws(nbytes, device)
    # (per thread as well: a library call enqueues its launches with the GIL released, so two threads feeding ONE stream could
    #  interleave them -- thread A's kernel, thread B's kernel, thread A's fix-up reading B's partials)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream, threading.get_ident())
    buf = _WS_HOT.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _WS_HOT[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
        total = sum(b.numel() for b in _WS_HOT.values())
        while len(_WS_HOT) > 1 and (total > _WS_HOT_TOTAL or len(_WS_HOT) > _WS_HOT_ENTRIES):
            k0 = next(iter(_WS_HOT))
            if k0 == key:
                _WS_HOT.move_to_end(k0)
                continue
            total -= _WS_HOT.pop(k0).numel()
    _WS_HOT.move_to_end(key)
    return buf


def _launch(name, on, *args, what=None):
    """pglamd_<name>(*args, stream of `on`) with `on`'s device current; raises through _ffi.check(rc, name) (`what`: the name the
    error message carries where it is not the symbol's)."""
    with torch.cuda.device(on.device):
        _ffi.check(getattr(_ffi.lib(), "pglamd_" + name)(*args, _stream(on)), what or name)


def _scratch(alloc, name, on, *sizes):
    """The scratch pglamd_<name>_workspace_bytes(*sizes) asks for, on `on`'s device, from `alloc`: _ws_hot for the per-step ops,
    _ws for the setup ops (a buffer of its own, which a graph capture may keep)."""
    return alloc(getattr(_ffi.lib(), "pglamd_%s_workspace_bytes" % name)(*sizes), on.device)


def _rows_out(out_size, default):
    """Output rows of an op with an `out_size` argument: out_size when given and positive, else `default`."""
    return int(out_size) if (out_size is not None and int(out_size) > 0) else int(default)


def _seed64(seed):
    return int(seed) & 0xFFFFFFFFFFFFFFFF


def _seed32(seed):
    return int(seed) & 0xFFFFFFFF


def tensor_version(t):
    """t._version, or None for a tensor that tracks none (created under torch.inference_mode(): reading the counter raises
    RuntimeError there -- ADVICE r4).  Callers treat None as "do not cache"."""
    try:
        if t.is_inference():
            return None
        return t._version
    except (RuntimeError, AttributeError):
        return None


def _code(dtype):
    if dtype not in _DTYPE:
        raise TypeError("pgl_amd: unsupported dtype %s" % dtype)
    return _DTYPE[dtype]


def _prod(shape):
    p = 1
    for s in shape:
        p *= int(s)
    return p


def _aligned(t, nbytes=16):
    """`t` as an entry point that reads it in lanes of `nbytes` can take it ("operand layout contract"): contiguous and at an
    address that is a multiple of `nbytes`.  A tensor that already is comes back as it is -- fresh allocations always are -- and a
    contiguous VIEW at an odd storage offset (m.flatten()[1:].view(n, d), a parameter inside a flat buffer) as a fresh copy: the
    kernels refuse such an operand (PGLAMD_E_SHAPE / PGLAMD_E_ARG) rather than read it in lanes wider than its address allows."""
    if t is None:
        return None
    t = t.contiguous()
    return t if t.data_ptr() % nbytes == 0 else t.clone(memory_format=torch.contiguous_format)


def _gat_lane_bytes(H, D, pow2=False):
    """Bytes per lane of the fused attention kernels on their [N, H, D] operands (gat_vec of gat_fused.hip): the narrowest lane of
    1, 2 or 4 floats of one head with which 64 lanes cover H * D columns (pow2: the heads on power-of-two lane spans)."""
    for v in (1, 2, 4):
        lph = D // v
        if D % v == 0 and H * D <= 64 * v and not (pow2 and lph & (lph - 1)):
            return 4 * v
    return 4                                                   # (no width fits: the entry point turns the SHAPE away)


# ------------------------------------------------------------------------------------------------
# CSR build / segment ids
# ------------------------------------------------------------------------------------------------
class CSR(object):
    """The index every aggregation, gather and attention kernel walks: indptr [num_nodes+1] int64 and, per position of the
    key-sorted stream, row32 (key), col32 (the row it reads) and eid32 (edge id; None = the position itself), all int32.
    degree and the reference's int64 arrays (sorted_u / sorted_v / sorted_eid) are None when absent.  max_row: the longest
    row when a caller has measured it (halo plans), 0 = unknown.  y_rows: the rows of an edge operand, 0 = num_edges (an index
    over a SUBSET of a graph's edges addresses the operand by the graph's edge ids).  edge_rows: col32 addresses EDGE rows or
    positions, not node rows (always so when col32 is None: the kernels then read the position as column) -- such an index has
    no hub rows and no per-source scale.  _hub / _es / _pos_by_dst / _slices: caches of this index object alone (hub_plan, edge_scale,
    _src_pos_in_dst_order, slice_plan), None until first filled."""
    __slots__ = ("indptr", "row32", "col32", "eid32", "num_nodes", "num_edges", "degree", "sorted_u", "sorted_v", "sorted_eid",
                 "max_row", "y_rows", "edge_rows", "_hub", "_es", "_pos_by_dst", "_slices")

    def __init__(self, indptr, row32, col32, eid32, num_nodes, num_edges, degree=None, sorted_u=None, sorted_v=None,
                 sorted_eid=None, max_row=0, y_rows=0, edge_rows=False):
        self.indptr, self.row32, self.col32, self.eid32 = indptr, row32, col32, eid32
        self.num_nodes, self.num_edges = int(num_nodes), int(num_edges)
        self.degree, self.sorted_u, self.sorted_v, self.sorted_eid = degree, sorted_u, sorted_v, sorted_eid
        self.max_row, self.y_rows = int(max_row), int(y_rows)
        self.edge_rows = bool(edge_rows) or col32 is None
        self._hub = self._es = self._pos_by_dst = self._slices = None

    def view(self, **changes):
        """A new index sharing every field of this one but `changes`, with empty caches of its own."""
        f = dict(indptr=self.indptr, row32=self.row32, col32=self.col32, eid32=self.eid32, num_nodes=self.num_nodes,
                 num_edges=self.num_edges, degree=self.degree, sorted_u=self.sorted_u, sorted_v=self.sorted_v,
                 sorted_eid=self.sorted_eid, max_row=self.max_row, y_rows=self.y_rows, edge_rows=self.edge_rows)
        f.update(changes)
        return CSR(**f)


def csr_build(u, v, num_nodes, want_i64=True, check_range=True):
    """EdgeIndex.from_edges (pgl/utils/edge_index.py:38-58) / build_index (graph_kernel.pyx:59-88).
    u, v: 1-D int64 CUDA tensors (may be strided views of the [E,2] edge tensor).
    want_i64=False skips the three int64 [E] outputs (sorted_v / sorted_u / sorted_eid stay None): the kernels only
    read the int32 copies, and EdgeIndex widens them on first access -- 480 MB less to write and hold at |E| = 20 M.
    check_range: read back the library's range flag (one host sync; this is the once-per-graph setup path) and raise
    ValueError for keys outside [0, num_nodes), as pglamd_build_index_host does on the host side.  Internal callers whose
    ids are in range by construction (halo plans, sampled blocks) pass False and stay asynchronous."""
    _need_cuda(u, v)
    if u.dtype != torch.int64 or v.dtype != torch.int64:
        u, v = u.to(torch.int64), v.to(torch.int64)
    E, N, dev = int(u.shape[0]), int(num_nodes), u.device
    i64 = dict(dtype=torch.int64, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    sorted_i64 = {k: torch.empty(E, **i64) for k in ("sorted_u", "sorted_v", "sorted_eid")} if want_i64 else {}
    c = CSR(torch.empty(N + 1, **i64), torch.empty(E, **i32), torch.empty(E, **i32), torch.empty(E, **i32), N, E,
            degree=torch.empty(N, **i64), **sorted_i64)
    su = u.stride(0) if E > 0 else 1
    sv = v.stride(0) if E > 0 else 1
    ws = _scratch(_ws, "csr_build", u, E, N)
    flag = torch.zeros(1, dtype=torch.int32, device=dev) if (check_range and E > 0) else None
    _launch("csr_build", u, _ptr(u), su, _ptr(v), sv, E, N, _ptr(c.degree), _ptr(c.sorted_v), _ptr(c.sorted_u), _ptr(c.sorted_eid),
            _ptr(c.indptr), _ptr(c.row32), _ptr(c.col32), _ptr(c.eid32), _ptr(flag), _ptr(ws), ws.numel())
    if flag is not None and int(flag.item()):
        raise ValueError("pgl_amd csr_build: edge ids outside [0, num_nodes=%d) (or >= 2^31); the graph index would be "
                         "garbage -- check num_nodes against the edge list" % N)
    return c


def csr_from_sorted(u_sorted, v, num_nodes, indptr=None, degree=None):
    """The index of edges ALREADY grouped by key (u non-decreasing) -- the blocks a neighbour sampler emits
    (pgl/sampling/sage.py:144-147: `reindex_graph` returns the destinations as repeat_interleave(arange, count)): indptr from
    the run boundaries (pglamd_seg_ptr_from_ids), eid = position, no sort.  The result equals csr_build(u, v) because a stable
    sort leaves a sorted sequence where it is.
    indptr / degree: a caller that holds them already (the relation-wise sampler: its counts ARE the block's degrees) passes them
    and vouches for them; int32 keys are taken as they are, so such a caller's block costs no launch."""
    _need_cuda(u_sorted, v)
    E, N, dev = int(u_sorted.shape[0]), int(num_nodes), u_sorted.device
    row32 = narrow_i64(u_sorted) if u_sorted.dtype == torch.int64 else u_sorted.to(torch.int32).contiguous()
    col32 = narrow_i64(v) if v.dtype == torch.int64 else v.to(torch.int32).contiguous()
    eid32 = torch.arange(E, dtype=torch.int32, device=dev)
    if indptr is None:
        indptr = seg_ptr_from_ids(row32, N)
    return CSR(indptr, row32, col32, eid32, N, E, degree=indptr[1:] - indptr[:-1] if degree is None else degree)


def unique_segment(degree, sorted_u):
    """unique_segment (pgl/utils/helper.py:156-160) on CSR-sorted keys -> (uniq_ind, segment_ids)."""
    _need_cuda(degree, sorted_u)
    N, E, dev = int(degree.shape[0]), int(sorted_u.shape[0]), degree.device
    uniq = torch.empty(N, dtype=torch.int64, device=dev)
    seg = torch.empty(E, dtype=torch.int64, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _scratch(_ws, "unique_segment", degree, E, N)
    _launch("unique_segment", degree, _ptr(degree), _ptr(sorted_u), E, N, _ptr(uniq), _ptr(seg), _ptr(cnt), _ptr(ws), ws.numel())
    return uniq[:int(cnt.item())], seg


def exclusive_scan_i64(t):
    """out[i] = t[0] + ... + t[i-1] (int64) -- pglamd_exclusive_scan_i64 (stands where the reference calls paddle.cumsum)."""
    _need_cuda(t)
    t = t.to(torch.int64).contiguous()
    n = int(t.shape[0])
    out = torch.empty_like(t)
    if n:
        ws = _scratch(_ws_hot, "exclusive_scan_i64", t, n)
        _launch("exclusive_scan_i64", t, _ptr(t), n, _ptr(out), _ptr(ws), ws.numel())
    return out


def narrow_i64(t):
    """int64 (possibly strided) -> contiguous int32."""
    _need_cuda(t)
    n = int(t.shape[0])
    out = torch.empty(n, dtype=torch.int32, device=t.device)
    if n:
        _launch("narrow_i64", t, _ptr(t), t.stride(0), n, _ptr(out))
    return out


# ------------------------------------------------------------------------------------------------
# broadcasting between x[src] tail dims and y tail dims
# ------------------------------------------------------------------------------------------------
def _trailing_ok(tail, out_tail):
    """True iff expanding `tail` to `out_tail` is 'column j reads element j // (dout/d)'."""
    r = len(out_tail)
    t = (1,) * (r - len(tail)) + tuple(tail)
    k = 0
    while k < r and t[k] == out_tail[k]:
        k += 1
    return all(s == 1 for s in t[k:])


def _bcast(x, y):
    """Returns (x2, y2, out_tail) with both operands in a layout the C ABI's trailing-dim rule covers."""
    xt, yt = tuple(x.shape[1:]), tuple(y.shape[1:])
    out_tail = tuple(torch.broadcast_shapes(xt, yt))
    if not _trailing_ok(xt, out_tail):
        x = x.reshape((x.shape[0],) + (1,) * (len(out_tail) - len(xt)) + xt).expand((x.shape[0],) + out_tail)
    if not _trailing_ok(yt, out_tail):
        y = y.reshape((y.shape[0],) + (1,) * (len(out_tail) - len(yt)) + yt).expand((y.shape[0],) + out_tail)
    return x.contiguous(), y.contiguous(), out_tail


# ------------------------------------------------------------------------------------------------
# aggregation (send_u_recv / send_ue_recv)
# ------------------------------------------------------------------------------------------------
_GAT_BWD_EDGE_BUFFER = os.environ.get("PGLAMD_GAT_BWD_EDGE_BUFFER", "1") != "0"
_GAT_POS_STATS = os.environ.get("PGLAMD_GAT_POS_STATS", "1") != "0"
# ---- hub table (round 6) -----------------------------------------------------------------------------------------------------------
# On a power-law graph most gathers go to a few thousand source rows (RMAT-20, 20 M edges: the top 32 768 rows by out-degree are read by
# 71 % of the edges).  Scattered over the [N, d] matrix they are spread over every DRAM page of it; packed into ONE contiguous table
# (16 MB) they are not.  Per call the hub rows are gathered into the table (12 us) and the launch takes the existing two-table path
# (pglamd_aggregate_ext: x2 = the table, the hubs' column ids remapped ONCE per index to N + rank): same edges in the same order, same
# values -- the result is bit-identical.  Measured (profiles/r06/hub_c2.txt, hub_c2p.txt, pmc_hub.txt): 1.134 -> 1.089 + 0.012 ms at
# |E| = 20 M, 6.58 -> 6.19 ms at |E| = 100 M; L2 misses, fetched bytes and translation misses are unchanged, so the gain is on the
# memory side of the fabric.  Used for plain fp32 rows of >= 384 bytes on indices of >= 8 M edges whose top rows cover >= 25 % of the
# edges (a uniform graph has no hubs: nothing to gain); PGLAMD_HUB_TABLE=0 switches it off.
_HUB_TABLE = os.environ.get("PGLAMD_HUB_TABLE", "1") != "0"
_HUB_MIN_EDGES = int(os.environ.get("PGLAMD_HUB_MIN_EDGES", "8000000"))
_HUB_TABLE_BYTES = 16 << 20
_HUB_MAX_ROWS = 32768
_HUB_MIN_COVER = 0.25


def hub_plan(csr, n_src, row_bytes):
    """-> (hub_ids int32 [K], col32 with the hubs remapped to n_src + rank) for this index, or None when a table would not pay.
    Built once per (index, K, n_src) on the device (one host read: the coverage) and cached on the index."""
    K = int(min(_HUB_MAX_ROWS, _HUB_TABLE_BYTES // max(int(row_bytes), 1), n_src // 8))
    if K < 1024:
        return None
    if csr._hub is None:
        csr._hub = {}
    cache = csr._hub
    key = (K, int(n_src))
    if key not in cache:
        if csr.col32.is_cuda and torch.cuda.is_current_stream_capturing():       # (the coverage read is a host sync: not inside a graph capture)
            return None
        col = csr.col32.long()
        deg = torch.bincount(col, minlength=n_src)[:n_src]
        ids = torch.argsort(deg, descending=True, stable=True)[:K]
        cover = float(deg[ids].sum()) / max(int(csr.num_edges), 1)
        if cover < _HUB_MIN_COVER:
            cache[key] = None
        else:
            rank = torch.full((n_src,), -1, dtype=torch.int64, device=col.device)
            rank[ids] = torch.arange(K, device=col.device)
            r = rank[col]
            cache[key] = (ids.to(torch.int32).contiguous(), torch.where(r >= 0, r + n_src, col).to(torch.int32).contiguous(), cover)
    return cache[key]


def hub_table(csr, x):
    """hub_plan for an aggregation of the plain rows x over csr, or None where no table is used.  Eligible: fp32 [n, d] rows of
    >= 384 bytes over an index of >= _HUB_MIN_EDGES edges whose columns are NODE rows -- an edge-row index (csr.edge_rows) reads
    every row once, so it has no hubs, and is turned away before any device work."""
    if csr.edge_rows or not _HUB_TABLE or x.dim() != 2 or x.dtype != torch.float32 or int(x.shape[1]) * 4 < 384 \
            or csr.num_edges < _HUB_MIN_EDGES or int(x.shape[0]) >= (1 << 30):
        return None
    return hub_plan(csr, int(x.shape[0]), int(x.shape[1]) * 4)


# ---- per-XCD hub slices -------------------------------------------------------------------------------------------------------------
# The eight XCDs' private L2s all cache the SAME hottest hub rows.  For rows longer than _SLICE_ROW_MIN edges the hub edges are taken
# out of the row and summed as eight virtual rows, one per residue of the hub's rank modulo 8, whose blocks run on the XCD of that
# residue (agg_flat_kernel, SLICED): every XCD then keeps one eighth of the hub table.  pglamd_aggregate_sliced walks the re-ordered
# stream in one launch and adds the eight partial rows to the row's own remainder in a fixed order.
_HUB_SLICES = os.environ.get("PGLAMD_HUB_SLICES", "1") != "0"
_SLICE_MIN_EDGES = int(os.environ.get("PGLAMD_SLICE_MIN_EDGES", "8000000"))
_SLICE_ROW_MIN = int(os.environ.get("PGLAMD_SLICE_ROW_MIN", "128"))
_SLICE_MIN_ROWS = 64
_SLICES = 8                              # one per XCD (csrc/common.hpp: kXcds)

SlicePlan = collections.namedtuple("SlicePlan", ["row32", "col32", "indptr", "long_rows", "n_long", "out_rows", "row_min", "chunk",
                                                 "seg_edges", "blocks", "blocks_dev", "n_blocks", "hub_ids"])


def _flat_chunk(num_edges):
    """Edges per chunk of the flat kernel for a stream of num_edges edges (csrc/aggregate.hip: chunk_edges_for)."""
    env = os.environ.get("PGLAMD_CHUNK")
    if env is not None:
        try:
            v = int(env)
        except ValueError:
            v = 0
        return max(v, 8) // 8 * 8
    return 256 if num_edges >= 12000000 else 128 if num_edges >= 5000000 else 64


def slice_blocks(seg_edges, num_edges, chunk):
    """-> (blocks, n_blocks): blocks[s] / blocks[9 + s] = first 4-chunk block and block count of segment s (0 = the rest stream,
    1 + s = slice s) on the launch's block grid; a block that straddles two segments belongs to the earlier one."""
    per = 4 * int(chunk)
    n_blocks = (int(num_edges) + per - 1) // per
    first = [0] + [min(-(-int(e) // per), n_blocks) for e in seg_edges[1:_SLICES + 1]] + [n_blocks]
    return first[:_SLICES + 1] + [first[s + 1] - first[s] for s in range(_SLICES + 1)], n_blocks


def slice_plan(csr, hub, n_src, out_rows, row_min=None):
    """The edge stream pglamd_aggregate_sliced walks for this index, or None where it does not apply (no hub plan, fewer than
    _SLICE_MIN_ROWS rows longer than row_min, a graph capture in progress).  Torch ops only, so it also runs on CPU tensors.

    rest stream: every edge that is not a hub edge of a row longer than row_min, rows and order as in the index, hubs as n_src + rank;
    slice s:     the hub edges of those long rows whose source has rank % 8 == s, in index order; the edges of (s, i-th long row) form
                 the virtual row out_rows + s * n_long + i.
    indptr covers the out_rows real rows and the 8 * n_long virtual ones.  Cached on the index per (hub plan, out_rows, row_min)."""
    if hub is None:
        return None
    row_min = _SLICE_ROW_MIN if row_min is None else int(row_min)
    if csr._slices is None:
        csr._slices = {}
    key = (int(hub[0].shape[0]), int(n_src), int(out_rows), row_min)
    if key not in csr._slices:
        if csr.row32.is_cuda and torch.cuda.is_current_stream_capturing():     # (host reads below: not inside a graph capture)
            return None
        csr._slices[key] = _build_slice_plan(csr, hub, int(n_src), int(out_rows), row_min)
    return csr._slices[key]


def _build_slice_plan(csr, hub, n_src, out_rows, row_min):
    dev = csr.row32.device
    n, E = csr.num_nodes, csr.num_edges
    if out_rows < n:
        return None
    deg = csr.indptr[1:] - csr.indptr[:-1]
    long_rows = torch.nonzero(deg > row_min).reshape(-1)
    R = int(long_rows.shape[0])
    if R < _SLICE_MIN_ROWS or out_rows + _SLICES * R >= (1 << 31) - 1:
        return None
    row, col = csr.row32.long(), hub[1].long()
    idx = torch.full((n,), -1, dtype=torch.int64, device=dev)
    idx[long_rows] = torch.arange(R, device=dev)
    i_long = idx[row]
    sliced = (col >= n_src) & (i_long >= 0)
    vrow = torch.where(sliced, out_rows + ((col - n_src) % _SLICES) * R + i_long, row)
    order = torch.argsort(vrow, stable=True)
    n_rows = out_rows + _SLICES * R
    indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    torch.cumsum(torch.bincount(vrow, minlength=n_rows), 0, out=indptr[1:])
    seg_edges = [0] + [int(v) for v in indptr[out_rows + R * torch.arange(_SLICES + 1, device=dev)].tolist()]
    chunk = _flat_chunk(E)
    blocks, n_blocks = slice_blocks(seg_edges, E, chunk)
    return SlicePlan(vrow[order].to(torch.int32).contiguous(), col[order].to(torch.int32).contiguous(), indptr,
                     long_rows.to(torch.int32).contiguous(), R, out_rows, row_min, chunk, seg_edges, blocks,
                     torch.tensor(blocks, dtype=torch.int32, device=dev), n_blocks, hub[0])


def slice_table(csr, x, hub, out_rows, out=None):
    """slice_plan for a plain fp32 sum of the rows x over csr into out_rows rows (hub: the call's hub_table), or None where the
    sliced path is not taken: PGLAMD_HUB_SLICES=0, fewer than _SLICE_MIN_EDGES edges, a width the sliced kernel is not built for
    (one tile of 8- or 16-byte lanes: even d up to 128, multiples of 4 up to 256), or an x / out (a view at an odd storage offset)
    that is not 16-byte aligned -- the library refuses those (PGLAMD_E_ARG); the other entry points serve them."""
    d = int(x.shape[1])
    if not _HUB_SLICES or csr.num_edges < _SLICE_MIN_EDGES or not (d % 4 == 0 and d <= 256 or d % 2 == 0 and d <= 128) \
            or x.data_ptr() % 16 or (out is not None and out.data_ptr() % 16):
        return None
    return slice_plan(csr, hub, int(x.shape[0]), out_rows)


def _aggregate_sliced(x, sp, out):
    """pglamd_aggregate_sliced over a slice_plan: table gather, the one sliced launch, fix-up and combine on x's stream."""
    d, E, K = int(x.shape[1]), int(sp.row32.shape[0]), int(sp.hub_ids.shape[0])
    ws = _scratch(_ws_hot, "aggregate_sliced", x, E, d, K, sp.n_long, sp.chunk)
    blocks = (ctypes.c_int32 * len(sp.blocks))(*sp.blocks)
    _launch("aggregate_sliced", x, _ptr(x), int(x.shape[0]), d, _ptr(sp.hub_ids), K, _ptr(sp.row32), _ptr(sp.col32), _ptr(sp.indptr), E,
            sp.out_rows, _ptr(sp.long_rows), sp.n_long, ctypes.cast(blocks, ctypes.c_void_p), _ptr(sp.blocks_dev), sp.chunk, _ptr(out),
            _ptr(ws), ws.numel())
    return out


_PRESCALE_ROW_BYTES = int(os.environ.get("PGLAMD_PRESCALE_ROW_BYTES", "704"))
_EDGE_SCALE = os.environ.get("PGLAMD_EDGE_SCALE", "1") != "0"


def edge_scale(csr, scale):
    """scale[col[p]] for every position p of the index's sorted stream ([E] fp32), cached on the index: the per-source scale of
    an aggregation (GCN's degree norm, pgl/nn/conv.py:242) in the layout the kernels read sequentially.  The cache entry is keyed
    by the scale vector's storage, offset, length and version counter and HOLDS the vector, so the address cannot be reused by
    another tensor while the entry lives; an in-place update of the vector bumps the version and rebuilds the entry."""
    scale = scale.reshape(-1)
    if not scale.is_contiguous():
        scale = scale.contiguous()
    ver = tensor_version(scale)
    key = None if ver is None else (scale.untyped_storage().data_ptr(), scale.storage_offset(), scale.numel(), ver, str(scale.device))
    hit = csr._es
    if key is not None and hit is not None and hit[0] == key:
        return hit[2]
    es = gather_rows(scale.reshape(-1, 1), csr.col32).reshape(-1)
    if key is not None:                                       # (inference-mode tensors carry no version counter: not cached)
        csr._es = (key, scale, es)
    return es


def _row_strided(t):
    """True for a 2-D column block of a wider row-major matrix (t = m[:, a:b]): rows are contiguous, the row stride is not
    the row length.  pglamd_aggregate_ext / pglamd_gather_rows_cast take such views as they are (ldx / ldout)."""
    return t.dim() == 2 and t.shape[1] > 0 and t.stride(1) == 1 and t.stride(0) > t.shape[1] and not t.is_contiguous()


AggregateRoute = collections.namedtuple("AggregateRoute", ["entry", "scale", "ldx", "ldo"])


def _aggregate_route(x, csr, y, src_scale, x2, zero_indptr, out, reduce_op, deal_chunks):
    """Which library entry point an aggregate() call takes and in which form its per-source scale travels -> AggregateRoute(entry,
    scale, ldx, ldo).  Reads shapes, dtypes, strides, csr.max_row, csr.edge_rows and the tuning globals only: no device work.

    scale (None without src_scale):
      "edge"      fp32 sum / mean rows wider than 128 bytes over node columns, no y: the scale of every edge's source laid out
                  along the sorted stream once per (index, scale vector) and cached on the index (edge_scale) -- 4 sequential
                  bytes per edge, neither a pass over [N, d] nor a random 4-byte read per edge (round 4; PGLAMD_EDGE_SCALE=0: off)
      "prescale"  floating rows of <= _PRESCALE_ROW_BYTES, no y: x * scale first -- one pass over [N, d] (0.17 ms at d = 128 fp32)
                  is cheaper than the fused form's random read per EDGE (+0.25 ms at 20 M edges) up to ~700-byte rows
      "fused"     everything else (an edge operand y, max / min on wider rows, wide non-fp32 rows): the kernel reads scale[col];
                  the library takes it for floating sum / mean only and answers anything else with ValueError
    ldx / ldo: row strides of x / out when they are column blocks of wider matrices (only without y, src_scale and x2), else 0.

    What each entry point honours:
                      x2  zero_indptr  ldx / ldo  max_row  deal_chunks  y  "edge" scale  "fused" scale  hub table
      aggregate_ext   yes     yes         yes       yes        yes     yes     yes            no           yes
      aggregate        no      no          no     ignored    ignored   yes     yes           yes            no
    aggregate_ext is taken when one of its first five options is present and the scale is not "fused".  max_row and deal_chunks
    are hints: a fused scale drops them.  x2 excludes src_scale and zero_indptr excludes a fused one (ValueError): the plain entry
    point would read x2's rows out of x and zero-fill by the index's own indptr."""
    ldx = ldo = 0
    if y is None and src_scale is None and x2 is None:
        if _row_strided(x):
            ldx = int(x.stride(0))
        if out is not None and _row_strided(out):
            ldo = int(out.stride(0))
    if x2 is not None and (x2.dtype != x.dtype or tuple(x2.shape[1:]) != tuple(x.shape[1:]) or src_scale is not None):
        raise ValueError("aggregate: x2 must have x's dtype and row shape, and excludes src_scale")
    scale = None
    if src_scale is not None:
        row_bytes = _prod(x.shape[1:]) * x.element_size()
        per_row = y is None and x.dim() >= 2 and src_scale.numel() == x.shape[0]
        if per_row and _EDGE_SCALE and not csr.edge_rows and x.dtype == torch.float32 and src_scale.dtype == torch.float32 \
                and reduce_op in ("sum", "mean") and row_bytes > 128:
            scale = "edge"
        elif per_row and x.is_floating_point() and row_bytes <= _PRESCALE_ROW_BYTES:
            scale = "prescale"
        else:
            scale = "fused"
    if scale == "fused" and zero_indptr is not None:
        raise ValueError("aggregate: zero_indptr excludes a fused src_scale (one with an edge operand y, a max / min reduce or non-fp32 "
                         "rows wider than %d bytes) -- multiply x by the scale first" % _PRESCALE_ROW_BYTES)
    ext = x2 is not None or zero_indptr is not None or csr.max_row > 0 or ldx > 0 or ldo > 0 or bool(deal_chunks)
    return AggregateRoute("aggregate_ext" if ext and scale != "fused" else "aggregate", scale, ldx, ldo)


def aggregate(x, csr, reduce_op="sum", out_size=None, y=None, message_op="add", src_scale=None, dst_scale=None,
              out=None, accumulate=False, x2=None, zero_indptr=None, deal_chunks=False):
    """paddle.geometric.send_u_recv / send_ue_recv (pgl/graph.py:859-861, 885-887, 929-937) over the
    graph's cached dst-CSR.  y (if given) is in ORIGINAL edge order, shape [E, ...].
    accumulate: False / 0 write every row of `out`; True / 1 combine the rows that receive edges with their old contents;
    2 overwrite only the rows that receive edges (include/pgl_amd.h).
    x2 / zero_indptr (pglamd_aggregate_ext, row-partitioned graphs): column ids >= x.shape[0] read row (id - x.shape[0]) of
    x2 (the rows received from peers); rows are zero-filled where zero_indptr -- not the index's own indptr -- says they
    have no edge.  An index carrying `max_row` (longest row) lets the library skip the split-row fix-up launches.
    x and out may be COLUMN BLOCKS of wider matrices (m[:, a:b]; no edge operand, no src_scale, no x2): the kernels walk them
    with the parent's row stride, nothing is copied.
    deal_chunks (PGLAMD_AGG_DEAL_CHUNKS, per call): the chunks of the edge stream are dealt round the XCDs instead of running in
    contiguous blocks per XCD -- for indices whose row order correlates with row length (HaloPlan(row_order="peers")).
    _aggregate_route says which entry point a call takes and which of these options that entry point honours.  Where hub_table
    applies, a plain fp32 "sum" (no dst_scale, no accumulate) over >= _SLICE_MIN_EDGES edges goes to pglamd_aggregate_sliced instead
    (slice_table): same sums in another, fixed association."""
    _need_cuda(x, y, src_scale, dst_scale, x2, zero_indptr)
    route = _aggregate_route(x, csr, y, src_scale, x2, zero_indptr, out, reduce_op, deal_chunks)
    ldx, ldo = route.ldx, route.ldo
    if not ldx:
        x = x.contiguous()
    if x2 is not None:
        x2 = x2.contiguous()
    es = None
    if route.scale == "edge":
        es = edge_scale(csr, src_scale)
    elif route.scale == "prescale":
        x = x * src_scale.reshape((-1,) + (1,) * (x.dim() - 1)).to(x.dtype)
    if route.scale != "fused":
        src_scale = None
    M = _rows_out(out_size, x.shape[0])
    if y is not None:
        if y.dtype != x.dtype:
            y = y.to(x.dtype)
        # (an index over a SUBSET of a graph's edges -- the interior / boundary indices of a partition -- addresses the operand
        #  by the graph's own edge ids and says how many rows that is in `y_rows`)
        n_y = csr.y_rows or csr.num_edges
        if int(y.shape[0]) != n_y:
            raise ValueError("edge feature has %d rows, graph has %d edges" % (y.shape[0], n_y))
        x, y, tail = _bcast(x, y)
        dy = _prod(y.shape[1:])
    else:
        tail, dy = tuple(x.shape[1:]), 0
    dx, dout = _prod(x.shape[1:]), _prod(tail)
    if out is None:
        if accumulate:
            raise ValueError("accumulate=True needs an existing `out`")
        out = torch.empty((M,) + tuple(tail), dtype=x.dtype, device=x.device)
    else:
        if tuple(out.shape) != (M,) + tuple(tail) or out.dtype != x.dtype or not (out.is_contiguous() or ldo):
            raise ValueError("out must be a contiguous %s tensor of dtype %s" % ((M,) + tuple(tail), x.dtype))
    if M == 0 or dout == 0:
        return out
    if ldo and csr.num_edges == 0:
        if not accumulate:
            out.zero_()
        return out
    code = _code(x.dtype)
    entry, col32 = route.entry, csr.col32
    hub = hub_table(csr, x) if x2 is None and y is None and src_scale is None and not ldx and not ldo else None
    if hub is not None and reduce_op == "sum" and dst_scale is None and not accumulate:
        sp = slice_table(csr, x, hub, M, out)
        if sp is not None:
            return _aggregate_sliced(x, sp, out)
    ws = _scratch(_ws_hot, "aggregate", x, csr.num_edges, dout, code)
    if hub is not None:
        x2 = gather_rows(x, hub[0])                       # the hub rows of THIS call's features, contiguous
        entry, col32 = "aggregate_ext", hub[1]
    # the edge operand the kernel reads: y in original edge order (through eid32), or the edge-laid-out scale as a [E, 1] "mul" operand
    op, d_op, msg = (y, dy, message_op) if es is None else (es, 1, "mul")
    eid = _ptr(csr.eid32) if y is not None else None
    if entry == "aggregate_ext":
        _launch("aggregate_ext", x, _ptr(x), _ptr(x2), int(x.shape[0]), code, dx, ldx, _ptr(op), d_op, eid, _ptr(csr.row32), _ptr(col32),
                _ptr(csr.indptr), _ptr(zero_indptr), csr.max_row, csr.num_edges, csr.num_nodes, M, dout, ldo, MSG[msg],
                REDUCE[reduce_op], _ptr(dst_scale), int(accumulate), _ptr(out), _ptr(ws), ws.numel(), 1 if deal_chunks else 0)
    else:
        _launch("aggregate", x, _ptr(x), code, int(x.shape[0]), dx, _ptr(op), d_op, eid, _ptr(csr.row32), _ptr(csr.col32),
                _ptr(csr.indptr), csr.num_edges, csr.num_nodes, M, dout, MSG[msg], REDUCE[reduce_op], _ptr(src_scale),
                _ptr(dst_scale), int(accumulate), _ptr(out), _ptr(ws), ws.numel())
    return out


def aggregate_dense_supported(x, d_out):
    """Shapes pglamd_aggregate_dense covers: fp32 [N, 64 | 128] rows, d_out a multiple of 16 up to 1024."""
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and int(x.shape[1]) in (64, 128)
            and int(d_out) % 16 == 0 and 0 < int(d_out) <= 1024)


def aggregate_dense(x, csr, w, bias=None, act=None, reduce_op="sum", dst_scale=None, out_size=None, keep_agg=False, src_scale=None):
    """act( (dst_scale * REDUCE_{u->v} src_scale[u] * x[u]) @ w + bias ) in one kernel (pglamd_aggregate_dense; GCNConv's
    aggregate -> linear -> bias -> activation, pgl/nn/conv.py:242-254).  w: [d_in, d_out] row-major.  src_scale (one value per
    source node) travels as one value per edge position of the sorted stream, cached on the index (edge_scale).
    -> (out, agg or None)."""
    _need_cuda(x, w, bias, dst_scale, src_scale)
    es = None
    if src_scale is not None:
        if _EDGE_SCALE and not csr.edge_rows and src_scale.numel() == x.shape[0]:
            es = edge_scale(csr, src_scale.to(torch.float32))
        else:
            x = x * src_scale.reshape(-1, 1).to(x.dtype)
    # x in 8-byte lanes; a 16-byte aligned w keeps the form that stages it into LDS in 16-byte lanes
    x = _aligned(x, 8); w = _aligned(w, 16)
    d_in, d_out = int(x.shape[1]), int(w.shape[1])
    if int(w.shape[0]) != d_in or w.dtype != torch.float32 or not aggregate_dense_supported(x, d_out):
        raise ValueError("aggregate_dense: fp32 rows of 64 or 128 columns and a [d_in, d_out] fp32 weight with d_out %% 16 == 0 "
                         "(got x %s %s, w %s)" % (tuple(x.shape), x.dtype, tuple(w.shape)))
    if act not in (None, "relu"):
        raise ValueError("aggregate_dense: activation None or 'relu'")
    M = _rows_out(out_size, x.shape[0])
    out = torch.empty((M, d_out), dtype=torch.float32, device=x.device)
    agg = torch.empty((M, d_in), dtype=torch.float32, device=x.device) if keep_agg else None
    if M == 0:
        return out, agg
    ws = _scratch(_ws_hot, "aggregate_dense", x, csr.num_edges, d_in, d_out)
    b = None if bias is None else bias.to(torch.float32).contiguous()
    ds = None if dst_scale is None else dst_scale.to(torch.float32).contiguous()
    _launch("aggregate_dense", x, _ptr(x), d_in, _ptr(csr.row32), _ptr(csr.col32), _ptr(csr.indptr), csr.num_edges, csr.num_nodes, M,
            REDUCE[reduce_op], _ptr(es), _ptr(ds), _ptr(w), _ptr(b), 1 if act == "relu" else 0, d_out, _ptr(agg), _ptr(out), _ptr(ws),
            ws.numel())
    return out, agg


def _lane_aligned(d, *ts):
    """The two gradient kernels read rows of more than 64 (128) columns in 2- (4-) element lanes and turn away operands that are not
    aligned for them (PGLAMD_E_SHAPE).  Fresh allocations always are; a contiguous VIEW at an odd storage offset (m.flatten()[1:].view(n, d))
    is not.  (A non-contiguous operand is copied -- hence aligned -- before the launch.)"""
    vec = 4 if d > 128 else 2 if d > 64 else 1
    return all(t is None or not t.is_contiguous() or t.data_ptr() % (4 * vec) == 0 for t in ts)


def winner_grad_supported(x, out, grad=None):
    d = _prod(x.shape[1:])
    return (x.is_cuda and x.dtype == torch.float32 and out.dtype == torch.float32 and x.dim() >= 2 and 0 < d <= 256
            and tuple(x.shape[1:]) == tuple(out.shape[1:]) and (d <= 64 or d % 2 == 0) and (d <= 128 or d % 4 == 0)
            and _lane_aligned(d, x, out, grad))


def winner_grad(grad_out, out, x, csr_src):
    """d x of send_recv(x, max | min) in one walk of the src-sorted stream (pglamd_winner_grad): every message equal to its
    destination's winner receives that destination's gradient (Paddle's rule)."""
    _need_cuda(grad_out, out, x)
    grad_out = grad_out.contiguous(); out = out.contiguous(); x = x.contiguous()
    n, d = int(x.shape[0]), _prod(x.shape[1:])
    gx = torch.empty_like(x)
    if n == 0:
        return gx
    ws = _scratch(_ws_hot, "winner_grad", x, csr_src.num_edges, d)
    _launch("winner_grad", x, _ptr(grad_out), _ptr(out), _ptr(x), d, _ptr(csr_src.row32), _ptr(csr_src.col32), _ptr(csr_src.indptr),
            csr_src.num_edges, n, _ptr(gx), _ptr(ws), ws.numel())
    return gx


def edge_operand_grad_supported(grad, x, y_shape, reads_x=True):
    """Shapes pglamd_edge_operand_grad covers: fp32, trailing-dim broadcast of y onto x's tail, groups on power-of-two lane spans,
    operands aligned for the lanes the width asks for (reads_x=False -- add / sub -- x is not handed to the kernel: only its shape counts)."""
    if not (grad.is_cuda and grad.dtype == torch.float32 and x.dtype == torch.float32 and grad.dim() >= 2):
        return False
    tail = tuple(grad.shape[1:])
    if tuple(x.shape[1:]) != tail:
        return False
    d, dy = _prod(tail), _prod(y_shape[1:])
    if not (0 < d <= 256 and dy > 0 and d % dy == 0 and _trailing_ok(tuple(y_shape[1:]), tail)):
        return False
    vec = 4 if d > 128 else 2 if d > 64 else 1
    if d % vec or not _lane_aligned(d, grad, x if reads_x else None):
        return False
    g = d // dy
    if g >= vec:
        lanes = g // vec
        return g % vec == 0 and lanes <= 64 and (lanes & (lanes - 1)) == 0
    return vec % g == 0


def edge_operand_grad(grad, x, y, csr_dst, message_op, y_shape, dst_scale=None):
    """d y of send_ue_recv(x, y, message_op, sum | mean) -> [E, ...] of shape y_shape in ORIGINAL edge order."""
    _need_cuda(grad, x, y, dst_scale)
    grad = grad.contiguous(); x = x.contiguous()
    d, dy = _prod(grad.shape[1:]), _prod(y_shape[1:])
    E = csr_dst.num_edges
    gy = torch.empty(tuple(y_shape), dtype=torch.float32, device=grad.device)
    if E:
        yy = None if y is None else y.contiguous()
        ds = None if dst_scale is None else dst_scale.to(torch.float32).contiguous()
        # (add / sub never read x: not handing it over keeps its alignment out of the kernel's lane choice)
        xx = x if message_op in ("mul", "div") else None
        _launch("edge_operand_grad", grad, _ptr(grad), _ptr(xx), _ptr(yy), _ptr(ds), d, dy, _ptr(csr_dst.row32), _ptr(csr_dst.col32),
                _ptr(csr_dst.eid32), E, MSG[message_op], _ptr(gy))
    return gy


def profile_begin():
    """Start bracketing every flat-kernel launch with HIP events (bench.py roofline leg)."""
    _ffi.check(_ffi.lib().pglamd_profile_begin(), "profile_begin")


def profile_end():
    """-> (summed kernel milliseconds, number of launches) since profile_begin."""
    (ms, p_ms), (n, p_n) = _np_out_scalar(ctypes.c_double), _np_out_scalar(ctypes.c_int64)
    _ffi.check(_ffi.lib().pglamd_profile_end(p_ms, p_n), "profile_end")
    return ms.value, n.value


def profile_last_kernel():
    return _ffi.lib().pglamd_profile_last_kernel().decode()


def scatter_add_coo(x, src32, dst32, out_rows):
    """un-indexed fp32 atomic variant (K1'); order-nondeterministic."""
    _need_cuda(x, src32, dst32)
    x = x.contiguous()
    d = _prod(x.shape[1:])
    out = torch.empty((int(out_rows),) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
    _launch("scatter_add_coo", x, _ptr(x), d, _ptr(src32), _ptr(dst32), int(src32.shape[0]), int(out_rows), _ptr(out))
    return out


_COO_ONCE_MAX = int(os.environ.get("PGLAMD_COO_ONCE_ELEMENTS", str(6_400_000)))       # 50 k edges at d = 128 (profiles/r05/coo.txt)


def send_u_recv(x, src_index, dst_index, reduce_op="sum", out_size=None):
    """paddle.geometric.send_u_recv(x, src_index, dst_index, reduce_op, out_size) on RAW index arrays -- the call behind
    Graph.send_recv in the reference (pgl/graph.py:859-861), for an edge list that is used once and has no cached index.
    Dispatch rule (measured, profiles/r05/coo.txt): fp32 sum with |E| * d <= 6.4 M elements (50 k edges at d = 128) -> the edge-parallel atomic kernel
    (pglamd_scatter_add_coo: one launch, no sort; last bits depend on the atomics' order); everything else -> csr_build +
    the flat aggregation kernel (deterministic; 0.58 + 1.11 ms at |E| = 20 M, d = 128 where the atomic kernel takes 10 ms)."""
    _need_cuda(x, src_index, dst_index)
    n_out = _rows_out(out_size, x.shape[0])
    E = int(src_index.shape[0])
    d = _prod(x.shape[1:])
    if reduce_op == "sum" and x.dtype == torch.float32 and x.dim() >= 2 and 0 < E * d <= _COO_ONCE_MAX and n_out * d <= 8 * _COO_ONCE_MAX:
        s32 = src_index if src_index.dtype == torch.int32 else src_index.to(torch.int32)
        t32 = dst_index if dst_index.dtype == torch.int32 else dst_index.to(torch.int32)
        return scatter_add_coo(x, s32.contiguous(), t32.contiguous(), n_out)
    csr = csr_build(dst_index.to(torch.int64), src_index.to(torch.int64), max(n_out, int(x.shape[0])), want_i64=False)
    return aggregate(x, csr, reduce_op, n_out)


def send_uv(x, y, src32, dst32, message_op="add"):
    """paddle.geometric.send_uv (pgl/graph.py:964-966)."""
    _need_cuda(x, y, src32, dst32)
    if y.dtype != x.dtype:
        y = y.to(x.dtype)
    E = int(src32.shape[0])
    x, y, out_tail = _bcast(x, y)
    out = torch.empty((E,) + out_tail, dtype=x.dtype, device=x.device)
    dout = _prod(out_tail)
    if E and dout:
        _launch("send_uv", x, _ptr(x), _ptr(y), _code(x.dtype), _prod(x.shape[1:]), _prod(y.shape[1:]), dout, _ptr(src32), _ptr(dst32),
                E, MSG[message_op], _ptr(out))
    return out


# ------------------------------------------------------------------------------------------------
# segment ops
# ------------------------------------------------------------------------------------------------
def segment_reduce(data, segment_ids, pool_type="sum", num_segments=None):
    """paddle.geometric.segment_{sum,mean,max,min} (pgl/math.py:30-178).  ids sorted; out rows =
    ids[-1]+1 (read back from the device unless num_segments is supplied)."""
    _need_cuda(data, segment_ids)
    data = data.contiguous()
    segment_ids = segment_ids.contiguous()
    if segment_ids.dtype not in (torch.int32, torch.int64):
        raise TypeError("segment_ids must be int32 or int64")
    n = int(data.shape[0])
    if int(segment_ids.shape[0]) != n:
        raise ValueError("segment_ids length %d != data rows %d" % (segment_ids.shape[0], n))
    if num_segments is None:
        num_segments = int(segment_ids[-1].item()) + 1 if n else 0
    R, d = int(num_segments), _prod(data.shape[1:])
    out = torch.empty((R,) + tuple(data.shape[1:]), dtype=data.dtype, device=data.device)
    if R == 0 or d == 0:
        return out
    code = _code(data.dtype)
    ws = _scratch(_ws_hot, "segment_reduce", data, n, d, R, code)
    _launch("segment_reduce", data, _ptr(data), code, _ptr(segment_ids), int(segment_ids.dtype == torch.int64), n, d, R,
            REDUCE[pool_type], _ptr(out), _ptr(ws), ws.numel())
    return out


def seg_ptr_from_ids(segment_ids, num_segments):
    _need_cuda(segment_ids)
    segment_ids = segment_ids.contiguous()
    out = torch.empty(int(num_segments) + 1, dtype=torch.int64, device=segment_ids.device)
    _launch("seg_ptr_from_ids", segment_ids, _ptr(segment_ids), int(segment_ids.dtype == torch.int64), int(segment_ids.shape[0]),
            int(num_segments), _ptr(out))
    return out


class SegView(object):
    """Index view a segment softmax needs: seg_ptr [n_seg+1] int64, row32 (sorted-order segment ids),
    elem_seg32 (segment id of each data row in the data's own order), perm32 (sorted position ->
    data row, None when the data is already sorted)."""
    __slots__ = ("seg_ptr", "row32", "elem_seg32", "perm32")

    def __init__(self, seg_ptr, row32, elem_seg32, perm32=None):
        self.seg_ptr, self.row32, self.elem_seg32, self.perm32 = seg_ptr, row32, elem_seg32, perm32

    def as_csr(self, n_elem):
        """The segment reduction over the n_elem data rows as an index for aggregate: columns = perm32 (data rows)."""
        return CSR(self.seg_ptr, self.row32, self.perm32, self.perm32, int(self.seg_ptr.shape[0]) - 1, n_elem, edge_rows=True)


def segment_softmax(data, view):
    """pgl.math.segment_softmax (pgl/math.py:181-224); with view.perm32 = sorted_eid also the gather /
    scatter of GF.edge_softmax (pgl/nn/functional/graph_op.py:117-123): result in data's own order."""
    _need_cuda(data, view.seg_ptr, view.row32, view.elem_seg32, view.perm32)
    data = data.contiguous()
    out = torch.empty_like(data)
    n, d = int(data.shape[0]), _prod(data.shape[1:])
    n_seg = int(view.seg_ptr.shape[0]) - 1
    if n == 0 or d == 0 or n_seg == 0:
        return out
    code = _code(data.dtype)
    ws = _scratch(_ws_hot, "segment_softmax", data, n, d, n_seg, code)
    _launch("segment_softmax", data, _ptr(data), code, n, d, _ptr(view.row32), _ptr(view.perm32), _ptr(view.elem_seg32),
            _ptr(view.seg_ptr), n_seg, _ptr(out), _ptr(ws), ws.numel())
    return out


def gat_aggregate(feature, attn_src, attn_dst, csr, negative_slope=0.2, out_size=None, return_stats=False,
                  drop_p=0.0, seed=0):
    """Fused send_uv(add) -> leaky_relu -> edge_softmax(dst) -> dropout -> send_ue_recv(mul, sum) of GATConv
    (pgl/nn/conv.py:331-339) in one pass over the edges.  feature [N,H,D] fp32, attn_* [N,H]."""
    _need_cuda(feature, attn_src, attn_dst)
    if feature.dtype != torch.float32 or feature.dim() != 3:
        raise TypeError("gat_aggregate: feature must be float32 [N, heads, head_dim]")
    n, H, D = (int(v) for v in feature.shape)
    feature = _aligned(feature, _gat_lane_bytes(H, D))
    attn_src = attn_src.to(torch.float32).contiguous(); attn_dst = attn_dst.to(torch.float32).contiguous()
    if tuple(attn_src.shape) != (n, H) or attn_dst.shape[1] != H:
        raise ValueError("gat_aggregate: attn_src/attn_dst must be [N, heads]")
    M = _rows_out(out_size, n)
    out = torch.empty((M, H, D), dtype=torch.float32, device=feature.device)
    mx = sm = out_pos = s_pos = None
    if return_stats:
        mx = torch.empty((M, H), dtype=torch.float32, device=feature.device)
        sm = torch.empty((M, H), dtype=torch.float32, device=feature.device)
        if _GAT_POS_STATS:
            # positive-part statistics: what the backward needs to form d a_dst per node instead of per edge
            out_pos = torch.empty((M, H, D), dtype=torch.float32, device=feature.device)
            s_pos = torch.empty((M, H), dtype=torch.float32, device=feature.device)
    if M == 0:                                             # an empty share of a partitioned graph: nothing to launch
        return (out, mx, sm, out_pos, s_pos) if return_stats else out
    ws = _scratch(_ws_hot, "gat_aggregate", feature, csr.num_edges, H, D)
    _launch("gat_aggregate", feature, _ptr(feature), _ptr(attn_src), _ptr(attn_dst), H, D, float(negative_slope), float(drop_p),
            _seed32(seed), _ptr(csr.row32), _ptr(csr.col32), _ptr(csr.eid32), _ptr(csr.indptr), csr.num_edges, csr.num_nodes, M,
            _ptr(out), _ptr(mx), _ptr(sm), _ptr(out_pos), _ptr(s_pos), _ptr(ws), ws.numel())
    return (out, mx, sm, out_pos, s_pos) if return_stats else out


def gat_backward(grad_out, feature, out, attn_src, attn_dst, row_max, row_sum, csr_dst, csr_src, negative_slope=0.2,
                 drop_p=0.0, seed=0, out_pos=None, sum_pos=None):
    """Backward of gat_aggregate -> (grad_feature [N,H,D], grad_attn_src [N,H], grad_attn_dst [N,H])."""
    _need_cuda(grad_out, feature, out)
    n, H, D = (int(v) for v in feature.shape)
    # (grad_out and out also feed the pack kernel's 16-byte loads, as out_pos does; the per-(node, head) scalars are read one float at a time)
    grad_out = _aligned(grad_out, 16); out = _aligned(out, 16); out_pos = _aligned(out_pos, 16)
    feature = _aligned(feature, _gat_lane_bytes(H, D, pow2=True))
    gf = torch.empty_like(feature)
    g_src = torch.empty((n, H), dtype=torch.float32, device=feature.device)
    # d a_dst either from a second (dst-sorted) walk inside the library, or -- 1.3 ms faster at C3, 4*E*H bytes of
    # scratch -- as the segment sum by destination of the d pre_e the src-sorted walk can emit
    # (round 2) with the forward's positive-part statistics d a_dst is a per-node formula inside the library's pack kernel:
    # neither the edge buffer nor the second walk is needed
    use_pre = _GAT_BWD_EDGE_BUFFER and out_pos is None
    g_dst = None if use_pre else torch.empty((n, H), dtype=torch.float32, device=feature.device)
    gpre = torch.empty((csr_dst.num_edges, H), dtype=torch.float32, device=feature.device) if use_pre else None
    if n == 0:
        return gf, g_src, (g_dst if g_dst is not None else torch.empty((0, H), dtype=torch.float32, device=feature.device))
    ws = _scratch(_ws_hot, "gat_backward", feature, csr_dst.num_edges, n, H, D)
    _launch("gat_backward", feature, _ptr(grad_out), _ptr(feature), _ptr(attn_src), _ptr(attn_dst), _ptr(row_max), _ptr(row_sum),
            _ptr(out), H, D, float(negative_slope), float(drop_p), _seed32(seed), _ptr(csr_dst.row32), _ptr(csr_dst.col32),
            _ptr(csr_dst.eid32), _ptr(csr_dst.indptr), _ptr(csr_src.row32), _ptr(csr_src.col32), _ptr(csr_src.eid32),
            _ptr(csr_src.indptr), csr_dst.num_edges, n, _ptr(gf), _ptr(g_src), _ptr(g_dst), _ptr(gpre), _ptr(out_pos), _ptr(sum_pos),
            _ptr(ws), ws.numel())
    if use_pre:                 # rows of the src-sorted edge buffer gathered in dst-sorted order
        pos = _src_pos_in_dst_order(csr_dst, csr_src)
        g_dst = aggregate(gpre, csr_dst.view(col32=pos, eid32=pos, edge_rows=True), "sum", n)
    return gf, g_src, g_dst


def _src_pos_in_dst_order(csr_dst, csr_src):
    """perm[p] = position in the src-sorted stream of the edge at position p of the dst-sorted one (cached on csr_src)."""
    hit = csr_src._pos_by_dst
    if hit is not None and hit[0] is csr_dst:
        return hit[1]
    E, dev_ = csr_dst.num_edges, csr_dst.row32.device
    ar = torch.arange(E, dtype=torch.int32, device=dev_)
    if csr_src.eid32 is None:
        inv = ar
    else:
        inv = torch.empty(E, dtype=torch.int32, device=dev_)
        inv[csr_src.eid32.long()] = ar
    perm = inv if csr_dst.eid32 is None else inv[csr_dst.eid32.long()].contiguous()
    csr_src._pos_by_dst = (csr_dst, perm)
    return perm


def sddmm(x, y, csr):
    """out[e, h] = <x[src[e], h, :], y[dst[e], h, :]> in ORIGINAL edge order (csr = dst-sorted CSR).
    x, y: [N, H, D] fp32.  Returns [E, H]."""
    _need_cuda(x, y)
    if x.dtype != torch.float32 or y.dtype != torch.float32 or x.dim() != 3 or y.dim() != 3:
        raise TypeError("sddmm: float32 [N, heads, head_dim] operands")
    H, D = int(x.shape[1]), int(x.shape[2])
    lane = _gat_lane_bytes(H, D, pow2=True)
    x = _aligned(x, lane); y = _aligned(y, lane)
    out = torch.empty((csr.num_edges, H), dtype=torch.float32, device=x.device)
    if csr.num_edges:
        _launch("sddmm", x, _ptr(x), _ptr(y), H, D, _ptr(csr.row32), _ptr(csr.col32), _ptr(csr.eid32), csr.num_edges, _ptr(out))
    return out


def add_score(x, y, w, csr, negative_slope=0.2):
    """s[e, h] = sum_d w[h, d] * leaky_relu(x[src_e, h, d] + y[dst_e, h, d]) for the edges of the dst-sorted `csr`, in the
    order its eid32 defines (None: CSR order).  GATv2's attention score without the [E, H, D] tensors."""
    _need_cuda(x, y, w)
    H, D = int(x.shape[1]), int(x.shape[2])
    lane = _gat_lane_bytes(H, D, pow2=True)
    x = _aligned(x, lane); y = _aligned(y, lane); w = _aligned(w, lane)
    out = torch.empty((csr.num_edges, H), dtype=torch.float32, device=x.device)
    if csr.num_edges:
        _launch("add_score", x, _ptr(x), _ptr(y), _ptr(w), H, D, float(negative_slope), _ptr(csr.row32), _ptr(csr.col32),
                _ptr(csr.eid32), csr.num_edges, _ptr(out))
    return out


def add_score_backward(x_by_col, y_by_row, w, grad_score, csr, n_rows, negative_slope=0.2, want_w=False):
    """Gradient of add_score w.r.t. the operand of `csr`'s ROW nodes (and, if want_w, w): see include/pgl_amd.h."""
    _need_cuda(x_by_col, y_by_row, w, grad_score)
    H, D = int(x_by_col.shape[1]), int(x_by_col.shape[2])
    lane = _gat_lane_bytes(H, D)
    x_by_col = _aligned(x_by_col, lane); y_by_row = _aligned(y_by_row, lane); grad_score = grad_score.contiguous()
    w = _aligned(w, 16)                                        # (the entry point asks 16 bytes of w at every width)
    out = torch.empty((int(n_rows), H, D), dtype=torch.float32, device=x_by_col.device)
    wpart = None
    if want_w:
        wpart = torch.empty((max(int(_ffi.lib().pglamd_add_score_chunks(csr.num_edges)), 1), H * D), dtype=torch.float32, device=out.device)
        if csr.num_edges == 0:
            wpart.zero_()
    ws = _scratch(_ws_hot, "gat_aggregate", out, csr.num_edges, H, D)
    _launch("add_score_backward", out, _ptr(x_by_col), _ptr(y_by_row), _ptr(w), _ptr(grad_score), H, D, float(negative_slope),
            _ptr(csr.row32), _ptr(csr.col32), _ptr(csr.eid32), _ptr(csr.indptr), csr.num_edges, int(n_rows), _ptr(out), _ptr(wpart),
            _ptr(ws), ws.numel())
    return out, (wpart.sum(0) if want_w else None)


def sddmm_supported(H, D):
    vec = 4 if D % 4 == 0 else 2 if D % 2 == 0 else 1
    lph = D // vec
    return H * D <= 64 * vec and H <= 64 and (lph & (lph - 1)) == 0


def dot_attention_supported(H, D):
    """True when the fused dot-product attention kernels (csrc/dot_attention.hip) take heads x head_dim: sddmm's geometry -- one
    64-lane tile of 1, 2 or 4 floats per lane, every head on a power-of-two span of lanes."""
    return sddmm_supported(int(H), int(D))


def _dot_operands(what, *ts):
    q = ts[0]
    _need_cuda(*ts)
    if q.dim() != 3 or any(t.dtype != torch.float32 or tuple(t.shape) != tuple(q.shape) for t in ts):
        raise TypeError("%s: float32 [N, heads, head_dim] operands of one shape" % what)
    return (int(s) for s in q.shape)


def dot_attention(q, k, v, csr, scale=1.0, drop_p=0.0, seed=0, return_stats=False):
    """out[i, h] = sum_{e = (u -> i)} keep_e,h softmax_i(scale * <q[i, h], k[u, h]>) v[u, h] in one pass over the edges of the
    dst-sorted `csr` (pglamd_dot_attention, include/pgl_amd.h).  q, k, v: fp32 [N, H, D] -> [N, H, D], or with return_stats
    (out, row_max [N, H], row_sum [N, H]).  drop_p: attention dropout from (seed, original edge id, head), GAT's mask."""
    n, H, D = _dot_operands("dot_attention", q, k, v)
    if n != csr.num_nodes:
        raise ValueError("dot_attention: q, k, v hold %d rows, the index %d nodes (bipartite operands are not supported)" % (n, csr.num_nodes))
    lane = _gat_lane_bytes(H, D, pow2=True)
    q = _aligned(q, lane); k = _aligned(k, lane); v = _aligned(v, lane)
    out = torch.empty((n, H, D), dtype=torch.float32, device=q.device)
    mx = sm = None
    if return_stats:
        mx = torch.empty((n, H), dtype=torch.float32, device=q.device)
        sm = torch.empty((n, H), dtype=torch.float32, device=q.device)
    if n:
        ws = _scratch(_ws_hot, "dot_attention", q, csr.num_edges, H, D)
        _launch("dot_attention", q, _ptr(q), _ptr(k), _ptr(v), H, D, float(scale), float(drop_p), _seed32(seed), _ptr(csr.row32),
                _ptr(csr.col32), _ptr(csr.eid32), _ptr(csr.indptr), csr.num_edges, n, _ptr(out), _ptr(mx), _ptr(sm), _ptr(ws), ws.numel())
    return (out, mx, sm) if return_stats else out


def dot_attention_backward(grad_out, q, k, v, out, row_max, row_sum, csr_dst, csr_src, scale=1.0, drop_p=0.0, seed=0):
    """Backward of dot_attention -> (dq, dk, dv), each [N, H, D]: alpha recomputed per edge from (row_max, row_sum), one walk of
    the dst-sorted and one of the src-sorted index (pglamd_dot_attention_backward)."""
    n, H, D = _dot_operands("dot_attention_backward", q, k, v, grad_out, out)
    if n != csr_dst.num_nodes or n != csr_src.num_nodes:
        raise ValueError("dot_attention_backward: the operands hold %d rows, the indices %d / %d nodes" % (n, csr_dst.num_nodes, csr_src.num_nodes))
    lane = _gat_lane_bytes(H, D, pow2=True)
    q = _aligned(q, lane); k = _aligned(k, lane); v = _aligned(v, lane)
    # (grad_out and out also feed the pack kernel's 16-byte loads)
    grad_out = _aligned(grad_out, 16); out = _aligned(out, 16)
    row_max = row_max.contiguous(); row_sum = row_sum.contiguous()
    dq, dk, dv = (torch.empty((n, H, D), dtype=torch.float32, device=q.device) for _ in range(3))
    if n:
        ws = _scratch(_ws_hot, "dot_attention_backward", q, csr_dst.num_edges, n, H, D)
        _launch("dot_attention_backward", q, _ptr(grad_out), _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(row_max), _ptr(row_sum), H, D,
                float(scale), float(drop_p), _seed32(seed), _ptr(csr_dst.row32), _ptr(csr_dst.col32), _ptr(csr_dst.eid32),
                _ptr(csr_dst.indptr), _ptr(csr_src.row32), _ptr(csr_src.col32), _ptr(csr_src.eid32), _ptr(csr_src.indptr),
                csr_dst.num_edges, n, _ptr(dq), _ptr(dk), _ptr(dv), _ptr(ws), ws.numel())
    return dq, dk, dv


# ------------------------------------------------------------------------------------------------
# row moves, degree norm
# ------------------------------------------------------------------------------------------------
def gather_rows(x, index):
    """paddle.gather(x, index, axis=0) (pgl/utils/op.py:45, pgl/message.py:157, pgl/graph.py:822)."""
    _need_cuda(x, index)
    if index.dim() == 0:                       # a scalar id (paddle.to_tensor(5) is a one-element tensor in Paddle 2.4): one row
        index = index.reshape(1)
    x = x.contiguous(); index = index.contiguous()
    if index.dtype not in (torch.int32, torch.int64):
        raise TypeError("index must be int32 or int64")
    n, d = int(index.shape[0]), _prod(x.shape[1:])
    out = torch.empty((n,) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    if n and d:
        _launch("gather_rows", x, _ptr(x), d, x.element_size(), _ptr(index), int(index.dtype == torch.int64), n, _ptr(out))
    return out


def gather_rows_cast(x, index, out_dtype, out=None):
    """out[i] = cast(x[index[i]]) (index None: a row-wise conversion) -- pglamd_gather_rows_cast, the wire pack / unpack of the
    halo exchange.  fp32 <-> fp16 / bf16 (and fp32 -> fp32: a plain pack).  x may be a column block m[:, a:b] of a wider matrix."""
    _need_cuda(x, index)
    ldx = int(x.stride(0)) if _row_strided(x) else 0
    if not ldx:
        x = x.contiguous()
    n = int(x.shape[0]) if index is None else int(index.shape[0])
    if index is not None:
        index = index.contiguous()
        if index.dtype != torch.int32:
            index = index.to(torch.int32)
    d = _prod(x.shape[1:])
    if out is None:
        out = torch.empty((n,) + tuple(x.shape[1:]), dtype=out_dtype, device=x.device)
    elif tuple(out.shape) != (n,) + tuple(x.shape[1:]) or out.dtype != out_dtype or not out.is_contiguous():
        raise ValueError("gather_rows_cast: out must be a contiguous %s tensor of dtype %s" % ((n,) + tuple(x.shape[1:]), out_dtype))
    if n and d:
        _launch("gather_rows_cast", x, _ptr(x), _code(x.dtype), d, ldx, _ptr(index), n, _ptr(out), _code(out_dtype))
    return out


def scatter_rows(out, index, x):
    """paddle.scatter(out, index, x, overwrite=True) with unique indices, in place on `out`
    (pgl/graph.py:828-830)."""
    _need_cuda(out, index, x)
    x = x.contiguous(); index = index.contiguous()
    if not out.is_contiguous():
        raise ValueError("scatter_rows: destination must be contiguous")
    n, d = int(index.shape[0]), _prod(x.shape[1:])
    if n and d:
        _launch("scatter_rows", x, _ptr(x), d, x.element_size(), _ptr(index), int(index.dtype == torch.int64), n, _ptr(out))
    return out


def degree_norm(degree, dtype=torch.float32):
    """GF.degree_norm body (pgl/nn/functional/graph_op.py:51-54) -> [N, 1]."""
    _need_cuda(degree)
    degree = degree.contiguous()
    if dtype not in (torch.float32, torch.float64):
        raise TypeError("degree_norm: float32/float64 only")
    n = int(degree.shape[0])
    out = torch.empty((n, 1), dtype=dtype, device=degree.device)
    if n:
        _launch("degree_norm", degree, _ptr(degree), n, _ptr(out), int(dtype == torch.float64))
    return out


# ------------------------------------------------------------------------------------------------
# neighbour sampling + relabel (row f3)
# ------------------------------------------------------------------------------------------------
MAX_SAMPLE = 64          # kMaxSample of sampling.hip: Floyd's chosen set is a per-lane array of this many positions


def _ids_out_of_range(ids, hi=None):
    """One aminmax + one host read: does a non-empty int64 CUDA tensor hold an id < 0 (or >= hi)?"""
    lo, top = torch.stack(torch.aminmax(ids)).tolist()
    return lo < 0 or (hi is not None and top >= hi)


def sample_neighbors(csr, nodes, sample_size, seed=0, return_eids=False, check_range=True, weights=None):
    """paddle.geometric.sample_neighbors (pgl/sampling/sage.py:144-145) over the dst-sorted CSR:
    -> (neighbors [sum count], count [len(nodes)][, eids]).  Per node: the whole row in row order when sample_size < 0 or
    degree <= sample_size, else sample_size entries uniformly without replacement, a pure function of (seed, node id, draw
    number) (tests/sampling_defs.py: sample_restated).  sample_size <= MAX_SAMPLE, else ValueError before any launch.
    check_range: ValueError for a node id outside [0, num_nodes) before the first launch (one more host read on a path that
    reads its total back anyway); callers whose ids are in range by construction (later frontiers of NeighborSampler) pass
    False.
    weights: a WeightTable over this index (edge_weight_table / Graph.edge_weight_table(w, "dst")): per node the edges of
    positive weight -- all of them in row order when there are at most sample_size, else sample_size of them by successive
    sampling (each draw proportional to the weights of the edges not yet chosen; tests/weighted_defs.py: sample_weighted_restated).
    A zero-weight edge is never returned."""
    _need_cuda(nodes)
    sample_size = int(sample_size)
    if sample_size > MAX_SAMPLE:
        raise ValueError("pgl_amd sample_neighbors: sample_size %d exceeds kMaxSample = %d (pass -1 for all neighbours)"
                         % (sample_size, MAX_SAMPLE))
    nodes = nodes.to(torch.int64).contiguous()
    n, dev = int(nodes.shape[0]), nodes.device
    if check_range and n and _ids_out_of_range(nodes, csr.num_nodes):
        raise ValueError("pgl_amd sample_neighbors: node ids outside [0, num_nodes=%d)" % csr.num_nodes)
    count = torch.empty(n, dtype=torch.int64, device=dev)
    if weights is None:
        _launch("sample_neighbors_count", nodes, _ptr(csr.indptr), _ptr(nodes), n, sample_size, _ptr(count))
    else:
        _check_table(weights, csr, "sample_neighbors")
        _launch("sample_neighbors_weighted_count", nodes, _ptr(weights.npos), _ptr(nodes), n, sample_size, _ptr(count))
    offsets = exclusive_scan_i64(count)
    total = int((offsets[-1] + count[-1]).item()) if n else 0
    nbr = torch.empty(total, dtype=torch.int64, device=dev)
    eids = torch.empty(total, dtype=torch.int64, device=dev) if return_eids else None
    if total and weights is None:
        _launch("sample_neighbors_fill", nodes, _ptr(csr.indptr), _ptr(csr.col32), _ptr(csr.eid32), _ptr(nodes), n, sample_size,
                _seed64(seed), _ptr(offsets), _ptr(nbr), _ptr(eids))
    elif total:
        _launch("sample_neighbors_weighted_fill", nodes, _ptr(csr.indptr), _ptr(csr.col32), _ptr(csr.eid32), _ptr(weights.cum),
                _ptr(weights.npos), _ptr(nodes), n, sample_size, _seed64(seed), _ptr(offsets), _ptr(nbr), _ptr(eids))
    return (nbr, count, eids) if return_eids else (nbr, count)


# ------------------------------------------------------------------------------------------------
# edge-weighted sampling: the integer weight table (weighted.hip) and draws from it
# ------------------------------------------------------------------------------------------------
WeightTable = collections.namedtuple("WeightTable", ["cum", "npos"])
WeightTable.__doc__ = """What every weighted draw reads (include/pgl_amd.h, pglamd_edge_weight_table): cum int64 [E], the inclusive prefix sums
WITHIN each row of the integer weights q = max(1, floor(w / row maximum * 2^32)) (0 for a zero weight), and npos int64 [N], the
number of positive-weight positions of every row.  Tensors on the device (edge_weight_table) or numpy arrays (host_edge_weight_table)."""

_WEIGHT_FLAGS = ((1, "a NaN weight"), (2, "a negative weight"), (4, "an infinite weight"),
                 (8, "an edge id outside the weight vector (or a row outside the index)"))


def _raise_weight_flag(flag, what):
    if flag:
        raise ValueError("pgl_amd %s: edge weights must be finite and >= 0; found %s"
                         % (what, ", ".join(w for b, w in _WEIGHT_FLAGS if flag & b)))


def _check_table(table, csr, what):
    if not isinstance(table, WeightTable):
        raise TypeError("pgl_amd %s: weights must be a WeightTable (ops.edge_weight_table / Graph.edge_weight_table), got %s"
                        % (what, type(table).__name__))
    if int(table.cum.shape[0]) != csr.num_edges or int(table.npos.shape[0]) != csr.num_nodes:
        raise ValueError("pgl_amd %s: the WeightTable has %d positions / %d rows, the index %d / %d -- build it over the index "
                         "the call walks (dst index for sample_neighbors, successor index for walks)"
                         % (what, int(table.cum.shape[0]), int(table.npos.shape[0]), csr.num_edges, csr.num_nodes))


def _table_weight(weight):
    """A weight vector as the library reads it: 1-D contiguous fp32 or fp64 (fp16 / bf16 / integer weights are cast to fp32)."""
    if weight.dim() == 2 and weight.shape[1] == 1:
        weight = weight.reshape(-1)
    if weight.dim() != 1:
        raise ValueError("pgl_amd edge_weight_table: weights must be a vector ([E] or [E, 1]), got shape %s" % (tuple(weight.shape),))
    if weight.dtype not in (torch.float32, torch.float64):
        weight = weight.to(torch.float32)
    return weight.contiguous()


def _device_table(indptr, row32, eid, weight, N, E, what):
    _need_cuda(indptr, weight, eid)
    weight = _table_weight(weight)
    dev = weight.device
    if eid is None and int(weight.shape[0]) != E:
        raise ValueError("pgl_amd %s: %d weights for %d positions" % (what, int(weight.shape[0]), E))
    if eid is not None:
        if eid.dtype != torch.int32 or int(eid.shape[0]) != E:
            raise ValueError("pgl_amd %s: eid must be int32 [%d]" % (what, E))
        eid = eid.contiguous()
    cum = torch.empty(E, dtype=torch.int64, device=dev)
    npos = torch.empty(N, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    ws = _scratch(_ws, "edge_weight_table", weight, N, E)
    _launch("edge_weight_table", weight, _ptr(indptr), _ptr(row32), _ptr(eid), _ptr(weight), int(weight.dtype == torch.float64), N, E,
            int(weight.shape[0]), _ptr(cum), _ptr(npos), _ptr(flag), _ptr(ws), ws.numel(), what=what)
    _raise_weight_flag(int(flag.item()), what)
    return WeightTable(cum, npos)


def edge_weight_table(csr, weight, eid=None):
    """-> WeightTable(cum, npos) of `weight` over the index `csr` (pglamd_edge_weight_table): position j of the index reads
    weight[eid[j]] (eid int32 [E]; None: weight[j], i.e. the weights are already in the index's order -- NOT csr.eid32;
    Graph.edge_weight_table passes the permutation that takes original edge order to the index).  fp32 / fp64 weights are read as
    they are, other dtypes are cast to fp32.  One host read (the flag): ValueError for a NaN, negative or infinite weight.  Zero
    weights are legal (never drawn); a relative weight below 2^-32 of its row's maximum is rounded up to one quantum."""
    return _device_table(csr.indptr, csr.row32, eid, weight, csr.num_nodes, csr.num_edges, "edge_weight_table")


def weight_table(weight):
    """The single-row form: a WeightTable over a plain vector of n weights (indptr = [0, n]) -- what sample_from_table draws
    from.  cum int64 [n], npos int64 [1]."""
    _need_cuda(weight)
    n = int(weight.numel())
    indptr = torch.tensor([0, n], dtype=torch.int64, device=weight.device)
    return _device_table(indptr, None, None, weight.reshape(-1), 1, n, "weight_table")


def host_edge_weight_table(indptr, weight, eid=None):
    """Host twin of edge_weight_table (pglamd_edge_weight_table_host): numpy in, a WeightTable of numpy arrays out, the same
    bits.  indptr int64 [N+1]; weight [E_w] (float32 / float64 as they are, anything else cast to float32); eid int32 [E] or
    None."""
    indptr = _np_i64(indptr)
    weight = np.asarray(weight)
    if weight.ndim == 2 and weight.shape[1] == 1:
        weight = weight.reshape(-1)
    if weight.ndim != 1:
        raise ValueError("pgl_amd host_edge_weight_table: weights must be a vector, got shape %s" % (weight.shape,))
    weight = np.ascontiguousarray(weight, dtype=weight.dtype if weight.dtype in (np.float32, np.float64) else np.float32)
    N = int(indptr.shape[0]) - 1
    if N < 0:
        raise ValueError("pgl_amd host_edge_weight_table: indptr must have num_nodes + 1 entries")
    E = int(indptr[-1])
    if eid is None and weight.shape[0] != E:
        raise ValueError("pgl_amd host_edge_weight_table: %d weights for %d positions" % (weight.shape[0], E))
    if eid is not None:
        eid = np.ascontiguousarray(eid, dtype=np.int32)
        if eid.shape != (E,):
            raise ValueError("pgl_amd host_edge_weight_table: eid must be int32 [%d]" % E)
    cum, npos, flag = np.empty(E, np.int64), np.empty(N, np.int64), np.zeros(1, np.int32)
    _ffi.check(_ffi.lib().pglamd_edge_weight_table_host(_np_ptr(indptr), _np_ptr(eid), _np_ptr(weight), int(weight.dtype == np.float64),
                                                        N, E, int(weight.shape[0]), _np_ptr(cum), _np_ptr(npos), _np_ptr(flag)),
               "edge_weight_table_host")
    _raise_weight_flag(int(flag[0]), "host_edge_weight_table")
    return WeightTable(cum, npos)


def sample_from_table(cum_row, count, seed=0):
    """`count` independent draws WITH replacement from a single-row table (weight_table(w).cum, or a WeightTable of one row)
    -> int64 [count] indices, index j with probability q[j] / sum(q): draw i is the smallest j with
    cum_row[j] > scale64(mix64(seed ^ mix64(i)), cum_row[-1]) (tests/weighted_defs.py: sample_from_table_restated).  One launch,
    no host read; a table whose weights are all zero answers -1 for every draw."""
    if isinstance(cum_row, WeightTable):
        if int(cum_row.npos.shape[0]) != 1:
            raise ValueError("pgl_amd sample_from_table: a single-row table expected (ops.weight_table), got %d rows" % int(cum_row.npos.shape[0]))
        cum_row = cum_row.cum
    _need_cuda(cum_row)
    if cum_row.dtype != torch.int64 or cum_row.dim() != 1:
        raise TypeError("pgl_amd sample_from_table: cum_row must be the int64 [n] cum of a weight table")
    cum_row = cum_row.contiguous()
    n, count = int(cum_row.shape[0]), int(count)
    if count < 0 or (count > 0 and n == 0):
        raise ValueError("pgl_amd sample_from_table: count must be >= 0 and the table non-empty")
    out = torch.empty(count, dtype=torch.int64, device=cum_row.device)
    if count:
        _launch("sample_from_table", cum_row, _ptr(cum_row), n, count, _seed64(seed), _ptr(out))
    return out


def reindex_graph(nodes, neighbors, count, check_range=True):
    """paddle.geometric.reindex_graph (pgl/sampling/sage.py:146-147): -> (reindex_src, reindex_dst, out_nodes).
    out_nodes[:len(nodes)] == nodes AS GIVEN, repeated ids included (reindex_dst = repeat(arange(len(nodes)), count) and a
    sampler's "first len(nodes) rows are the destinations" rely on it); the neighbour ids that are no seed follow in order of
    first appearance; a neighbour equal to a seed is relabelled to that seed's FIRST position (tests/sampling_defs.py:
    reindex_restated).  Ids are >= 0 (-1 is the relabel table's empty marker): check_range reads the minima back and raises
    ValueError for a negative id; callers whose ids come from a graph index pass False and skip the read."""
    _need_cuda(nodes, neighbors, count)
    nodes = nodes.to(torch.int64).contiguous(); neighbors = neighbors.to(torch.int64).contiguous()
    if check_range and any(int(t.shape[0]) and _ids_out_of_range(t) for t in (nodes, neighbors)):
        raise ValueError("pgl_amd reindex_graph: negative ids (ids must be >= 0)")
    src, out_nodes = _relabel(nodes, neighbors)
    dst = torch.repeat_interleave(torch.arange(int(nodes.shape[0]), device=nodes.device), count)
    return src, dst, out_nodes


# ------------------------------------------------------------------------------------------------
# induced subgraph (S2; graph_kernel.pyx:394-432, pgl/sampling/custom.py:23-83)
# ------------------------------------------------------------------------------------------------
def induced_subgraph_launch_threads():
    """The largest number of lanes one launch of the induced-subgraph kernels starts (they stride beyond it)."""
    return int(_ffi.lib().pglamd_induced_subgraph_launch_threads())


def induced_subgraph(csr, nodes, check=True):
    """The edges of the dst-sorted index `csr` between the nodes of `nodes` (distinct ids inside [0, num_nodes), any order)
    -> (src_local, dst_local, eids), int64: for i, v in enumerate(nodes), for every position j of row v in CSR order whose
    source is selected, (position of col[j] in nodes, i, eid[j]) -- grouped by dst_local, non-decreasing; multi-edges and
    self-loops kept (tests/subgraph_defs.py: induced_restated).  eids in the order graph_kernel.extract_edges_from_nodes
    returns them.  One host read (kept edges + the flags of the id check) between the counting launches and the fill.
    check: ValueError for a repeated or out-of-range id (an out-of-range id is never dereferenced either way; check=False only
    skips the raise, for callers whose ids are distinct and in range by construction -- the result is undefined otherwise)."""
    _need_cuda(nodes, csr.indptr)
    if csr.col32 is None or csr.edge_rows:
        raise ValueError("pgl_amd induced_subgraph: needs an index over node rows (Graph.adj_dst_index.csr)")
    nodes = nodes.to(device=csr.indptr.device, dtype=torch.int64).reshape(-1).contiguous()
    n, dev = int(nodes.shape[0]), nodes.device
    N, E = int(csr.num_nodes), int(csr.num_edges)
    empty = lambda: tuple(torch.empty(0, dtype=torch.int64, device=dev) for _ in range(3))
    if n == 0:
        return empty()
    if n > N:
        raise ValueError("pgl_amd induced_subgraph: %d node ids for a graph of %d nodes (ids must be distinct)" % (n, N))
    status = torch.empty(4, dtype=torch.int64, device=dev)
    ws = _scratch(_ws, "induced_subgraph", nodes, N, n, E)
    _launch("induced_subgraph_count", nodes, _ptr(csr.indptr), _ptr(csr.col32), N, E, _ptr(nodes), n, _ptr(status), _ptr(ws), ws.numel())
    kept, flags, _, _ = status.tolist()
    if flags and check:
        raise ValueError("pgl_amd induced_subgraph: node ids %s" % " and ".join(
            w for b, w in ((1, "outside [0, num_nodes=%d)" % N), (2, "repeated (ids must be distinct)")) if flags & b))
    if flags or kept == 0:
        return empty()
    src, dst, eids = (torch.empty(kept, dtype=torch.int64, device=dev) for _ in range(3))
    _launch("induced_subgraph_fill", nodes, _ptr(csr.indptr), _ptr(csr.col32), _ptr(csr.eid32), N, E, _ptr(nodes), n, _ptr(src), _ptr(dst),
            _ptr(eids), _ptr(ws), ws.numel())
    return src, dst, eids


def host_induced_subgraph(indptr, col, eid, nodes, num_nodes=None):
    """Host twin of induced_subgraph (pglamd_induced_subgraph_host): numpy in, numpy out, the same three int64 arrays.
    eid None: the edge id of a position is the position.  ValueError for a repeated or out-of-range id."""
    indptr, col, nodes = _np_i64(indptr), _np_i64(col), _np_i64(nodes).reshape(-1)
    eid = _np_opt_i64(eid)
    N = int(indptr.shape[0]) - 1 if num_nodes is None else int(num_nodes)
    if N < 0 or indptr.shape[0] != N + 1 or (eid is not None and eid.shape[0] != col.shape[0]) or (N and int(indptr[-1]) != col.shape[0]):
        raise ValueError("host_induced_subgraph: indptr must have num_nodes + 1 entries and end at len(col) == len(eid)")
    n = int(nodes.shape[0])
    ok = nodes[(nodes >= 0) & (nodes < N)]
    cap = int((indptr[ok + 1] - indptr[ok]).sum()) if len(ok) == n else 0      # (a bad id is refused by the library below)
    src, dst, eids = (np.empty(cap, np.int64) for _ in range(3))
    num = np.zeros(1, np.int64)
    _ffi.check(_ffi.lib().pglamd_induced_subgraph_host(_np_ptr(indptr), _np_ptr(col), _np_ptr(eid), N, _np_ptr(nodes), n, _np_ptr(src),
                                                       _np_ptr(dst), _np_ptr(eids), _np_ptr(num)), "induced_subgraph_host")
    k = int(num[0])
    return src[:k].copy(), dst[:k].copy(), eids[:k].copy()


# ------------------------------------------------------------------------------------------------
# random walks + skip-gram pairs (pgl/sampling/walk.py:23-185, graph_kernel.pyx:140-224 / 341-364)
# ------------------------------------------------------------------------------------------------
WALK_UNIFORM, WALK_NODE2VEC, WALK_PLUS = 0, 1, 2


def walk_params(p=1.0, q=1.0, plus=False):
    """-> (mode, (thr_return, thr_in, thr_out)): the acceptance thresholds floor(2^32 * w / max(1/p, 1, 1/q)) of the node2vec
    weights 1/p (back to prev), 1 (a successor of prev / of the walk so far) and 1/q (otherwise), exact from the float values of
    p and q (so every caller -- device or host -- hands the library the same integers).  p == q == 1 is a uniform walk."""
    from fractions import Fraction
    p, q = float(p), float(q)
    if not (p > 0 and q > 0) or p == float("inf") or q == float("inf"):
        raise ValueError("random walk: p and q must be finite and > 0 (got p=%r, q=%r)" % (p, q))
    w = [1 / Fraction(p), Fraction(1), 1 / Fraction(q)]
    m = max(w)
    thr = tuple(max(1, int(x * (1 << 32) // m)) for x in w)
    if p == 1.0 and q == 1.0:
        return WALK_UNIFORM, thr
    return (WALK_PLUS if plus else WALK_NODE2VEC), thr


def default_max_trials(p=1.0, q=1.0):
    """Rejection trials per step before the exact scan when the caller names none: 32 * wmax / wmin (at least 64), so even at
    a node whose every candidate has the smallest weight the scan is reached with probability below (1 - 1/r)^(32 r) < e^-32.
    The scan keeps the law exact but reads a whole successor row per candidate test; on a hub (10^5 successors) one lane's scan
    stalls its wave for milliseconds, so it should stay a guarantee, not a path."""
    w = (1.0 / float(p), 1.0, 1.0 / float(q))
    return int(min((1 << 20) - 1, max(64, math.ceil(32.0 * max(w) / min(w)))))


def _walk_args(num_steps, max_trials, p=1.0, q=1.0):
    if max_trials is None:
        max_trials = default_max_trials(p, q)
    num_steps, max_trials = int(num_steps), int(max_trials)
    if num_steps < 0:
        raise ValueError("random walk: num_steps must be >= 0 (got %d)" % num_steps)
    if not 0 <= max_trials < (1 << 20):
        raise ValueError("random walk: max_trials must lie in [0, 2^20) (got %d)" % max_trials)
    return num_steps, max_trials


def _weighted_walk_mode(mode, what):
    if mode != WALK_UNIFORM:
        raise ValueError("pgl_amd %s: edge weights together with p != 1 or q != 1 (weighted node2vec) are not provided -- the exact "
                         "fallback scan would need 128-bit sums of weight x bias; pass p = q = 1 or no weights" % what)


def random_walk(csr, starts, num_steps, p=1.0, q=1.0, plus=False, seed=0, max_trials=None, check_range=True, weights=None):
    """Walks of num_steps steps from every start over a successor index whose rows are sorted by dst (Graph._csr_succ_sorted):
    -> (paths int64 [W, num_steps + 1], -1 after a dead end; lengths int64 [W]).  p == q == 1: uniform steps; else node2vec
    (plus=True: node2vec-plus, pgl/graph_kernel.pyx:180-224).  max_trials: rejection trials per step before one exact scan
    (0 = scan only; None = default_max_trials(p, q)).  One launch, no host sync unless check_range (then one read of the range
    flag: ValueError for a start outside [0, N)).
    weights: a WeightTable over THIS index (Graph.edge_weight_table(w, "succ")): every step picks a successor edge with
    probability proportional to its weight (one draw and one binary search of the row's prefix sums; a row whose weights are all
    zero is a dead end).  Only with p == q == 1."""
    _need_cuda(starts)
    starts = starts.to(torch.int64).contiguous()
    mode, thr = walk_params(p, q, plus)
    num_steps, max_trials = _walk_args(num_steps, max_trials, p, q)
    if weights is not None:
        _weighted_walk_mode(mode, "random_walk")
        _check_table(weights, csr, "random_walk")
    W, dev = int(starts.shape[0]), starts.device
    paths = torch.empty((W, num_steps + 1), dtype=torch.int64, device=dev)
    lengths = torch.empty(W, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev) if (check_range and W) else None
    if W and weights is not None:
        _launch("random_walk_weighted", starts, _ptr(csr.indptr), _ptr(csr.col32), _ptr(weights.cum), csr.num_nodes, _ptr(starts), W,
                num_steps, _seed64(seed), _ptr(paths), _ptr(lengths), _ptr(flag))
    elif W:
        _launch("random_walk", starts, _ptr(csr.indptr), _ptr(csr.col32), csr.num_nodes, _ptr(starts), W, num_steps, mode, thr[0], thr[1],
                thr[2], max_trials, _seed64(seed), _ptr(paths), _ptr(lengths), _ptr(flag))
    if flag is not None and int(flag.item()):
        raise ValueError("pgl_amd random_walk: start nodes outside [0, num_nodes=%d)" % csr.num_nodes)
    return paths, lengths


def skip_gram_pairs(paths, lengths, win_size=5, seed=0):
    """skip_gram_gen_pair (pgl/graph_kernel.pyx:341-364) over every walk of (paths, lengths) on the device -> (src, dst) int64:
    walk by walk, position by position, (walk[i], walk[j]) for j in [max(0, i - r), min(l - 1, i + r)] ascending with
    walk[j] != walk[i]; r in [1, win_size] is a hash of (seed, walk, i) (walk_core.hpp skip_gram_window).  One host sync (the
    pair total), as sample_neighbors."""
    _need_cuda(paths, lengths)
    paths = paths.to(torch.int64).contiguous(); lengths = lengths.to(torch.int64).contiguous()
    if paths.dim() != 2 or lengths.shape != (paths.shape[0],):
        raise ValueError("skip_gram_pairs: paths [W, L] and lengths [W] expected")
    if int(win_size) < 1:
        raise ValueError("skip_gram_pairs: win_size must be >= 1")
    W, width, dev = int(paths.shape[0]), int(paths.shape[1]), paths.device
    if W == 0 or width == 0:
        e = torch.empty(0, dtype=torch.int64, device=dev)
        return e, e.clone()
    count = torch.empty(W * width, dtype=torch.int64, device=dev)
    _launch("skip_gram_count", paths, _ptr(paths), _ptr(lengths), W, width, int(win_size), _seed64(seed), _ptr(count))
    offsets = exclusive_scan_i64(count)
    total = int((offsets[-1] + count[-1]).item())
    src = torch.empty(total, dtype=torch.int64, device=dev)
    dst = torch.empty(total, dtype=torch.int64, device=dev)
    if total:
        _launch("skip_gram_fill", paths, _ptr(paths), _ptr(lengths), W, width, int(win_size), _seed64(seed), _ptr(offsets), _ptr(src),
                _ptr(dst))
    return src, dst


# ------------------------------------------------------------------------------------------------
# metapath walks over the relations of a HeterGraph (walk.hip: pglamd_metapath_walk)
# ------------------------------------------------------------------------------------------------
StackedRelations = collections.namedtuple("StackedRelations", ["indptr", "col", "num_nodes", "edge_base"])
StackedRelations.__doc__ = """The relation-stacked successor index a metapath walk reads (include/pgl_amd.h, pglamd_metapath_walk): indptr
int64 [R, N + 1], row r = relation r's sorted successor indptr plus edge_base[r], so its entries are absolute positions of col;
col int32 [sum E_r], the relations' col32 concatenated (every row still ascending); edge_base: R + 1 Python ints, relation r owns
col[edge_base[r] : edge_base[r + 1]].  Tensors on the device (stack_relations) or numpy arrays (host_stack_relations)."""
StackedRelations.num_relations = property(lambda self: len(self.edge_base) - 1)
# ------------------------------------------------------------------------------------------------
# negative sampling checked against the graph (negative.hip)
# ------------------------------------------------------------------------------------------------
NEG_MAX_TRIALS = 16      # rejection trials per draw before the exact fallback when the caller names none
NEG_RANGE, NEG_EMPTY = 1, 2        # PGLAMD_NEG_RANGE / PGLAMD_NEG_EMPTY


def _negative_args(num_nodes, num_neg, lo, hi, noise, max_trials, what):
    """-> (num_neg, lo, hi, max_trials) as the library wants them; ValueError / TypeError before any launch for what it would
    refuse."""
    num_neg, lo = int(num_neg), int(lo)
    max_trials = NEG_MAX_TRIALS if max_trials is None else int(max_trials)
    if num_neg < 1:
        raise ValueError("pgl_amd %s: num_neg must be >= 1 (got %d)" % (what, num_neg))
    if not 0 <= max_trials < (1 << 20):
        raise ValueError("pgl_amd %s: max_trials must lie in [0, 2^20) (got %d)" % (what, max_trials))
    if noise is not None:
        if not isinstance(noise, WeightTable) or int(noise.npos.shape[0]) != 1:
            raise TypeError("pgl_amd %s: noise must be a single-row WeightTable (ops.weight_table)" % what)
        n_table = int(noise.cum.shape[0])
        if lo != 0 or (hi is not None and int(hi) != n_table):
            raise ValueError("pgl_amd %s: weighted noise over a sub-range is not provided -- with noise, lo must be 0 and hi the "
                             "table's length %d (got lo=%d, hi=%r)" % (what, n_table, lo, hi))
        hi = n_table
    hi = int(num_nodes) if hi is None else int(hi)
    if not 0 <= lo < hi <= num_nodes:
        raise ValueError("pgl_amd %s: the candidate range [lo=%d, hi=%d) must be non-empty and lie inside [0, num_nodes=%d]"
                         % (what, lo, hi, num_nodes))
    return num_neg, lo, hi, max_trials


def _raise_negative_flags(flag, num_nodes, allow_empty, what):
    if flag & NEG_RANGE:
        raise ValueError("pgl_amd %s: sources outside [0, num_nodes=%d)" % (what, num_nodes))
    if flag & NEG_EMPTY and not allow_empty:
        raise ValueError("pgl_amd %s: a source whose successors (and itself, with exclude_self) cover the whole candidate range, or "
                         "all of the noise weight, has no negative; pass allow_empty=True to get -1 there" % what)


def sample_negatives(csr, src, num_neg, seed=0, lo=0, hi=None, noise=None, exclude_self=False, max_trials=None, return_pos=False,
                     check=True, allow_empty=False):
    """Negatives checked against the graph (pglamd_sample_negatives; the per-user `while True: randint` loop of
    examples/lightgcn/utils.py UniformSample_original_python): for every source of `src` num_neg ids of [lo, hi) (hi=None: all
    nodes) that are NOT successors of it in `csr`, a successor index whose rows are sorted by dst (Graph._csr_succ_sorted; the
    predecessor index Graph._csr_pred_sorted corrupts heads instead) -> neg int64 [n, num_neg], or (neg, pos) with return_pos:
    pos int64 [n], one uniform successor per source (a multi-edge counts twice), -1 for a source without successors.
    exclude_self: the source itself is no candidate either.  noise: a single-row WeightTable (ops.weight_table(w), w over the ids
    0 .. hi-1) -- candidates are drawn proportionally to w instead of uniformly; a zero-weight id is never returned.  Up to
    max_trials (None: NEG_MAX_TRIALS) rejection trials per draw, then one exact draw from the complement, so the law is exact
    and the call always ends; the draws are a pure function of (seed, POSITION in src, k) (tests/negative_defs.py restates them).
    One launch.  check=True reads the flags once: ValueError for a source outside [0, num_nodes), and for a source with no
    negative at all unless allow_empty (its row is then -1).  check=False makes no host read: such rows are -1."""
    _need_cuda(src)
    src = src.to(torch.int64).reshape(-1).contiguous()
    num_neg, lo, hi, max_trials = _negative_args(csr.num_nodes, num_neg, lo, hi, noise, max_trials, "sample_negatives")
    if noise is not None:
        _need_cuda(noise.cum)
    n, dev = int(src.shape[0]), src.device
    neg = torch.empty((n, num_neg), dtype=torch.int64, device=dev)
    pos = torch.empty(n, dtype=torch.int64, device=dev) if return_pos else None
    flags = torch.zeros(1, dtype=torch.int32, device=dev) if (check and n) else None
    if n:
        _launch("sample_negatives", src, _ptr(csr.indptr), _ptr(csr.col32), csr.num_nodes, _ptr(None if noise is None else noise.cum), lo, hi,
                _ptr(src), n, num_neg, int(bool(exclude_self)), max_trials, _seed64(seed), _ptr(neg), _ptr(pos), _ptr(flags))
    if flags is not None:
        _raise_negative_flags(int(flags.item()), csr.num_nodes, allow_empty, "sample_negatives")
    return (neg, pos) if return_pos else neg


MAX_METAPATH = 64        # walk::kMaxMetapath


def _edge_base(num_edges):
    base = [0]
    for e in num_edges:
        base.append(base[-1] + int(e))
    return tuple(base)


def stack_relations(csrs):
    """-> StackedRelations of R >= 1 sorted successor indices (Graph._csr_succ_sorted() of every relation of a HeterGraph, in the
    order their relation numbers name) over one node set.  Device tensors in, device tensors out, no host read."""
    csrs = list(csrs)
    if not csrs:
        raise ValueError("pgl_amd stack_relations: at least one relation expected")
    N = csrs[0].num_nodes
    if any(c.num_nodes != N for c in csrs):
        raise ValueError("pgl_amd stack_relations: the relations must share one node set (got %s nodes)" % [c.num_nodes for c in csrs])
    _need_cuda(*[c.indptr for c in csrs])
    base = _edge_base(c.num_edges for c in csrs)
    indptr = torch.stack([c.indptr + b for c, b in zip(csrs, base)]).contiguous()
    col = torch.cat([c.col32 for c in csrs]).contiguous()
    return StackedRelations(indptr, col, N, base)


def host_stack_relations(indices):
    """The numpy twin of stack_relations: `indices` = [(indptr int64 [N+1], col [E_r])] (a numpy graph's _csr_succ_sorted())."""
    indices = [(_np_i64(p).reshape(-1), np.ascontiguousarray(c, dtype=np.int32).reshape(-1)) for p, c in indices]
    if not indices:
        raise ValueError("pgl_amd host_stack_relations: at least one relation expected")
    N = int(indices[0][0].shape[0]) - 1
    if N < 0 or any(int(p.shape[0]) != N + 1 for p, _ in indices):
        raise ValueError("pgl_amd host_stack_relations: the relations must share one node set")
    base = _edge_base(c.shape[0] for _, c in indices)
    indptr = np.ascontiguousarray(np.stack([p + b for (p, _), b in zip(indices, base)]))
    return StackedRelations(indptr, np.concatenate([c for _, c in indices]), N, base)


def stack_weight_tables(tables):
    """The WeightTable of a stacked index from the relations' own tables over their sorted successor indices
    (Graph.edge_weight_table(w, "succ")), in the stack's order: cum and npos concatenated -- the prefix sums are sums WITHIN a row,
    so nothing is rebased.  Device tensors or numpy arrays, as given."""
    tables = list(tables)
    cat = torch.cat if isinstance(tables[0].cum, torch.Tensor) else np.concatenate
    return WeightTable(cat([t.cum for t in tables]), cat([t.npos for t in tables]))


def _check_stacked_table(table, stacked, what):
    if not isinstance(table, WeightTable):
        raise TypeError("pgl_amd %s: weights must be a WeightTable over the stacked index (ops.stack_weight_tables), got %s"
                        % (what, type(table).__name__))
    E, rows = stacked.edge_base[-1], stacked.num_relations * stacked.num_nodes
    if int(table.cum.shape[0]) != E or int(table.npos.shape[0]) != rows:
        raise ValueError("pgl_amd %s: the WeightTable has %d positions / %d rows, the stacked index %d / %d -- concatenate the "
                         "relations' successor tables in the stack's order (ops.stack_weight_tables)"
                         % (what, int(table.cum.shape[0]), int(table.npos.shape[0]), E, rows))


def _metapath_array(metapath):
    return np.ascontiguousarray(np.asarray(list(metapath), dtype=np.int64).reshape(-1).astype(np.int32))


def metapath_walk(stacked, starts, metapath, num_steps, phase=0, seed=0, weights=None, check_range=True):
    """metapath_randomwalk (examples/metapath2vec/datasets/sampling.py:285-340) for every walker in one launch: walks of num_steps
    steps over a StackedRelations index, the step from position t drawn from the successors under relation
    metapath[(phase + t) % len(metapath)] (`metapath`: a sequence of 1 .. MAX_METAPATH relation numbers of the stack)
    -> (paths int64 [W, num_steps + 1], -1 after a dead end; lengths int64 [W]).  A node without successors under the step's
    relation ends the walk.  Uniform steps, or with weights (a WeightTable over the stacked index: stack_weight_tables) by edge
    weight; the draws are random_walk's, so a one-relation metapath returns what random_walk returns over that relation with
    the same seed.  No host sync unless check_range (then one read of the range flag: ValueError for a start outside [0, N));
    a bad metapath, phase or num_steps is the library's PGLAMD_E_ARG (ValueError)."""
    _need_cuda(starts, stacked.indptr, stacked.col)
    starts = starts.to(torch.int64).reshape(-1).contiguous()
    mp, num_steps = _metapath_array(metapath), int(num_steps)
    if weights is not None:
        _check_stacked_table(weights, stacked, "metapath_walk")
        _need_cuda(weights.cum)
    W, dev = int(starts.shape[0]), starts.device
    paths = torch.empty((W, max(num_steps, 0) + 1), dtype=torch.int64, device=dev)
    lengths = torch.empty(W, dtype=torch.int64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev) if (check_range and W) else None
    _launch("metapath_walk", starts, _ptr(stacked.indptr), _ptr(stacked.col), _ptr(None if weights is None else weights.cum),
            stacked.num_nodes, stacked.num_relations, _np_ptr(mp), int(mp.shape[0]), int(phase), _ptr(starts), W, num_steps,
            _seed64(seed), _ptr(paths), _ptr(lengths), _ptr(flag))
    if flag is not None and int(flag.item()):
        raise ValueError("pgl_amd metapath_walk: start nodes outside [0, num_nodes=%d)" % stacked.num_nodes)
    return paths, lengths


def host_metapath_walk(stacked, starts, metapath, num_steps, phase=0, seed=0, weights=None, check_range=True, threads=0):
    """The host twin of metapath_walk (pglamd_metapath_walk_host: same step logic, same RNG, bit-identical result, independent of
    `threads`; <= 0: up to 16) over a StackedRelations of numpy arrays (host_stack_relations); weights: a WeightTable of numpy
    arrays over the stacked index."""
    indptr = _np_i64(stacked.indptr); col = np.ascontiguousarray(stacked.col, dtype=np.int32); starts = _np_i64(starts).reshape(-1)
    mp, num_steps = _metapath_array(metapath), int(num_steps)
    cum = None
    if weights is not None:
        _check_stacked_table(weights, stacked, "host_metapath_walk")
        cum = _np_i64(weights.cum)
    W = int(starts.shape[0])
    paths = np.empty((W, max(num_steps, 0) + 1), np.int64)
    lengths = np.empty(W, np.int64)
    flag = np.zeros(1, np.int32)
    _ffi.check(_ffi.lib().pglamd_metapath_walk_host(_np_ptr(indptr), _np_ptr(col), _np_ptr(cum), stacked.num_nodes, stacked.num_relations,
                                                    _np_ptr(mp), int(mp.shape[0]), int(phase), _np_ptr(starts), W, num_steps,
                                                    _seed64(seed), int(threads), _np_ptr(paths), _np_ptr(lengths), _np_ptr(flag)),
               "metapath_walk_host")
    if check_range and int(flag[0]):
        raise ValueError("pgl_amd metapath_walk: start nodes outside [0, num_nodes=%d)" % stacked.num_nodes)
    return paths, lengths


# ------------------------------------------------------------------------------------------------
# relation-wise neighbour sampling over the relations of a HeterGraph (sampling_rel.hip: pglamd_sample_relations_count / _fill)
# ------------------------------------------------------------------------------------------------
class StackedIndex(collections.namedtuple("StackedIndex", ["indptr", "col", "eid", "num_nodes", "edge_base"])):
    # (no __slots__: what aggregate_relations learns about an index -- max_segment, the long-row lists, the mean scales -- is kept
    #  on the instance; the five fields stay the tuple's)
    pass


StackedIndex.__doc__ = """The relation-stacked PREDECESSOR index the relation-wise sampler reads (include/pgl_amd.h, pglamd_sample_relations_count):
indptr int64 [R, N + 1], row r = relation r's dst-sorted indptr plus edge_base[r], so its entries are absolute positions of col and
eid; col int32 [sum E_r], the sources by position, the relations concatenated; eid int32 [sum E_r], the relation-LOCAL original edge
ids by position, concatenated; edge_base: R + 1 Python ints, relation r owns positions [edge_base[r], edge_base[r + 1]).  Tensors on
the device (stack_indices) or numpy arrays (host_stack_indices).  (StackedRelations is the walks' index: sorted by source, no edge ids.)"""
StackedIndex.num_relations = property(lambda self: len(self.edge_base) - 1)
MAX_RELATIONS = 64       # PGLAMD_SAMPLE_MAX_RELATIONS: the fan-outs travel in the kernel's argument block

RelationSample = collections.namedtuple("RelationSample", ["neighbors", "dst", "count", "edge_split", "eids"])
RelationSample.__doc__ = """What sample_neighbors_relations returns.  neighbors / dst / eids int64 [T]: relation-major, then seed position, then
draw order -- the sampled source, the seed POSITION of the slot, the relation-local edge id (eids None unless asked for);
count int64 [R, n]; edge_split: R + 1 Python ints, relation r owns [edge_split[r], edge_split[r + 1])."""

_U64 = 0xFFFFFFFFFFFFFFFF


def _mix64(z):
    """mix64 of csrc/sample_core.hpp (the splitmix64 finaliser) on a Python int, modulo 2^64."""
    z = (z + 0x9E3779B97F4A7C15) & _U64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _U64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _U64
    return z ^ (z >> 31)


def relation_seed(seed, r):
    """The seed relation r of a stacked index samples with: mix64(uint64(seed) ^ mix64(uint64(r))) (sample_core.hpp).  Relation r of
    sample_neighbors_relations(.., seed) holds what sample_neighbors returns over that relation with seed=relation_seed(seed, r)."""
    return _mix64(_seed64(seed) ^ _mix64(int(r) & _U64))


def stack_indices(csrs):
    """-> StackedIndex of R >= 1 dst-sorted indices (Graph.adj_dst_index.csr of every relation of a HeterGraph, in the order their
    relation numbers name) over one node set.  Device tensors in, device tensors out, no host read."""
    csrs = list(csrs)
    if not csrs:
        raise ValueError("pgl_amd stack_indices: at least one relation expected")
    N = csrs[0].num_nodes
    if any(c.num_nodes != N for c in csrs):
        raise ValueError("pgl_amd stack_indices: the relations must share one node set (got %s nodes)" % [c.num_nodes for c in csrs])
    _need_cuda(*[c.indptr for c in csrs])
    base = _edge_base(c.num_edges for c in csrs)
    indptr = torch.stack([c.indptr + b for c, b in zip(csrs, base)]).contiguous()
    col = torch.cat([c.col32 for c in csrs]).contiguous()
    eid = torch.cat([c.eid32 if c.eid32 is not None else torch.arange(c.num_edges, dtype=torch.int32, device=c.indptr.device)
                     for c in csrs]).contiguous()
    return StackedIndex(indptr, col, eid, N, base)


def host_stack_indices(indices):
    """The numpy twin of stack_indices: `indices` = [(indptr int64 [N+1], col [E_r], eid [E_r])], the dst-sorted index of every
    relation (a numpy graph's adj_dst_index: _indptr, _sorted_v, _sorted_eid)."""
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32).reshape(-1)
    indices = [(_np_i64(p).reshape(-1), i32(c), i32(e)) for p, c, e in indices]
    if not indices:
        raise ValueError("pgl_amd host_stack_indices: at least one relation expected")
    N = int(indices[0][0].shape[0]) - 1
    if N < 0 or any(int(p.shape[0]) != N + 1 for p, _, _ in indices):
        raise ValueError("pgl_amd host_stack_indices: the relations must share one node set")
    base = _edge_base(c.shape[0] for _, c, _ in indices)
    indptr = np.ascontiguousarray(np.stack([p + b for (p, _, _), b in zip(indices, base)]))
    return StackedIndex(indptr, np.concatenate([c for _, c, _ in indices]), np.concatenate([e for _, _, e in indices]), N, base)


def _fanout_array(fanouts, stacked, what):
    """The fan-outs as the library reads them (int64 [R], host); ValueError for a wrong length or a fan-out above MAX_SAMPLE."""
    fan = np.ascontiguousarray(np.asarray(list(fanouts), dtype=np.int64).reshape(-1))
    R = stacked.num_relations
    if R > MAX_RELATIONS:
        raise ValueError("pgl_amd %s: %d relations exceed MAX_RELATIONS = %d" % (what, R, MAX_RELATIONS))
    if int(fan.shape[0]) != R:
        raise ValueError("pgl_amd %s: %d fan-outs for %d relations" % (what, int(fan.shape[0]), R))
    if R and int(fan.max()) > MAX_SAMPLE:
        raise ValueError("pgl_amd %s: fan-out %d exceeds kMaxSample = %d (pass -1 for all neighbours)" % (what, int(fan.max()), MAX_SAMPLE))
    return fan


def _sample_relations(stacked, nodes, fanouts, seed, return_eids, check_range):
    """sample_neighbors_relations plus what the block builder goes on with: -> (RelationSample, offsets int64 [R * n] or None when
    n == 0: the exclusive scan of count, bounds int64 [R + 1] on the device or None: edge_split before the host read)."""
    _need_cuda(nodes, stacked.indptr, stacked.col, stacked.eid)
    fan = _fanout_array(fanouts, stacked, "sample_neighbors_relations")
    R, N = stacked.num_relations, stacked.num_nodes
    nodes = nodes.to(torch.int64).reshape(-1).contiguous()
    n, dev = int(nodes.shape[0]), nodes.device
    if check_range and n and _ids_out_of_range(nodes, N):
        raise ValueError("pgl_amd sample_neighbors_relations: node ids outside [0, num_nodes=%d)" % N)
    i64 = dict(dtype=torch.int64, device=dev)
    count = torch.empty((R, n), **i64)
    if n == 0:
        e = torch.empty(0, **i64)
        return RelationSample(e, e.clone(), count, (0,) * (R + 1), e.clone() if return_eids else None), None, None
    _launch("sample_relations_count", nodes, _ptr(stacked.indptr), N, R, _np_ptr(fan), _ptr(nodes), n, _ptr(count))
    flat = count.view(-1)
    offsets = exclusive_scan_i64(flat)
    # the one host read: the scan's values at the relation boundaries plus the total
    bounds = torch.cat([offsets.view(R, n)[:, 0], offsets[-1:] + flat[-1:]])
    split = tuple(bounds.tolist())
    total = split[-1]
    nbr, dst = torch.empty(total, **i64), torch.empty(total, **i64)
    eids = torch.empty(total, **i64) if return_eids else None
    if total:
        _launch("sample_relations_fill", nodes, _ptr(stacked.indptr), _ptr(stacked.col), _ptr(stacked.eid), N, R, _np_ptr(fan), _ptr(nodes),
                n, _seed64(seed), _ptr(offsets), _ptr(nbr), _ptr(dst), _ptr(eids))
    return RelationSample(nbr, dst, count, split, eids), offsets, bounds


def sample_neighbors_relations(stacked, nodes, fanouts, seed=0, return_eids=False, check_range=True):
    """The per-edge-type sample_neighbors loop of a relational mini-batch (examples/NeurIPS2022-OGB-Challenge/MAG240M/dataset/
    new_dataset_p2p.py:163-193) for every relation in one count launch, one scan and one fill launch over a StackedIndex
    -> RelationSample(neighbors, dst, count, edge_split, eids).  Relation r, seed position i: exactly what
    sample_neighbors(csr_r, nodes, fanouts[r], seed=relation_seed(seed, r)) returns for position i -- the same Floyd draws in the same
    order, the whole row when fanouts[r] < 0 or degree <= fanouts[r]; fanouts[r] == 0 samples nothing from relation r
    (tests/relation_sampling_defs.py: sample_relations_restated).  `dst` is written by the fill kernel (no repeat_interleave).
    One host read of R + 1 numbers (edge_split).  ValueError before any launch for a fan-out above MAX_SAMPLE, len(fanouts) != R,
    more than MAX_RELATIONS relations or (check_range) a node id outside [0, num_nodes).  Edge weights are not supported here."""
    return _sample_relations(stacked, nodes, fanouts, seed, return_eids, check_range)[0]


def host_sample_neighbors_relations(stacked, nodes, fanouts, seed=0, return_eids=False, check_range=True, threads=0):
    """The host twin of sample_neighbors_relations (pglamd_sample_relations_host: the same draws, bit-identical arrays, independent
    of `threads`; <= 0: up to 16) over a StackedIndex of numpy arrays (host_stack_indices).  The node range is always checked."""
    fan = _fanout_array(fanouts, stacked, "host_sample_neighbors_relations")
    R, N = stacked.num_relations, stacked.num_nodes
    indptr = _np_i64(stacked.indptr); col = np.ascontiguousarray(stacked.col, dtype=np.int32); eid = np.ascontiguousarray(stacked.eid, dtype=np.int32)
    nodes = _np_i64(nodes).reshape(-1)
    n = int(nodes.shape[0])
    if n and (int(nodes.min()) < 0 or int(nodes.max()) >= N):
        raise ValueError("pgl_amd sample_neighbors_relations: node ids outside [0, num_nodes=%d)" % N)
    count = np.empty((R, n), np.int64)
    split = np.zeros(R + 1, np.int64)
    nbr = dst = eids = None

    def call(num_out):
        _ffi.check(_ffi.lib().pglamd_sample_relations_host(_np_ptr(indptr), _np_ptr(col), _np_ptr(eid), N, R, _np_ptr(fan), _np_ptr(nodes), n,
                                                           _seed64(seed), int(threads), _np_ptr(count), _np_ptr(split), _np_ptr(nbr),
                                                           _np_ptr(dst), _np_ptr(eids), num_out), "sample_relations_host")
    call(0)                                                     # the counting pass sizes the outputs
    total = int(split[-1])
    nbr, dst = np.empty(total, np.int64), np.empty(total, np.int64)
    eids = np.empty(total, np.int64) if return_eids else None
    if total:
        call(total)
    return RelationSample(nbr, dst, count, tuple(int(s) for s in split), eids)


def _relabel(nodes, neighbors):
    """pglamd_reindex: -> (reindex_src int64 [m], out_nodes) with reindex_graph's contract (out_nodes[:n] == nodes as given, new ids
    in order of first appearance, a neighbour equal to a seed maps to that seed's first position).  One host read: len(out_nodes)."""
    n, m, dev = int(nodes.shape[0]), int(neighbors.shape[0]), nodes.device
    src = torch.empty(m, dtype=torch.int64, device=dev)
    out_nodes = torch.empty(n + m, dtype=torch.int64, device=dev)
    num = torch.zeros(1, dtype=torch.int64, device=dev)
    ws = _scratch(_ws, "reindex", nodes, n, m)
    _launch("reindex", nodes, _ptr(nodes), n, _ptr(neighbors), m, _ptr(src), _ptr(out_nodes), _ptr(num), _ptr(ws), ws.numel())
    return src, out_nodes[:int(num.item())]


def _host_relabel(nodes, neighbors):
    """The numpy twin of _relabel: the same two arrays."""
    n = int(nodes.shape[0])
    keys = np.concatenate([nodes, neighbors])
    _, first, inverse = np.unique(keys, return_index=True, return_inverse=True)       # first: the lowest position of every id
    fresh = np.sort(first[first >= n])                                                # ids that are no seed, by first appearance
    new_id = np.where(first < n, first, n + np.searchsorted(fresh, first))
    return new_id[np.ravel(inverse)[n:]].astype(np.int64), np.concatenate([nodes, keys[fresh]])


def reindex_heter_graph(nodes, neighbors, count, check_range=True):
    """paddle.geometric.reindex_heter_graph (new_dataset_p2p.py:185-187): `neighbors` and `count` are per-relation lists (what a
    sample_neighbors call per edge type returns) -> (reindex_src, reindex_dst, out_nodes), the relations concatenated in list
    order.  ONE relabel over the concatenation with reindex_graph's contract: out_nodes[:len(nodes)] == nodes as given, new ids
    follow in order of first appearance across the concatenation, a neighbour equal to a seed maps to that seed's first position;
    reindex_dst = every relation's repeat(arange(len(nodes)), count_r) (tests/relation_sampling_defs.py: reindex_heter_restated).
    Device tensors -> pglamd_reindex on the device (check_range: ValueError for a negative id); numpy arrays -> numpy."""
    neighbors, count = list(neighbors), list(count)
    if len(neighbors) != len(count) or not neighbors:
        raise ValueError("pgl_amd reindex_heter_graph: neighbors and count must be lists of equal length >= 1 (one entry per relation)")
    if not isinstance(nodes, torch.Tensor):
        nodes = _np_i64(nodes).reshape(-1)
        flat = np.concatenate([_np_i64(x).reshape(-1) for x in neighbors])
        if check_range and ((nodes.size and nodes.min() < 0) or (flat.size and flat.min() < 0)):
            raise ValueError("pgl_amd reindex_heter_graph: negative ids (ids must be >= 0)")
        src, out_nodes = _host_relabel(nodes, flat)
        ar = np.arange(nodes.shape[0], dtype=np.int64)
        return src, np.concatenate([np.repeat(ar, _np_i64(c).reshape(-1)) for c in count]), out_nodes
    _need_cuda(nodes, *neighbors, *count)
    nodes = nodes.to(torch.int64).reshape(-1).contiguous()
    flat = torch.cat([x.to(torch.int64).reshape(-1) for x in neighbors]).contiguous()
    if check_range and any(int(t.shape[0]) and _ids_out_of_range(t) for t in (nodes, flat)):
        raise ValueError("pgl_amd reindex_heter_graph: negative ids (ids must be >= 0)")
    src, out_nodes = _relabel(nodes, flat)
    n, R = int(nodes.shape[0]), len(count)
    dst = torch.repeat_interleave(torch.arange(n, device=nodes.device).repeat(R), torch.cat([c.to(torch.int64).reshape(-1) for c in count]))
    return src, dst, out_nodes


# ------------------------------------------------------------------------------------------------
# relational aggregation over a StackedIndex (aggregate_rel.hip: pglamd_aggregate_relations)
# ------------------------------------------------------------------------------------------------
# The longest segment one lane group walks by itself.  A group's walk is a chain of dependent loads (col, then the row), eight
# rows at a time, so a long segment keeps one group busy for many memory latencies while the rest of its wave idles.  Measured on
# the RMAT-20 full graph (20 M edges in 4 relations, longest segment 20 837; profiles/relation_aggregate/README.md): without the
# split 13.6 ms, long_row = 1024: 2.79, 256: 2.36, 128: 2.07, 64: 1.99, 32: 1.95, 16: 1.99 ms at d = 64 (d = 128 alike) -- flat
# below 64.  64 = MAX_SAMPLE is also the largest segment a sampler's block can have when every fan-out is >= 0, so those
# blocks never take the second launch or build a list.
LONG_ROW = 64


def stacked_segments(stacked):
    """Segment lengths int64 [R, rows] of a StackedIndex (also of a flat [R * n + 1] table viewed with a relation stride of n)."""
    return stacked.indptr[:, 1:] - stacked.indptr[:, :-1]


def stacked_max_segment(stacked):
    """The longest segment of a StackedIndex: the instance's `max_segment` when someone set it (the sampler knows it from its
    fan-outs), else computed ONCE (one host read) and kept on the instance."""
    m = stacked.__dict__.get("max_segment")
    if m is None:
        seg = stacked_segments(stacked)
        m = stacked.max_segment = int(seg.max().item()) if seg.numel() else 0
    return m


def stacked_long_rows(stacked, long_row):
    """int64 [n] device list of the rows that own a segment longer than `long_row`, or None when max_segment says there is none:
    one compaction and one host read (its length) per (index, long_row), kept on the instance."""
    if stacked_max_segment(stacked) <= long_row:
        return None
    cache = stacked.__dict__.setdefault("_long_rows", {})
    if long_row not in cache:
        rows = (stacked_segments(stacked) > long_row).any(0).nonzero().reshape(-1).contiguous()
        cache[long_row] = rows if int(rows.shape[0]) else None
    return cache[long_row]


def stacked_mean_scale(stacked, out_rows):
    """fp32 [R, out_rows]: 1 / len(seg(r, v)), 0 for an empty segment -- the per-(relation, column) scale the backward of "mean"
    multiplies the incoming gradient by.  torch ops, no host read, kept on the instance per out_rows."""
    cache = stacked.__dict__.setdefault("_mean_scale", {})
    if out_rows not in cache:
        seg = stacked_segments(stacked)[:, :out_rows]
        cache[out_rows] = torch.where(seg > 0, 1.0 / seg.clamp(min=1).to(torch.float32), torch.zeros((), device=seg.device)).contiguous()
    return cache[out_rows]


def aggregate_relations(x, stacked, reduce_op="mean", out_size=None, per_relation=False, col_scale=None, out=None, long_row=None):
    """Every relation's send_recv(x, reduce_op) over a StackedIndex in one launch -- the aggregation of the reference's RGCNConv
    loop (pgl/nn/conv.py:1014-1019).  With seg(r, v) = the positions indptr[r, v] .. indptr[r, v + 1]:
        S[r, v] = s_r(v) * sum over e in seg(r, v) of c[r, col[e]] * x_r[col[e]]       s_r(v) = 1 ("sum") or 1 / len(seg) ("mean")
    x: fp32 [n_src, d] (shared by the relations) or [R, n_src, d] (x_r = x[r]); any strides with a unit last one (a [M, R, d]
    tensor permuted to [R, M, d] is read in place).  col_scale: c, fp32 [R, n_src] or None (all ones).  M = out_size or rows.
    -> out[v] = sum over r of S[r, v], fp32 [M, d]; per_relation=True: S itself as [M, R, d] (so that one GEMM against
    W.reshape(R * d, d_out) finishes an RGCN layer).  out=: write there instead ([M, d] / [M, R, d], any strides with a unit last
    one).  An element without a contributing edge is +0.0; a column outside [0, n_src) contributes nothing; no atomics, the result
    is bit-identical from run to run.  long_row (default LONG_ROW): segments longer than that are summed by a second launch in
    fixed slices (stacked_long_rows: the list is built once per index); with max_segment <= long_row it is one launch and no host
    read.  ValueError before any launch for a dtype other than fp32, a reduce_op other than "sum" / "mean", or shapes that do not
    fit the index."""
    what = "pgl_amd aggregate_relations"
    if reduce_op not in ("sum", "mean"):
        raise ValueError("%s: reduce_op %r (only 'sum' and 'mean' are defined over relations)" % (what, reduce_op))
    R, rows = stacked.num_relations, stacked.num_nodes
    if x.dtype != torch.float32 or (col_scale is not None and col_scale.dtype != torch.float32) or (out is not None and out.dtype != torch.float32):
        raise ValueError("%s: fp32 only (got %s)" % (what, x.dtype))
    if x.dim() not in (2, 3) or (x.dim() == 3 and int(x.shape[0]) != R):
        raise ValueError("%s: features of shape %s for %d relations ([n_src, d] or [R, n_src, d] expected)" % (what, tuple(x.shape), R))
    n_src, d = int(x.shape[-2]), int(x.shape[-1])
    if d < 1:
        raise ValueError("%s: empty feature rows" % what)
    if col_scale is not None and tuple(col_scale.shape) != (R, n_src):
        raise ValueError("%s: col_scale of shape %s, expected (R, n_src) = %s" % (what, tuple(col_scale.shape), (R, n_src)))
    M = _rows_out(out_size, rows)
    if M > rows:
        raise ValueError("%s: out_size %d exceeds the index's %d rows" % (what, M, rows))
    want = (M, R, d) if per_relation else (M, d)
    if out is not None and tuple(out.shape) != want:
        raise ValueError("%s: out of shape %s, expected %s" % (what, tuple(out.shape), want))
    long_row = LONG_ROW if long_row is None else int(long_row)
    if long_row < 1:
        raise ValueError("%s: long_row %d < 1" % (what, long_row))
    _need_cuda(x, stacked.indptr, stacked.col, col_scale, out)
    if x.stride(-1) != 1 and n_src:
        x = x.contiguous()
    if col_scale is not None:
        col_scale = col_scale.contiguous()
    if out is None:
        out = torch.empty(want, dtype=torch.float32, device=x.device)
    elif out.stride(-1) != 1 and M:
        raise ValueError("%s: out needs a unit last stride" % what)
    if M == 0:
        return out
    if stacked.edge_base[-1] == 0:
        return out.zero_()
    long_rows = stacked_long_rows(stacked, long_row)
    indptr = stacked.indptr
    # (torch reports arbitrary strides for dimensions of size 1, which are never stepped over: the packed ones are passed there)
    ldx = x.stride(-2) if n_src > 1 else d
    x_rel = (x.stride(0) if R > 1 else n_src * d) if (x.dim() == 3 and n_src) else 0
    ldo = out.stride(0) if M > 1 else (R * d if per_relation else d)
    o_rel = (out.stride(1) if R > 1 else d) if per_relation else 0
    _launch("aggregate_relations", x, _ptr(x), n_src, ldx, x_rel, _ptr(indptr), indptr.stride(0) if R > 1 else 0, _ptr(stacked.col),
            _ptr(col_scale), n_src, R, M, d, REDUCE[reduce_op], _ptr(out), ldo, o_rel, long_row, _ptr(long_rows),
            0 if long_rows is None else int(long_rows.shape[0]))
    return out


# ------------------------------------------------------------------------------------------------
# PinSAGE neighbourhoods: visit counts of short walks and their top-k (walk_visit.hip)
# ------------------------------------------------------------------------------------------------
VISIT_MAX = 4096         # PGLAMD_VISIT_MAX: num_walks * num_steps, the visits one seed's LDS table holds
VISIT_MAX_TOPK = 256     # PGLAMD_VISIT_MAX_TOPK


def _visit_args(num_walks, num_steps, top_k, what):
    num_walks, num_steps, top_k = int(num_walks), int(num_steps), int(top_k)
    if num_walks < 1 or num_steps < 1 or top_k < 1:
        raise ValueError("pgl_amd %s: num_walks, num_steps and top_k must be >= 1 (got %d, %d, %d)" % (what, num_walks, num_steps, top_k))
    if num_walks * num_steps > VISIT_MAX:
        raise ValueError("pgl_amd %s: num_walks * num_steps = %d x %d exceeds PGLAMD_VISIT_MAX = %d visits per seed"
                         % (what, num_walks, num_steps, VISIT_MAX))
    if top_k > VISIT_MAX_TOPK:
        raise ValueError("pgl_amd %s: top_k %d exceeds PGLAMD_VISIT_MAX_TOPK = %d" % (what, top_k, VISIT_MAX_TOPK))
    return num_walks, num_steps, top_k


def _visit_mode(p, q, weights, what):
    """The visit counts walk uniformly or by edge weight: p / q other than 1 raise what the weighted walk raises for node2vec."""
    mode, _ = walk_params(p, q)
    if weights is not None:
        _weighted_walk_mode(mode, what)
    elif mode != WALK_UNIFORM:
        raise ValueError("pgl_amd %s: node2vec steps (p != 1 or q != 1) are not provided for visit counts; pass p = q = 1" % what)


def walk_visit_topk(csr, seeds, num_walks, num_steps, top_k, seed=0, weights=None, check_range=True, *, p=1.0, q=1.0):
    """PinSAGE neighbourhoods over a successor index whose rows are sorted by dst (Graph._csr_succ_sorted): for every seed the
    top_k nodes most often visited by num_walks walks of num_steps steps from it -> (nbr int64 [S, top_k], padding -1; cnt int32
    [S, top_k], padding 0; num int32 [S] = min(top_k, distinct visited nodes)).  Walker s * num_walks + r takes the walk that row
    of random_walk(csr, seeds.repeat_interleave(num_walks), num_steps, seed=seed, weights=weights) holds; the visits of a seed are
    positions 1 .. len-1 of its walks without the seed itself, counted per node and ordered by (count descending, id ascending)
    (tests/pinsage_defs.py).  One launch, no paths in memory, no host sync unless check_range (then one read of the range flag:
    ValueError for a seed outside [0, N); without it such a seed's row is all -1 / 0).
    num_walks * num_steps <= VISIT_MAX and top_k <= VISIT_MAX_TOPK, else ValueError before any launch.
    weights: a WeightTable over THIS index (Graph.edge_weight_table(w, "succ")): the walks step by edge weight.
    p, q: accepted only as 1 (uniform and edge-weighted steps only; ValueError otherwise, as the weighted walk's)."""
    _need_cuda(seeds)
    seeds = seeds.to(torch.int64).reshape(-1).contiguous()
    num_walks, num_steps, top_k = _visit_args(num_walks, num_steps, top_k, "walk_visit_topk")
    _visit_mode(p, q, weights, "walk_visit_topk")
    if weights is not None:
        _check_table(weights, csr, "walk_visit_topk")
    S, dev = int(seeds.shape[0]), seeds.device
    nbr = torch.empty((S, top_k), dtype=torch.int64, device=dev)
    cnt = torch.empty((S, top_k), dtype=torch.int32, device=dev)
    num = torch.empty(S, dtype=torch.int32, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev) if (check_range and S) else None
    if S:
        _launch("walk_visit_topk", seeds, _ptr(csr.indptr), _ptr(csr.col32), _ptr(None if weights is None else weights.cum), csr.num_nodes,
                _ptr(seeds), S, num_walks, num_steps, top_k, _seed64(seed), _ptr(nbr), _ptr(cnt), _ptr(num), _ptr(flag))
    if flag is not None and int(flag.item()):
        raise ValueError("pgl_amd walk_visit_topk: seeds outside [0, num_nodes=%d)" % csr.num_nodes)
    return nbr, cnt, num


# ------------------------------------------------------------------------------------------------
# host (CPU, numpy) helpers -- same shared library, HOST pointers
# ------------------------------------------------------------------------------------------------
def _np_i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _np_opt_i64(a):
    return None if a is None else _np_i64(a)


def _np_ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _np_out_scalar(ctype):
    """-> (a ctype(0), the void pointer the library writes it through): the cut / milliseconds / count out-parameters."""
    c = ctype(0)
    return c, ctypes.cast(ctypes.pointer(c), ctypes.c_void_p)


def _np_edge_columns(edges):
    """An [E, 2] edge list as the library reads it -> (src, dst, stride in elements, E): two strided int64 views, nothing copied
    when the list is int64 already."""
    e = np.asarray(edges)
    if e.dtype != np.int64:
        e = e.astype(np.int64)
    E = int(e.shape[0])
    if not E:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 2, 0
    return e[:, 0], e[:, 1], e.strides[0] // 8, E


def host_build_index(u, v, num_nodes):
    """graph_kernel.build_index (pgl/graph_kernel.pyx:59-88) for numpy-mode graphs."""
    u = np.asarray(u); v = np.asarray(v)
    if u.dtype != np.int64:
        u = u.astype(np.int64)
    if v.dtype != np.int64:
        v = v.astype(np.int64)
    E, N = int(u.shape[0]), int(num_nodes)
    if u.ndim != 1 or v.ndim != 1 or v.shape[0] != E:
        raise ValueError("u and v must be 1-D of equal length")
    su = u.strides[0] // 8 if E else 1
    sv = v.strides[0] // 8 if E else 1
    degree = np.empty(N, np.int64); indptr = np.empty(N + 1, np.int64)
    sorted_v = np.empty(E, np.int64); sorted_u = np.empty(E, np.int64); sorted_eid = np.empty(E, np.int64)
    _ffi.check(_ffi.lib().pglamd_build_index_host(_np_ptr(u), su, _np_ptr(v), sv, E, N, _np_ptr(degree),
                                                  _np_ptr(sorted_v), _np_ptr(sorted_u), _np_ptr(sorted_eid),
                                                  _np_ptr(indptr)), "build_index_host")
    return degree, sorted_v, sorted_u, sorted_eid, indptr


def host_map_ids(ids, reindex):
    """graph_kernel.map_nodes (pyx:123-138): ids -> reindex[ids] (missing keys map to 0)."""
    ids = _np_i64(ids)
    keys = _np_i64(list(reindex.keys())); vals = _np_i64(list(reindex.values()))
    out = np.empty(ids.shape, np.int64)
    _ffi.check(_ffi.lib().pglamd_map_ids(_np_ptr(keys), _np_ptr(vals), len(keys), _np_ptr(ids), ids.size, _np_ptr(out)),
               "map_ids")
    return out


def host_partition_kway(num_nodes, indptr, adjncy, nparts, node_weights=None, edge_weights=None, seed=0):
    """Engine partitioner standing in for METIS_PartGraphKway (pgl/graph_kernel.pyx:434-472)."""
    indptr = _np_i64(indptr); adjncy = _np_i64(adjncy)
    vw, ew = _np_opt_i64(node_weights), _np_opt_i64(edge_weights)
    part = np.empty(int(num_nodes), np.int64)
    cut, p_cut = _np_out_scalar(ctypes.c_int64)
    _ffi.check(_ffi.lib().pglamd_partition_kway(int(num_nodes), _np_ptr(indptr), _np_ptr(adjncy), _np_ptr(vw),
                                                _np_ptr(ew), int(nparts), int(seed), _np_ptr(part), p_cut), "partition_kway")
    return part, int(cut.value)


def host_partition_kway2(num_nodes, indptr, adjncy, nparts, node_weights=None, node_weights2=None, edge_weights=None,
                         ub=1.03, ub2=1.03, seed=0, threads=0):
    """pglamd_partition_kway2: the engine's partitioner with a second balance constraint and explicit imbalance bounds."""
    indptr = _np_i64(indptr); adjncy = _np_i64(adjncy)
    vw, vw2, ew = _np_opt_i64(node_weights), _np_opt_i64(node_weights2), _np_opt_i64(edge_weights)
    part = np.empty(int(num_nodes), np.int64)
    cut, p_cut = _np_out_scalar(ctypes.c_int64)
    _ffi.check(_ffi.lib().pglamd_partition_kway2(int(num_nodes), _np_ptr(indptr), _np_ptr(adjncy), _np_ptr(vw), _np_ptr(vw2),
                                                 _np_ptr(ew), int(nparts), float(ub), float(ub2), int(seed), int(threads),
                                                 _np_ptr(part), p_cut), "partition_kway2")
    return part, int(cut.value)


def host_partition_edges(edges, num_nodes, nparts, node_weights=None, node_weights2=None, ub=1.03, ub2=1.03, seed=0, threads=0):
    """pglamd_partition_edges: partition the graph of a DIRECTED [E, 2] int64 edge list (symmetrised inside the library)."""
    src, dst, st, E = _np_edge_columns(edges)
    vw, vw2 = _np_opt_i64(node_weights), _np_opt_i64(node_weights2)
    part = np.empty(int(num_nodes), np.int64)
    cut, p_cut = _np_out_scalar(ctypes.c_int64)
    _ffi.check(_ffi.lib().pglamd_partition_edges(_np_ptr(src), st, _np_ptr(dst), st, E, int(num_nodes), _np_ptr(vw), _np_ptr(vw2),
                                                 int(nparts), float(ub), float(ub2), int(seed), int(threads), _np_ptr(part), p_cut),
               "partition_edges")
    return part, int(cut.value)


def host_halo_plan(edges, num_nodes, part, rank, world):
    """pglamd_halo_plan_sizes / _fill: one rank's pull plan as a dict of int64 numpy arrays (see include/pgl_amd.h)."""
    src, dst, st, E = _np_edge_columns(edges)
    part, N = _np_i64(part), int(num_nodes)
    L = _ffi.lib()
    sizes = np.zeros(5, np.int64)
    args = (_np_ptr(src), st, _np_ptr(dst), st, E, N, _np_ptr(part), int(rank), int(world))
    _ffi.check(L.pglamd_halo_plan_sizes(*args, _np_ptr(sizes)), "halo_plan_sizes")
    n_own, n_loc, n_hal, n_halo, n_send = (int(v) for v in sizes)
    out = {"offsets": np.zeros(world + 1, np.int64), "own_global": np.zeros(n_own, np.int64), "loc_rows": np.zeros(n_loc, np.int64),
           "loc_cols": np.zeros(n_loc, np.int64), "hal_rows": np.zeros(n_hal, np.int64), "hal_cols": np.zeros(n_hal, np.int64),
           "halo_global": np.zeros(n_halo, np.int64), "send_idx": np.zeros(n_send, np.int64), "halo_splits": np.zeros(world, np.int64),
           "pull_splits": np.zeros(world, np.int64), "in_degree": np.zeros(n_own, np.int64), "out_degree": np.zeros(n_own, np.int64),
           "edge_global": np.zeros(n_loc + n_hal, np.int64)}
    order = ("offsets", "own_global", "loc_rows", "loc_cols", "hal_rows", "hal_cols", "halo_global", "send_idx", "halo_splits",
             "pull_splits", "in_degree", "out_degree", "edge_global")
    _ffi.check(L.pglamd_halo_plan_fill(*args, *[_np_ptr(out[k]) for k in order]), "halo_plan_fill")
    return out


# ------------------------------------------------------------------------------------------------
# layer epilogue (row f1): bias + activation + L2 row normalisation in one pass each way
# ------------------------------------------------------------------------------------------------
def row_epilogue_width_ok(d):
    """Row widths pglamd_row_epilogue covers (one wave per row, <= 8 vectors per lane)."""
    d = int(d)
    vec = 4 if d % 4 == 0 else 2 if d % 2 == 0 else 1
    return 0 < d <= 64 * vec * 8


def _row_epilogue_lane_bytes(d):
    """Bytes per lane of pglamd_row_epilogue / _backward on rows of d floats: what z, dy and y must be aligned to."""
    return 16 if d % 4 == 0 else 8 if d % 2 == 0 else 4


def row_epilogue_supported(z, width=None):
    """True when the fused epilogue can run on a tensor shaped / typed like `z` whose rows are `width` wide (default: z's own
    width).  Layers gate on the tensor the kernel PROCESSES -- the GEMM output, `width` = hidden / output size -- not on the
    GEMM's input."""
    if not (z.is_cuda and z.dtype == torch.float32 and z.dim() == 2):
        return False
    return row_epilogue_width_ok(z.shape[-1] if width is None else width)


def row_epilogue(z, bias=None, act=None, normalize=False, eps=1e-12):
    """y = normalize_L2(act(z + bias)) -> (y, inv_norm or None).  act: None | "relu".  GraphSageConv's epilogue
    (pgl/nn/conv.py:109-115) and GCNConv's (pgl/nn/conv.py:250-254) in one kernel."""
    _need_cuda(z, bias)
    if z.dtype != torch.float32 or z.dim() != 2 or (bias is not None and bias.dtype != torch.float32):
        raise TypeError("row_epilogue: float32 [n, d] rows and a float32 bias (got %s / %s)"
                        % (z.dtype, None if bias is None else bias.dtype))
    if not row_epilogue_width_ok(z.shape[1]):
        raise ValueError("row_epilogue: rows of %d elements are wider than the kernel covers" % z.shape[1])
    n, d = int(z.shape[0]), int(z.shape[1])
    z = _aligned(z, _row_epilogue_lane_bytes(d))
    y = torch.empty_like(z)
    inv = torch.empty(n, dtype=torch.float32, device=z.device) if normalize else None
    if n:
        b = None if bias is None else bias.contiguous()
        _launch("row_epilogue", z, _ptr(z), _ptr(b), n, d, 1 if act == "relu" else 0, int(bool(normalize)), float(eps), _ptr(y), _ptr(inv))
    return y, inv


def row_epilogue_backward(dy, y, inv_norm, act=None, normalize=False, want_bias=False):
    """-> (dz, dbias or None) for row_epilogue."""
    _need_cuda(dy, y, inv_norm)
    n, d = int(dy.shape[0]), int(dy.shape[1])
    lane = _row_epilogue_lane_bytes(d)
    dy = _aligned(dy, lane); y = _aligned(y, lane)
    inv_norm = None if inv_norm is None else inv_norm.contiguous()
    dz = torch.empty_like(dy)
    part = torch.zeros((int(_ffi.lib().pglamd_row_epilogue_partials(n)), d), dtype=torch.float32, device=dy.device) if want_bias else None
    if n:
        _launch("row_epilogue_backward", dy, _ptr(dy), _ptr(y), _ptr(inv_norm), n, d, 1 if act == "relu" else 0, int(bool(normalize)),
                _ptr(dz), _ptr(part))
    return dz, (part.sum(0) if want_bias else None)


def host_random_walk(indptr, col, starts, num_steps, p=1.0, q=1.0, plus=False, seed=0, max_trials=None, threads=0, weights=None):
    """The host twin of random_walk (pglamd_random_walk_host: same step logic, same RNG, bit-identical result) for numpy-mode
    graphs: indptr int64 [N+1] and col [E] of the dst-sorted successor index, numpy in and out.  threads <= 0: up to 16.
    weights: a WeightTable of numpy arrays over this index (host_edge_weight_table), p == q == 1 only."""
    indptr = _np_i64(indptr); col = np.ascontiguousarray(col, dtype=np.int32); starts = _np_i64(starts).reshape(-1)
    mode, thr = walk_params(p, q, plus)
    num_steps, max_trials = _walk_args(num_steps, max_trials, p, q)
    W, N = int(starts.shape[0]), int(indptr.shape[0]) - 1
    paths = np.empty((W, num_steps + 1), np.int64)
    lengths = np.empty(W, np.int64)
    if weights is not None:
        _weighted_walk_mode(mode, "host_random_walk")
        if not isinstance(weights, WeightTable) or weights.cum.shape != col.shape or weights.npos.shape != (N,):
            raise ValueError("pgl_amd host_random_walk: weights must be a WeightTable over this index (host_edge_weight_table)")
    rc = 0
    if W and weights is not None:
        cum = _np_i64(weights.cum)
        rc = _ffi.lib().pglamd_random_walk_weighted_host(_np_ptr(indptr), _np_ptr(col), _np_ptr(cum), N, _np_ptr(starts),
                                                         W, num_steps, _seed64(seed), int(threads), _np_ptr(paths),
                                                         _np_ptr(lengths))
    elif W:
        rc = _ffi.lib().pglamd_random_walk_host(_np_ptr(indptr), _np_ptr(col), N, _np_ptr(starts), W, num_steps, mode, thr[0], thr[1],
                                                thr[2], max_trials, _seed64(seed), int(threads), _np_ptr(paths),
                                                _np_ptr(lengths))
    if rc == -3:            # PGLAMD_E_RANGE: a start outside [0, N) -- the ValueError the device path raises too
        raise ValueError("pgl_amd random_walk: %s" % _ffi.lib().pglamd_last_error().decode("utf-8", "replace"))
    _ffi.check(rc, "random_walk_host")
    return paths, lengths


def host_sample_negatives(indptr, col, src, num_neg, seed=0, lo=0, hi=None, noise=None, exclude_self=False, max_trials=None,
                          return_pos=False, allow_empty=False, threads=0):
    """The host twin of sample_negatives (pglamd_sample_negatives_host: the same draws, bit-identical result whatever the thread
    count) for numpy-mode graphs: indptr int64 [N+1] and col [E] of a successor index whose rows are sorted by dst, numpy in and
    out.  noise: a single-row WeightTable of numpy arrays (host_edge_weight_table([0, n], w)).  threads <= 0: up to 16.
    ValueError for a source outside [0, N), and for a source with no negative unless allow_empty."""
    indptr = _np_i64(indptr); col = np.ascontiguousarray(col, dtype=np.int32); src = _np_i64(src).reshape(-1)
    N = int(indptr.shape[0]) - 1
    num_neg, lo, hi, max_trials = _negative_args(N, num_neg, lo, hi, noise, max_trials, "host_sample_negatives")
    cum = None if noise is None else _np_i64(noise.cum)
    n = int(src.shape[0])
    neg = np.empty((n, num_neg), np.int64)
    pos = np.empty(n, np.int64) if return_pos else None
    flags = np.zeros(1, np.int32)
    rc = _ffi.lib().pglamd_sample_negatives_host(_np_ptr(indptr), _np_ptr(col), N, _np_ptr(cum), lo, hi, _np_ptr(src), n, num_neg,
                                                 int(bool(exclude_self)), max_trials, _seed64(seed), int(threads), _np_ptr(neg),
                                                 _np_ptr(pos), _np_ptr(flags))
    if rc == -3:            # PGLAMD_E_RANGE: a source outside [0, N) -- the ValueError the device path raises too
        raise ValueError("pgl_amd sample_negatives: %s" % _ffi.lib().pglamd_last_error().decode("utf-8", "replace"))
    _ffi.check(rc, "sample_negatives_host")
    _raise_negative_flags(int(flags[0]), N, allow_empty, "host_sample_negatives")
    return (neg, pos) if return_pos else neg


def host_walk_visit_topk(indptr, col, seeds, num_walks, num_steps, top_k, seed=0, weights=None, threads=0, check_range=True, *,
                         p=1.0, q=1.0):
    """The host twin of walk_visit_topk (pglamd_walk_visit_topk_host: the same walks, the same integer counts and order,
    bit-identical result) for numpy-mode graphs: indptr int64 [N+1] and col [E] of the dst-sorted successor index, numpy in
    and out -> (nbr int64 [S, top_k], cnt int32 [S, top_k], num int32 [S]).  threads <= 0: up to 16.
    weights: a WeightTable of numpy arrays over this index (host_edge_weight_table)."""
    indptr = _np_i64(indptr); col = np.ascontiguousarray(col, dtype=np.int32); seeds = _np_i64(seeds).reshape(-1)
    num_walks, num_steps, top_k = _visit_args(num_walks, num_steps, top_k, "host_walk_visit_topk")
    _visit_mode(p, q, weights, "host_walk_visit_topk")
    S, N = int(seeds.shape[0]), int(indptr.shape[0]) - 1
    cum = None
    if weights is not None:
        if not isinstance(weights, WeightTable) or weights.cum.shape != col.shape or weights.npos.shape != (N,):
            raise ValueError("pgl_amd host_walk_visit_topk: weights must be a WeightTable over this index (host_edge_weight_table)")
        cum = _np_i64(weights.cum)
    nbr = np.empty((S, top_k), np.int64)
    cnt = np.empty((S, top_k), np.int32)
    num = np.empty(S, np.int32)
    flag = np.zeros(1, np.int32)
    if S:
        _ffi.check(_ffi.lib().pglamd_walk_visit_topk_host(_np_ptr(indptr), _np_ptr(col), _np_ptr(cum), N, _np_ptr(seeds), S, num_walks,
                                                          num_steps, top_k, _seed64(seed), int(threads), _np_ptr(nbr), _np_ptr(cnt),
                                                          _np_ptr(num), _np_ptr(flag)), "walk_visit_topk_host")
    if check_range and int(flag[0]):
        raise ValueError("pgl_amd walk_visit_topk: seeds outside [0, num_nodes=%d)" % N)
    return nbr, cnt, num
