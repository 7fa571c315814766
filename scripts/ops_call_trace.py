#!/usr/bin/env python3
"""Call trace of the Python front end (pgl_amd/ops.py): which library calls a fixed list of small cases makes, with which
arguments, and what comes back.  For showing that a change to the front end left every call into libpglamd.so as it was:
run it on the commit before and on the commit after and diff the two files.

    python scripts/ops_call_trace.py OUT.jsonl

Needs one GPU.  In a fresh process `_ffi._lib` is swapped for a proxy that forwards every call and writes one JSON line per call:
the symbol, every scalar argument as it is, every pointer argument as "ptr" or "NULL", and the return value.  After each case
one more line gives shape, dtype and the SHA-256 of the bytes of every tensor the case returned (after a synchronize).  The
cases run in a fixed order on seeded inputs -- the order also fixes which scratch buffer `_ws_hot` hands out -- and use nothing
but the public functions of `pgl_amd.ops` (and the module switches `_GAT_POS_STATS` / `_GAT_BWD_EDGE_BUFFER` / `_COO_ONCE_MAX` that
tests assign to).

The graph: 37 nodes, 300 edges, destination 5 receives 150 of them (the row straddles the 64-edge chunks, so the split-row
fix-up runs), nodes 11 and 29 receive none, out_size 41.  The atomic scatter_add_coo route is order-nondeterministic by
contract: its call is traced, its result is not hashed.

The attention family runs a second time at the end, on the "classes" graph (3 000 nodes, 12 554 edges): on the dst-sorted and on the
src-sorted stream its first five rows have 1025, 63, 1089, 100 and 3000 edges -- with 64-edge chunks a row finished by one wave at the
limit of 16 further pieces, an unsplit row, the first row (17) of the block-parallel fix-up, a row with 1 further piece and a hub --
at (heads, head_dim) = (4, 8), (8, 16), (8, 32): 1, 2 and 4 columns per lane.
"""
import ctypes
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from pgl_amd import _ffi, ops

N, E, HUB, EMPTY, M = 37, 300, 5, (11, 29), 41


class Recorder(object):
    """Stands where the ctypes handle stands: every pglamd_* attribute is the real function behind a recording wrapper."""

    def __init__(self, real, sink):
        self.__dict__["_real"], self.__dict__["_sink"], self.__dict__["case"] = real, sink, ""

    def __setattr__(self, k, v):
        self.__dict__[k] = v

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name not in _ffi._SIGNATURES:
            return fn
        res, argtypes = _ffi._SIGNATURES[name]

        def call(*args):
            assert len(args) == len(argtypes), name
            rc = fn(*args)
            rec = {"case": self.case, "sym": name, "args": [_describe(a, t) for a, t in zip(args, argtypes)],
                   "ret": rc.decode("utf-8", "replace") if isinstance(rc, bytes) else rc}
            self._sink.write(json.dumps(rec) + "\n")
            return rc
        self.__dict__[name] = call
        return call


def _describe(a, argtype):
    if argtype is ctypes.c_void_p:
        v = a.value if isinstance(a, ctypes.c_void_p) else a
        return "ptr" if v else "NULL"
    if isinstance(a, bytes):
        return a.decode()
    return a


def _tensors(r):
    """The tensors of a result, in a fixed order; None stays None."""
    if r is None or isinstance(r, torch.Tensor):
        return [r]
    if isinstance(r, ops.CSR):
        return [getattr(r, k) for k in ops.CSR.__slots__ if not k.startswith("_") and isinstance(getattr(r, k), torch.Tensor)]
    if isinstance(r, (tuple, list)):
        return [t for x in r for t in _tensors(x)]
    raise TypeError(type(r))


def _digest(t):
    if t is None:
        return None
    b = t.detach().contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes()
    return {"shape": list(t.shape), "dtype": str(t.dtype), "sha256": hashlib.sha256(b).hexdigest()}


CLASS_ROWS, CLASS_N, CLASS_FILL = (1025, 63, 1089, 100, 3000), 3000, 2000


def classes_graph(rng):
    """-> (src, dst): nodes 0..4 receive CLASS_ROWS edges each and send CLASS_ROWS edges each; no other edge touches them."""
    k, heavy = sum(CLASS_ROWS), np.repeat(np.arange(len(CLASS_ROWS)), CLASS_ROWS)
    src = np.concatenate([rng.integers(100, CLASS_N - 100, k), heavy, rng.integers(100, CLASS_N - 100, CLASS_FILL)])
    dst = np.concatenate([heavy, rng.integers(50, CLASS_N, k), rng.integers(50, CLASS_N, CLASS_FILL)])
    order = rng.permutation(src.shape[0])
    src, dst = src[order].astype(np.int64), dst[order].astype(np.int64)
    for ids in (src, dst):                                           # further pieces of the first five rows, 64-edge chunks
        ptr = np.concatenate([[0], np.cumsum(np.bincount(ids, minlength=CLASS_N))])
        assert [int((ptr[r + 1] - 1) // 64 - ptr[r] // 64) for r in range(5)] == [16, 0, 17, 1, 47]
    return src, dst


def main(path):
    dev = torch.device("cuda:0")
    real = _ffi.lib()
    sink = open(path, "w")
    rec = _ffi._lib = Recorder(real, sink)
    rng = np.random.default_rng(20)

    def cu(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    def rand(*shape, dtype=torch.float32):
        return cu(rng.standard_normal(shape)).to(dtype)

    def case(name, fn, hashed=True):
        rec.case = name
        try:
            r = fn()
        except (ValueError, TypeError, OverflowError) as e:           # an input the front end or the library turns away: traced as such
            r, out = None, {"raised": type(e).__name__, "message": str(e)}
        else:
            torch.cuda.synchronize()
            out = [_digest(t) if hashed else "not hashed" for t in _tensors(r)]
        sink.write(json.dumps({"case": name, "out": out}) + "\n")
        sink.flush()
        return r

    # ---- the graph ------------------------------------------------------------------------------------------------------
    receivers = np.array([v for v in range(N) if v != HUB and v not in EMPTY])
    dst = np.concatenate([np.full(150, HUB), receivers, rng.choice(receivers, E - 150 - len(receivers))]).astype(np.int64)
    src = rng.integers(0, N, E).astype(np.int64)
    order = rng.permutation(E)
    src, dst = src[order], dst[order]
    assert np.bincount(dst, minlength=N)[HUB] == 150 and all(np.bincount(dst, minlength=N)[list(EMPTY)] == 0)
    src_t, dst_t = cu(src), cu(dst)
    src32, dst32 = src_t.int(), dst_t.int()
    both = cu(np.stack([src, dst], 1))

    csr = case("csr_build", lambda: ops.csr_build(dst_t, src_t, N))
    csr_src = case("csr_build.transposed_strided_no_i64", lambda: ops.csr_build(both[:, 0], both[:, 1], N, want_i64=False))
    case("csr_from_sorted", lambda: ops.csr_from_sorted(csr.sorted_u, csr.sorted_v, N))
    succ = case("csr_build.successors", lambda: ops.csr_build(csr.col32.long(), csr.row32.long(), N, want_i64=False, check_range=False))
    case("unique_segment", lambda: ops.unique_segment(csr.degree, csr.sorted_u))
    case("exclusive_scan_i64", lambda: ops.exclusive_scan_i64(csr.degree))
    case("narrow_i64", lambda: ops.narrow_i64(both[:, 1]))
    case("seg_ptr_from_ids", lambda: ops.seg_ptr_from_ids(csr.row32, N))

    # ---- aggregate: every route ---------------------------------------------------------------------------------------------
    scale = rand(N).abs() + 0.5
    agg = lambda name, x, index=csr, **kw: case("aggregate." + name, lambda: ops.aggregate(x, index, kw.pop("reduce_op", "sum"), M, **kw))
    x8 = rand(N, 8)
    agg("group_fp32_d8", x8)
    agg("narrow_fp32_d1", rand(N, 1))
    agg("mean_dst_scale", x8, reduce_op="mean", dst_scale=rand(M).abs() + 0.5)
    agg("min_d8", x8, reduce_op="min")
    agg("edge_scale_sum_d33", rand(N, 33), src_scale=scale)
    agg("edge_scale_mean_d33_cached", rand(N, 33), reduce_op="mean", src_scale=scale)
    agg("prescale_fp64_d8", rand(N, 8, dtype=torch.float64), src_scale=scale)
    agg("prescale_fp32_d8", x8, src_scale=scale.reshape(N, 1))
    agg("fused_max_d192", rand(N, 192), reduce_op="max", src_scale=scale)
    agg("fused_fp64_d96", rand(N, 96, dtype=torch.float64), src_scale=scale)
    agg("y_add_E1", x8, y=rand(E, 1), message_op="add")
    agg("y_sub_Ed", x8, y=rand(E, 8), message_op="sub")
    agg("y_mul_E1_max", x8, y=rand(E, 1), message_op="mul", reduce_op="max")
    agg("y_div_Ed", x8, y=rand(E, 8).abs() + 0.5, message_op="div")
    agg("y_mul_src_scale_fused", x8, y=rand(E, 8), message_op="mul", src_scale=scale)
    agg("y_heads_broadcast", rand(N, 2, 4), y=rand(E, 2, 1), message_op="mul")
    wide_in, wide_out = rand(N, 48), torch.zeros(M, 40, device=dev)
    agg("column_block_x", wide_in[:, 8:40])
    agg("column_blocks_both", wide_in[:, 8:40], out=wide_out[:, 4:36])
    case("aggregate.column_block_parent", lambda: wide_out)
    full = rand(N, 8)
    agg("x2_split_30", full[:30], x2=full[30:])
    agg("x2_split_30_max_row", full[:30], index=csr.view(max_row=150), x2=full[30:], reduce_op="max")
    deg = np.bincount(dst, minlength=N)
    deg[EMPTY[0]] = 1                                                # a row empty in this index, filled elsewhere: left untouched
    zin = cu(np.concatenate([[0], np.cumsum(deg)]).astype(np.int64))
    agg("zero_indptr", x8, zero_indptr=zin, out=torch.full((M, 8), 7.0, device=dev))
    agg("zero_indptr_prescale", x8, zero_indptr=zin, src_scale=scale, out=torch.full((M, 8), 7.0, device=dev))
    agg("zero_indptr_edge_scale", rand(N, 33), zero_indptr=zin, src_scale=scale, out=torch.full((M, 33), 7.0, device=dev))
    agg("max_row_150", x8, index=csr.view(max_row=150))
    agg("max_row_150_y", x8, index=csr.view(max_row=150), y=rand(E, 1), message_op="mul")
    agg("deal_chunks", x8, deal_chunks=True)
    agg("deal_chunks_edge_scale", rand(N, 33), deal_chunks=True, src_scale=scale)
    for mode in (0, 1, 2):
        agg("accumulate_%d" % mode, x8, out=torch.full((M, 8), 3.0, device=dev), accumulate=mode)
    agg("accumulate_true_max", x8, out=torch.full((M, 8), 0.25, device=dev), accumulate=True, reduce_op="max")
    agg("fp16_d32", rand(N, 32, dtype=torch.float16))
    agg("bf16_d32", rand(N, 32, dtype=torch.bfloat16))
    agg("fp16_d32_src_scale", rand(N, 32, dtype=torch.float16), src_scale=scale)
    agg("int32_sum", cu(rng.integers(-50, 50, (N, 4)).astype(np.int32)))
    agg("int64_sum", cu(rng.integers(-50, 50, (N, 4)).astype(np.int64)))
    agg("int32_src_scale_fused", cu(rng.integers(-50, 50, (N, 4)).astype(np.int32)), src_scale=scale)
    agg("edge_rows_index", rand(E, 4), index=csr.view(col32=csr.eid32, edge_rows=True), src_scale=rand(E).abs() + 0.5)
    agg("zero_width", rand(N, 0))
    case("aggregate.out_size_default", lambda: ops.aggregate(x8, csr, "sum"))
    empty = ops.CSR(torch.zeros(N + 1, dtype=torch.int64, device=dev), *(torch.zeros(0, dtype=torch.int32, device=dev) for _ in range(3)), N, 0)
    agg("no_edges", x8, index=empty)
    agg("no_edges_column_block_out", x8, index=empty, out=wide_out[:, 0:8])

    # ---- every other device wrapper ---------------------------------------------------------------------------------------------
    data = rand(E, 4)
    case("segment_reduce.sum_i64", lambda: ops.segment_reduce(data, csr.sorted_u, "sum", N))
    case("segment_reduce.max_i32", lambda: ops.segment_reduce(data, csr.row32, "max", N))
    case("segment_reduce.mean_read_back", lambda: ops.segment_reduce(data, csr.sorted_u, "mean"))
    case("segment_softmax.edge_order", lambda: ops.segment_softmax(rand(E, 2), ops.SegView(csr.indptr, csr.row32, dst32, csr.eid32)))
    case("segment_softmax.sorted", lambda: ops.segment_softmax(rand(E, 2), ops.SegView(csr.indptr, csr.row32, csr.row32, None)))

    H, D = 2, 4
    feat, a_s, a_d, g_out = rand(N, H, D), rand(N, H), rand(N, H), rand(N, H, D)
    case("gat_aggregate.plain", lambda: ops.gat_aggregate(feat, a_s, a_d, csr))
    case("gat_aggregate.dropout_out_size", lambda: ops.gat_aggregate(feat, a_s, a_d, csr, 0.1, M, False, 0.5, (1 << 40) + 12345))
    for pos in (True, False):
        ops._GAT_POS_STATS = pos
        st = case("gat_aggregate.stats_pos_%d" % pos, lambda: ops.gat_aggregate(feat, a_s, a_d, csr, return_stats=True))
        case("gat_backward.pos_%d" % pos, lambda: ops.gat_backward(g_out, feat, st[0], a_s, a_d, st[1], st[2], csr, csr_src, 0.2, 0.0, 0, st[3], st[4]))
    ops._GAT_POS_STATS = True
    yh, w = rand(N, H, D), rand(H, D)
    case("sddmm", lambda: ops.sddmm(feat, yh, csr))
    case("add_score", lambda: ops.add_score(feat, yh, w, csr, 0.2))
    g_score = rand(E, H)
    case("add_score_backward.rows_and_w", lambda: ops.add_score_backward(feat, yh, w, g_score, csr, N, 0.2, want_w=True))
    case("add_score_backward.cols", lambda: ops.add_score_backward(yh, feat, w, g_score, csr_src, N, 0.2))

    idx = cu(rng.integers(0, N, 50).astype(np.int64))
    case("gather_rows.i64", lambda: ops.gather_rows(x8, idx))
    case("gather_rows.i32_scalar", lambda: (ops.gather_rows(x8, idx.int()), ops.gather_rows(x8, idx[3])))
    case("gather_rows_cast.fp16_index", lambda: ops.gather_rows_cast(x8, idx, torch.float16))
    case("gather_rows_cast.bf16_column_block", lambda: ops.gather_rows_cast(wide_in[:, 8:40], None, torch.bfloat16))
    case("gather_rows_cast.widen_into_out", lambda: ops.gather_rows_cast(x8.half(), None, torch.float32, out=torch.empty(N, 8, device=dev)))
    perm = cu(rng.permutation(N).astype(np.int64))
    case("scatter_rows", lambda: ops.scatter_rows(torch.zeros(N, 8, device=dev), perm, x8))
    case("degree_norm.fp32", lambda: ops.degree_norm(csr.degree))
    case("degree_norm.fp64", lambda: ops.degree_norm(csr.degree, torch.float64))
    case("send_uv.add", lambda: ops.send_uv(x8, rand(N, 8), src32, dst32, "add"))
    case("send_uv.mul_broadcast", lambda: ops.send_uv(rand(N, 2, 1), rand(N, 1, 3, dtype=torch.float64), src32, dst32, "mul"))
    case("send_u_recv.atomic", lambda: ops.send_u_recv(x8, src_t, dst_t, "sum", M), hashed=False)
    case("send_u_recv.index_max", lambda: ops.send_u_recv(x8, src_t, dst_t, "max", M))
    coo_max, ops._COO_ONCE_MAX = ops._COO_ONCE_MAX, 0
    case("send_u_recv.index_sum", lambda: ops.send_u_recv(x8, src32, dst32, "sum"))
    ops._COO_ONCE_MAX = coo_max

    won = ops.aggregate(x8, csr, "max", N)
    case("winner_grad", lambda: ops.winner_grad(rand(N, 8), won, x8, csr_src))
    grad = rand(N, 8)
    case("edge_operand_grad.mul", lambda: ops.edge_operand_grad(grad, x8, None, csr, "mul", (E, 1)))
    case("edge_operand_grad.div_dst_scale", lambda: ops.edge_operand_grad(grad, x8, rand(E, 8).abs() + 0.5, csr, "div", (E, 8), rand(N).abs()))
    case("edge_operand_grad.add", lambda: ops.edge_operand_grad(grad, x8, None, csr, "add", (E, 8)))
    x64, w64 = rand(N, 64), rand(64, 16)
    case("aggregate_dense.plain", lambda: ops.aggregate_dense(x64, csr, w64))
    case("aggregate_dense.all", lambda: ops.aggregate_dense(x64, csr, w64, rand(16), "relu", "mean", rand(M).abs(), M, True, scale))
    z, bias = rand(N, 16), rand(16)
    case("row_epilogue.plain", lambda: ops.row_epilogue(z))
    ep = case("row_epilogue.all", lambda: ops.row_epilogue(z, bias, "relu", True))
    case("row_epilogue_backward.all", lambda: ops.row_epilogue_backward(rand(N, 16), ep[0], ep[1], "relu", True, True))
    case("row_epilogue_backward.plain", lambda: ops.row_epilogue_backward(rand(N, 16), ep[0], None))

    wt = rng.random(E).astype(np.float32) + 0.1
    wt[rng.choice(E, 20, replace=False)] = 0.0
    table = case("edge_weight_table.index_order", lambda: ops.edge_weight_table(csr, cu(wt)))
    table_succ = case("edge_weight_table.eid_fp64", lambda: ops.edge_weight_table(succ, cu(wt.astype(np.float64)), succ.eid32))
    row = case("weight_table", lambda: ops.weight_table(cu(wt[:20])))
    case("sample_from_table", lambda: (ops.sample_from_table(row, 50, seed=9), ops.sample_from_table(row.cum, 0)))
    seeds = cu(np.array([HUB, 0, EMPTY[0], 17, 30, 3], np.int64))
    nb = case("sample_neighbors.plain", lambda: ops.sample_neighbors(csr, seeds, 4, seed=(1 << 63) + 7, return_eids=True))
    case("sample_neighbors.all", lambda: ops.sample_neighbors(csr, seeds, -1, check_range=False))
    case("sample_neighbors.weighted", lambda: ops.sample_neighbors(csr, seeds, 4, seed=7, return_eids=True, weights=table))
    case("sample_neighbors.none", lambda: ops.sample_neighbors(csr, seeds[2:3], 4))
    case("reindex_graph", lambda: ops.reindex_graph(seeds, nb[0], nb[1]))
    case("induced_subgraph", lambda: ops.induced_subgraph(csr, cu(np.array([HUB, 1, 2, 3, 8, 13, 21, 34, 30, 17], np.int64))))
    case("induced_subgraph.no_edges", lambda: ops.induced_subgraph(csr, cu(np.array([EMPTY[0]], np.int64)), check=False))
    starts = cu(np.arange(N, dtype=np.int64))
    walk = case("random_walk.uniform", lambda: ops.random_walk(succ, starts, 6, seed=3))
    case("random_walk.node2vec", lambda: ops.random_walk(succ, starts, 6, p=0.25, q=4.0, seed=-1, check_range=False))
    case("random_walk.plus_scan_only", lambda: ops.random_walk(succ, starts, 6, p=4.0, q=0.25, plus=True, seed=5, max_trials=0))
    case("random_walk.weighted", lambda: ops.random_walk(succ, starts, 6, seed=11, weights=table_succ))
    case("skip_gram_pairs", lambda: ops.skip_gram_pairs(walk[0], walk[1], 3, seed=5))

    # ---- the attention family over every class of split row, at 1, 2 and 4 columns per lane ---------------------------------------
    c_src, c_dst = classes_graph(rng)
    n, e = CLASS_N, len(c_src)
    ccsr = case("classes.csr_build", lambda: ops.csr_build(cu(c_dst), cu(c_src), n))
    ccsr_src = case("classes.csr_build.transposed", lambda: ops.csr_build(cu(c_src), cu(c_dst), n, want_i64=False))
    routes = (("pos_stats", True, True), ("edge_buffer", False, True), ("two_walks", False, False))
    keep = (ops._GAT_POS_STATS, ops._GAT_BWD_EDGE_BUFFER)
    for H, D in ((4, 8), (8, 16), (8, 32)):
        tag = "classes.%dx%d." % (H, D)
        feat, a_s, a_d, g_out = rand(n, H, D), rand(n, H), rand(n, H), rand(n, H, D)
        case(tag + "gat_aggregate.plain", lambda: ops.gat_aggregate(feat, a_s, a_d, ccsr))
        case(tag + "gat_aggregate.dropout", lambda: ops.gat_aggregate(feat, a_s, a_d, ccsr, 0.2, None, False, 0.4, 99))
        for name, pos, buf in routes:
            ops._GAT_POS_STATS, ops._GAT_BWD_EDGE_BUFFER = pos, buf
            if name != "two_walks":                                  # (the forward of the two-walk route is the edge-buffer route's)
                st = case(tag + "gat_aggregate.stats_pos_%d" % pos, lambda: ops.gat_aggregate(feat, a_s, a_d, ccsr, 0.2, None, True, 0.4, 99))
            case(tag + "gat_backward." + name, lambda: ops.gat_backward(g_out, feat, st[0], a_s, a_d, st[1], st[2], ccsr, ccsr_src, 0.2, 0.4, 99, st[3], st[4]))
        ops._GAT_POS_STATS, ops._GAT_BWD_EDGE_BUFFER = keep
        yh, w, g_score = rand(n, H, D), rand(H, D), rand(e, H)
        case(tag + "sddmm", lambda: ops.sddmm(feat, yh, ccsr))
        case(tag + "add_score", lambda: ops.add_score(feat, yh, w, ccsr, 0.2))
        for want_w in (False, True):
            case(tag + "add_score_backward.rows_w_%d" % want_w, lambda: ops.add_score_backward(feat, yh, w, g_score, ccsr, n, 0.2, want_w=want_w))
            case(tag + "add_score_backward.cols_w_%d" % want_w, lambda: ops.add_score_backward(yh, feat, w, g_score, ccsr_src, n, 0.2, want_w=want_w))
    sink.close()
    print("ops_call_trace: %d lines -> %s" % (sum(1 for _ in open(path)), path))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else "ops_call_trace.jsonl")
