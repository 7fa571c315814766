/*
 * pgl_amd.h -- C ABI of libpglamd.so: the MI355X (gfx950) message-passing engine that sits
 * behind PGL's Graph.send / recv / send_recv / send_ue_recv / send_uv and pgl.math.segment_*.
 *
 * The reference (PaddlePaddle/PGL 2.2.6) has no plugin registry for this path: the seam is the
 * set of paddle.* tensor ops its Python makes.  Each entry point below
 * replaces one of those call sites; the reference file:line it stands in for is cited on it.
 * INTEGRATION.md shows the ctypes stub a PGL maintainer would add on the reference side.
 *
 * Conventions (all entry points)
 *   - plain pointers + sizes; every pointer is a DEVICE pointer unless it says "host";
 *     no torch / paddle types anywhere in a signature;
 *   - row-major, rows contiguous (last dim fastest), same as paddle/torch default layout;
 *   - the caller owns every buffer, including outputs and scratch: query
 *     pglamd_<op>_workspace_bytes(...) first, allocate, pass `workspace`;
 *     the library never allocates or frees device memory on these paths;
 *   - work is enqueued asynchronously on `stream` (a hipStream_t, NULL = default stream);
 *     no hidden synchronisation unless the entry point says so;
 *   - return 0 on success, a negative PGLAMD_E_* otherwise; pglamd_last_error() gives the
 *     thread-local message;
 *   - index validity (ids < num_nodes) is the caller's contract, exactly as in the reference.
 *
 * "CSR order" below means the order graph_kernel.build_index emits (pgl/graph_kernel.pyx:59-88):
 * edges stably sorted by key u (= dst for adj_dst_index, pgl/graph.py:1319-1328), ascending
 * original edge id within a row.
 */
#ifndef PGL_AMD_H_
#define PGL_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGLAMD_ABI_VERSION 4

/* status codes */
#define PGLAMD_OK 0
#define PGLAMD_E_SHAPE (-1)     /* bad size / unsupported broadcast */
#define PGLAMD_E_DTYPE (-2)     /* dtype not supported by this entry point */
#define PGLAMD_E_RANGE (-3)     /* num_nodes / num_edges beyond the int32 engine range */
#define PGLAMD_E_WORKSPACE (-4) /* workspace NULL or too small */
#define PGLAMD_E_HIP (-5)       /* HIP runtime error (message has hipGetErrorString) */
#define PGLAMD_E_ARG (-6)       /* NULL pointer / bad enum */
#define PGLAMD_E_UNAVAILABLE (-7) /* optional helper library (METIS, RCCL) not present */
#define PGLAMD_E_RCCL (-8)      /* RCCL error (message has ncclGetErrorString) */

/* element types */
#define PGLAMD_F16 0
#define PGLAMD_F32 1
#define PGLAMD_F64 2
#define PGLAMD_I32 3
#define PGLAMD_I64 4
#define PGLAMD_BF16 5

/* reduce_op of send_u_recv / send_ue_recv / segment_* ("sum","mean","max","min") */
#define PGLAMD_SUM 0
#define PGLAMD_MEAN 1
#define PGLAMD_MAX 2
#define PGLAMD_MIN 3

/* message_op of send_ue_recv / send_uv ("add","sub","mul","div") */
#define PGLAMD_ADD 0
#define PGLAMD_SUB 1
#define PGLAMD_MUL 2
#define PGLAMD_DIV 3

int32_t pglamd_abi_version(void);
/* Process-wide TUNING option (tests and experiments; every hot-path choice a caller makes is a per-call argument -- see
 * PGLAMD_AGG_DEAL_CHUNKS -- and the entry points are re-entrant).
 * "csr_onesweep": how pglamd_csr_build sorts.  -1 (default) = by size: one-sweep passes (one histogram of all digits, then ONE kernel per
 * digit with decoupled look-back: 7 launches) for up to 1 M edges, the multi-kernel passes (histogram / scan / scatter per digit: 12
 * launches, XCD-local tile order) above; 0 = always multi-kernel; g >= 1 = always one-sweep with g consecutive tiles per XCD.  The output
 * is bit-identical either way.
 * "slice_front": pglamd_aggregate_sliced's block schedule.  Every XCD walks its hub slice's blocks interleaved with rest-stream blocks
 * over the first `value` per cent of its block sequence and only rest-stream blocks after that; 100 = spread over the whole launch,
 * values above 100 are 100, a negative value restores the built-in default.  The output is bit-identical for every value. */
int32_t pglamd_set_option(const char* name, int64_t value);
const char* pglamd_last_error(void);
/* name of the device the library sees, e.g. "gfx950..." (host string, valid until next call) */
const char* pglamd_device_arch(void);

/* ------------------------------------------------------------------------------------------------
 * K8  CSR build.   Replaces graph_kernel.build_index (pgl/graph_kernel.pyx:59-88) as called by
 * EdgeIndex.from_edges (pgl/utils/edge_index.py:38-58; numpy path :56-57, tensor path :42-54).
 *   u, v            int64 keys / neighbours, element strides u_stride / v_stride (so a column of
 *                   the [E,2] edge array can be passed in place: stride 2)
 *   degree[N] sorted_v[E] sorted_u[E] sorted_eid[E] indptr[N+1]     int64, reference layout,
 *                   bit-identical to build_index (stable by original edge id)
 *   row32[E] col32[E] eid32[E]   optional (NULL to skip) int32 copies of sorted_u / sorted_v /
 *                   sorted_eid that the aggregation kernels read (halves index traffic)
 *   range_flag      optional device int32[1] (caller zeroes it): set to 1 when a key lies outside
 *                   [0, N) or a neighbour id outside [0, 2^31).  Offending keys are clamped to row 0
 *                   so the call itself stays memory-safe; the call is asynchronous, the CALLER
 *                   decides when to read the flag (pgl_amd.ops.csr_build raises ValueError, the
 *                   error pglamd_build_index_host returns as PGLAMD_E_RANGE on the host side).
 * Limits: N < 2^31, E < 2^31 (PGLAMD_E_RANGE otherwise).
 * ---------------------------------------------------------------------------------------------- */
size_t pglamd_csr_build_workspace_bytes(int64_t num_edges, int64_t num_nodes);
int32_t pglamd_csr_build(const int64_t* u, int64_t u_stride, const int64_t* v, int64_t v_stride,
                         int64_t num_edges, int64_t num_nodes, int64_t* degree, int64_t* sorted_v,
                         int64_t* sorted_u, int64_t* sorted_eid, int64_t* indptr, int32_t* row32,
                         int32_t* col32, int32_t* eid32, int32_t* range_flag, void* workspace,
                         size_t workspace_bytes, void* stream);

/* Replaces unique_segment(dst_sorted) = paddle.unique(return_inverse=True)
 * (pgl/utils/helper.py:156-160, cached by Graph.get_segment_ids, pgl/graph.py:1397-1407).
 *   uniq_ind[<=N]   ascending ids of rows with degree > 0 (first *num_uniq entries valid)
 *   segment_ids[E]  dense rank of each CSR-ordered edge's row
 *   num_uniq        device int64[1]                                                              */
size_t pglamd_unique_segment_workspace_bytes(int64_t num_edges, int64_t num_nodes);
int32_t pglamd_unique_segment(const int64_t* degree, const int64_t* sorted_u, int64_t num_edges,
                              int64_t num_nodes, int64_t* uniq_ind, int64_t* segment_ids,
                              int64_t* num_uniq, void* workspace, size_t workspace_bytes,
                              void* stream);

/* strided int64 -> int32 narrowing copy (src/dst columns of the edge array for send_uv) */
int32_t pglamd_narrow_i64(const int64_t* in, int64_t in_stride, int64_t n, int32_t* out,
                          void* stream);

/* ------------------------------------------------------------------------------------------------
 * K1 / K2  aggregation over a CSR-ordered edge list (atomic-free, deterministic).
 * Replaces paddle.geometric.send_u_recv  (pgl/graph.py:859-861, 885-887: Graph.send_recv /
 * send_u_recv) and paddle.geometric.send_ue_recv (pgl/graph.py:929-937: Graph.send_ue_recv):
 *
 *     out[r, j] = dst_scale[r] * REDUCE_{p : row[p]==r}  ( src_scale[col[p]] * x[col[p], xj] (mop) y[yp, yj] )
 *
 *   x          [n_x_rows, dx]   node features, `dtype`
 *   row, col   [E] int32, CSR order (row non-decreasing): destination row / source row per edge
 *   indptr     [n_csr_rows+1] int64 (the reference's indptr)
 *   y          NULL for send_u_recv; else edge features [E, dy] of `dtype` in ORIGINAL edge order
 *              when eid != NULL (yp = eid[p]) or already in CSR order when eid == NULL (yp = p).
 *              Routing note: y = [E, 1] (dy == 1) with eid == NULL, message_op MUL, reduce SUM / MEAN, F32 and rows wider
 *              than 128 bytes is one fp32 value per edge POSITION multiplied into the gathered row -- the library answers it
 *              with the flat kernel's per-position scale slot (the `edge_scale` of pglamd_aggregate_dense: 4 sequential
 *              bytes per edge) instead of the general edge-operand path.  Same result up to the order of one multiplication
 *              (x * y summed, both ways); every accumulate mode and out_rows < n_csr_rows behave as documented below
 *              (tests/test_a7_a9_attention_ops.py::test_abi_edge_operand_e1_mul_reroute_equals_the_general_path).
 *   dx, dy, dout   trailing sizes.  Broadcast rule supported on the fast path: trailing-dim
 *              broadcast only, xj = j / (dout/dx), yj = j / (dout/dy)  (covers [H,D]x[H,1],
 *              [H,D]x[H,D], [D]x[1]); other numpy patterns must be expanded by the caller.
 *   src_scale, dst_scale   optional float32 [n_x_rows] / [out_rows] (NULL = 1): fuses GCN's
 *              symmetric degree normalisation (pgl/nn/conv.py:242,250) into the aggregation;
 *              only for floating dtypes with reduce_op SUM / MEAN.
 *   out        [out_rows, dout]; every row is written exactly once (rows without messages = 0,
 *              as the reference guarantees); out_rows may exceed n_csr_rows (out_size semantics)
 *   reduce_op  PGLAMD_SUM/MEAN/MAX/MIN ; message_op PGLAMD_ADD/SUB/MUL/DIV (ignored if y NULL)
 *   accumulate 0: out is overwritten (rows without edges = 0).  1: rows that receive edges are
 *              combined (+ / max / min) with their existing contents, other rows are untouched --
 *              used to add the halo-source edges after the local-source edges of a partitioned
 *              graph (still deterministic: the two launches are ordered on the stream); not with MEAN.
 *              2: rows that receive edges are OVERWRITTEN, other rows are untouched -- the boundary rows of a
 *              partitioned graph are finished after the halo arrives, on top of the interior rows' launch
 *              (max / min have no identity that an empty first launch could leave behind).
 * ---------------------------------------------------------------------------------------------- */
size_t pglamd_aggregate_workspace_bytes(int64_t num_edges, int64_t dout, int32_t dtype);
int32_t pglamd_aggregate(const void* x, int32_t dtype, int64_t n_x_rows, int64_t dx, const void* y,
                         int64_t dy, const int32_t* eid, const int32_t* row, const int32_t* col,
                         const int64_t* indptr, int64_t num_edges, int64_t n_csr_rows,
                         int64_t out_rows, int64_t dout, int32_t message_op, int32_t reduce_op,
                         const float* src_scale, const float* dst_scale, int32_t accumulate, void* out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* K1x  pglamd_aggregate with what a ROW-PARTITIONED graph needs (pgl_amd/distributed.py; the reference's multi-GPU graph,
 * pgl/graph.py:1475-1553, all-reduces [N, d] partial sums instead).  Every argument shared with pglamd_aggregate means the same;
 * there is no src_scale (a caller scales owned rows before they travel).  The additions:
 *   x2, x_split     second source table: a column id c >= x_split reads row (c - x_split) of x2, c < x_split reads row c of x.
 *                   x = the rows this rank owns, x2 = the rows received from its peers: the boundary rows of a partition
 *                   aggregate straight from the two buffers, nothing is copied into an [owned | halo] matrix first.
 *                   x2 NULL: one table, as pglamd_aggregate.  Same dtype and row length (dx == dout) for both.
 *   zero_indptr     [n_csr_rows+1] or NULL (= indptr).  With accumulate 0 a row r is zero-filled iff
 *                   zero_indptr[r] == zero_indptr[r+1]; rows that are empty in THIS index but not in zero_indptr are left
 *                   untouched.  The interior launch of a partition passes the indptr of ALL local edges: it writes interior
 *                   rows and truly empty rows, the boundary launch (accumulate 2) writes the rest -- every output row is
 *                   written exactly once across the two launches.
 *   max_row_edges   longest row of the index, or 0 when unknown.  No row of <= chunk edges is ever split between waves, so a
 *                   launcher that sees max_row_edges <= its chunk skips the counter reset and the fix-up launch
 *                   (pack indices of a halo plan: every row has one edge).
 *   ldx, ldout      row strides in elements of x (and x2) and of out; 0 = dense (dx / dout).  A launch may read and write a
 *                   COLUMN BLOCK of wider matrices: pass the address of the block's first column, its width as dx / dout and
 *                   the full row length as the stride.  The column-pipelined halo exchange aggregates columns [0, d/2) of the
 *                   received rows while columns [d/2, d) are still on the wire.  (With accumulate 0 a strided output needs
 *                   num_edges > 0: the stand-alone zero-fill of an edgeless index is dense.)
 *   flags           per-call launch choices (ABI 4; replaces the process-wide "xcd_swizzle" option of ABI <= 3, which two threads
 *                   with different plans raced on).  PGLAMD_AGG_DEAL_CHUNKS: the chunks of the destination-sorted edge stream are
 *                   dealt round the 8 XCDs instead of running in contiguous blocks per XCD (the default: neighbouring chunks share
 *                   an L2, which partition- / cluster-ordered graphs use) -- for row orders that correlate with row LENGTH
 *                   (pgl_amd.distributed.HaloPlan(row_order="peers")), where the blocked mapping gives one XCD all the short rows.
 * ---------------------------------------------------------------------------------------------- */
#define PGLAMD_AGG_DEAL_CHUNKS 1
int32_t pglamd_aggregate_ext(const void* x, const void* x2, int64_t x_split, int32_t dtype, int64_t dx,
                             int64_t ldx, const void* y, int64_t dy, const int32_t* eid, const int32_t* row,
                             const int32_t* col, const int64_t* indptr, const int64_t* zero_indptr,
                             int64_t max_row_edges, int64_t num_edges, int64_t n_csr_rows,
                             int64_t out_rows, int64_t dout, int64_t ldout, int32_t message_op, int32_t reduce_op,
                             const float* dst_scale, int32_t accumulate, void* out, void* workspace,
                             size_t workspace_bytes, int32_t flags, void* stream);

/* K1s  fp32 SUM over an index whose long rows' hub edges have been set apart as eight per-XCD slices (pgl_amd.ops.slice_plan):
 *     out[r, :] = SUM_{p : row[p]==r} x[col[p], :]
 * The eight XCDs' private L2s otherwise all hold the same hottest source rows.  The stream (row, col, indptr) is a REST stream --
 * every edge but the hub edges of the long rows, rows and order as in the original index -- followed by slice 0..7: the hub edges
 * of the long rows whose hub has rank % 8 == s, as virtual rows numbered out_rows + s * n_long + i for the i-th long row.  indptr
 * has out_rows + 8 * n_long + 1 entries.  A column id c >= n_x_rows reads hub c - n_x_rows, i.e. row hub_ids[c - n_x_rows] of x; the
 * call gathers those rows into a table in the workspace first.  One launch walks the whole stream: XCD s takes slice s's blocks and
 * an eighth of the rest's, interleaved.  A virtual row's sum goes to a partial table in the workspace, and a last kernel computes
 * out[r] = (((out[r] + P[0, i]) + P[1, i]) ... + P[7, i]) for the long rows r = long_rows[i] -- a fixed order: results repeat bit for bit.
 * A row's terms inside one chunk, and those nine rows, are summed in fp64 and rounded to fp32 once.
 *   blocks / blocks_dev   the same 18 ints in host and in device memory: first 4-chunk block [9] and block count [9] of the rest
 *                         stream and of slice 0..7; together they tile the ceil(ceil(num_edges / chunk) / 4) blocks of the stream
 *   chunk                 edges per chunk the table was made for (a multiple of 8)
 *   d                     even and <= 128, or a multiple of 4 and <= 256; x / out dense [., d], 8-byte (d > 128: 16-byte) aligned
 * ---------------------------------------------------------------------------------------------- */
size_t pglamd_aggregate_sliced_workspace_bytes(int64_t num_edges, int64_t d, int64_t n_hubs, int64_t n_long, int32_t chunk);
int32_t pglamd_aggregate_sliced(const float* x, int64_t n_x_rows, int64_t d, const int32_t* hub_ids, int64_t n_hubs,
                                const int32_t* row, const int32_t* col, const int64_t* indptr, int64_t num_edges,
                                int64_t out_rows, const int32_t* long_rows, int64_t n_long, const int32_t* blocks,
                                const int32_t* blocks_dev, int32_t chunk, float* out, void* workspace,
                                size_t workspace_bytes, void* stream);

/* K1d  aggregation feeding a dense layer inside ONE kernel (row f1: "SpMM -> GEMM epilogue"; GCNConv's
 * send_recv(sum) -> linear -> + bias -> activation, pgl/nn/conv.py:242-254, when input_size <= output_size):
 *     agg[r, :] = dst_scale[r] * REDUCE_{p : row[p]==r} x[col[p], :]            (SUM or MEAN, F32, d_in = 64 or 128)
 *     out[r, :] = act( agg[r, :] @ w + bias )                                    (w [d_in, d_out] row-major, d_out % 16 == 0)
 * Two forms behind this entry (pgl_amd/csrc/aggregate_dense2.hpp says why):
 *   - where w fits in LDS (d_in * d_out * 4 + ring <= 80 KB): persistent workgroups of 8 producer waves + 4 matrix waves; the
 *     producers walk the edges and hand finished rows through a ring in LDS to the matrix waves, which hold w in LDS for the
 *     life of the workgroup and multiply 16 rows at a time with v_mfma_f32_16x16x4_f32;
 *   - otherwise: every wave of the flat aggregation kernel parks its finished rows in a 16-row LDS tile of its own and
 *     multiplies it by w (B operand from memory).
 * fp32 inputs, fp32 accumulation -- the reference's arithmetic up to re-association; only `out` is written: the [n_rows, d_in]
 * intermediate never travels through HBM, and the matrix cores run in the shadow of the row gathers.
 * edge_scale (optional, ABI 2): one fp32 value per edge POSITION of the sorted stream, multiplied into the gathered row
 *     (agg[r] = dst_scale[r] * SUM_p edge_scale[p] * x[col[p]]): GCN's source-side degree norm (pgl/nn/conv.py:242) laid out
 *     along the stream once per graph -- 4 sequential bytes per edge instead of a pass over [N, d_in] per layer.
 * agg_out (optional): the aggregated rows are ALSO stored (training: the weight gradient is agg^T @ d out).
 * act: 0 none, 1 relu.  Rows without edges get act(bias).  Rows longer than a chunk go through the split-row fix-up and get the
 * layer from a small MFMA kernel afterwards.  Deterministic.  w 16-byte aligned for the first form.  Workspace (8-byte aligned):
 * pglamd_aggregate_dense_workspace_bytes.
 * Operand layout: x, agg_out and the workspace are walked in 8-byte lanes -- PGLAMD_E_ARG when one of them is not 8-byte
 * aligned, nothing is written.  w is staged in 16-byte lanes by the first form only; a w below that takes the second form,
 * which reads it one float at a time.  bias, edge_scale, dst_scale and out: one float at a time, 4-byte aligned. */
size_t pglamd_aggregate_dense_workspace_bytes(int64_t num_edges, int64_t d_in, int64_t d_out);
int32_t pglamd_aggregate_dense(const float* x, int64_t d_in, const int32_t* row, const int32_t* col,
                               const int64_t* indptr, int64_t num_edges, int64_t n_csr_rows,
                               int64_t out_rows, int32_t reduce_op, const float* edge_scale,
                               const float* dst_scale, const float* w, const float* bias, int32_t act, int64_t d_out,
                               float* agg_out, float* out, void* workspace, size_t workspace_bytes,
                               void* stream);

/* Gradients that pgl_amd/autograd.py used to compose from [E, d] row gathers (F32; PaddlePaddle implements them inside
 * graph_send_recv_grad / graph_send_ue_recv_grad behind the call sites at pgl/graph.py:834-937).
 *
 * pglamd_winner_grad: d x of send_recv(x, max | min).  The gradient of an output row goes to EVERY message equal to the winner
 * (Paddle's rule):  grad_x[u, j] = sum_{e = (u -> v)} [x[u, j] == out[v, j]] * grad_out[v, j].  One walk of the SRC-sorted
 * stream (src_row / src_col / src_indptr = the src-keyed CSR: row = u, col = v), d <= 256, deterministic.
 *
 * pglamd_edge_operand_grad: d y of send_ue_recv(x, y, message_op, sum | mean) for trailing-dim broadcast operands
 * (y [E, dy], d % dy == 0; the [E, H, 1] case also has pglamd_sddmm):
 *     grad_y[eid[p], jy] = sum_{j in group jy} dst_scale[row[p]] * grad_out[row[p], j] * { 1 | -1 | x[col[p], j] | -x[col[p], j] / y^2 }
 * for ADD | SUB | MUL | DIV; row / col / eid = the dst-sorted CSR (eid NULL: grad_y in CSR order); dst_scale NULL = 1
 * (MEAN: 1 / in-degree); x is needed for MUL / DIV, y (original edge order, like grad_y) for DIV. */
size_t pglamd_winner_grad_workspace_bytes(int64_t num_edges, int64_t d);
int32_t pglamd_winner_grad(const float* grad_out, const float* out, const float* x, int64_t d,
                           const int32_t* src_row, const int32_t* src_col, const int64_t* src_indptr,
                           int64_t num_edges, int64_t n_x_rows, float* grad_x, void* workspace,
                           size_t workspace_bytes, void* stream);
int32_t pglamd_edge_operand_grad(const float* grad_out, const float* x, const float* y,
                                 const float* dst_scale, int64_t d, int64_t dy, const int32_t* row,
                                 const int32_t* col, const int32_t* eid, int64_t num_edges,
                                 int32_t message_op, float* grad_y, void* stream);

/* Measurement hook for the dominant kernel (bench.py roofline leg): between profile_begin and
 * profile_end every launch of the flat aggregation kernel is bracketed by HIP events on its own
 * launch stream; profile_end synchronises them and returns the summed kernel time (host out). */
int32_t pglamd_profile_begin(void);
int32_t pglamd_profile_end(double* total_ms, int64_t* launches);
/* name + template arguments of the flat kernel the last pglamd_aggregate call launched (host string) */
const char* pglamd_profile_last_kernel(void);

/* K1'  un-indexed COO variant (edges in arbitrary order, hardware float atomics; SUM only, F32): what answers
 * paddle.geometric.send_u_recv(x, src, dst) (pgl/graph.py:859-861; Paddle-free fallback pgl/utils/helper.py:163-210) on a SMALL
 * edge list used once, where the launches of a CSR build cost more than the aggregation: |E| * d <= 6.4 M elements (measured on
 * MI355X, profiles/r05/coo.txt: 0.023 vs 0.074 ms at 13 k edges, d = 128; break-even near 50 k edges).  Above that the memory-side
 * read-modify-write of every 512-byte destination row makes it 3-7 x slower than pglamd_csr_build + pglamd_aggregate, which is
 * what pgl_amd.ops.send_u_recv runs there.  Result is order-nondeterministic in the last bits, unlike pglamd_aggregate.  `out`
 * is zero-filled here. */
int32_t pglamd_scatter_add_coo(const float* x, int64_t d, const int32_t* src, const int32_t* dst,
                               int64_t num_edges, int64_t out_rows, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K3  send_uv.  Replaces paddle.geometric.send_uv (pgl/graph.py:964-966):
 *     out[e, j] = x[src[e], j/(dout/dx)] (mop) y[dst[e], j/(dout/dy)]      (original edge order)
 * ---------------------------------------------------------------------------------------------- */
int32_t pglamd_send_uv(const void* x, const void* y, int32_t dtype, int64_t dx, int64_t dy,
                       int64_t dout, const int32_t* src, const int32_t* dst, int64_t num_edges,
                       int32_t message_op, void* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K5  segment reduce.  Replaces paddle.geometric.segment_{sum,mean,max,min}
 * (pgl/math.py:30-178; Message.reduce_*, pgl/message.py:34-105).
 *   data [E, d] of `dtype`; ids [E] sorted non-decreasing, int32 (ids_i64 = 0) or int64 (= 1);
 *   out [n_out_rows, d] with n_out_rows = ids[E-1] + 1 supplied by the caller; rows whose id
 *   never occurs are 0.
 * ---------------------------------------------------------------------------------------------- */
size_t pglamd_segment_reduce_workspace_bytes(int64_t num_rows, int64_t d, int64_t n_out_rows,
                                             int32_t dtype);
int32_t pglamd_segment_reduce(const void* data, int32_t dtype, const void* ids, int32_t ids_i64,
                              int64_t num_rows, int64_t d, int64_t n_out_rows, int32_t reduce_op,
                              void* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K4  segment softmax.  Replaces pgl.math.segment_softmax (pgl/math.py:181-224: segment_max,
 * gather, sub, exp, segment_sum, gather, div) and -- with perm32 = sorted_eid -- the whole of
 * GF.edge_softmax (pgl/nn/functional/graph_op.py:101-123: gather by eid, segment_softmax,
 * scatter back by eid): data and out are only ever addressed in the data's OWN order.
 *   data/out        [num_rows, d] F32 or F64 (out != data)
 *   row32           [num_rows] segment id of the p-th element in SEGMENT-SORTED order (non-decreasing)
 *   perm32          [num_rows] position in `data` of the p-th sorted element, or NULL if data is
 *                   already sorted by segment (pgl.math.segment_softmax)
 *   seg_of_elem32   [num_rows] segment id of data row i (== row32 when perm32 is NULL; the dst
 *                   column of the edge list for edge_softmax by dst)
 *   seg_ptr         [n_seg+1] int64 offsets of each segment in sorted order (the reference's indptr)
 * Arithmetic is the reference's: e = exp(x - max_seg); out = e / sum_seg(e).  Deterministic.
 * ---------------------------------------------------------------------------------------------- */
size_t pglamd_segment_softmax_workspace_bytes(int64_t num_rows, int64_t d, int64_t n_seg, int32_t dtype);
int32_t pglamd_segment_softmax(const void* data, int32_t dtype, int64_t num_rows, int64_t d,
                               const int32_t* row32, const int32_t* perm32,
                               const int32_t* seg_of_elem32, const int64_t* seg_ptr, int64_t n_seg,
                               void* out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K3+K4+K2 fused: the attention aggregation of GATConv (pgl/nn/conv.py:331-339) in ONE pass over
 * the dst-sorted edges, with an online softmax per (row, head):
 *     out[v,h,:] = sum_{e=(u->v)} softmax_v( leaky_relu(attn_src[u,h] + attn_dst[v,h], slope) ) * feature[u,h,:]
 * == send_uv("add") -> leaky_relu -> edge_softmax(by dst) -> send_ue_recv("mul","sum") of the
 * reference, without materialising any [E,H] tensor.  F32.  heads*head_dim <= 256.
 *   feature [N, heads, head_dim], attn_src/attn_dst [N, heads]; row/col/indptr: dst-sorted CSR
 *   out [out_rows, heads, head_dim] (rows without in-edges = 0)
 *   row_max,row_sum  optional [out_rows, heads]: the softmax statistics (max logit, sum of
 *                    exp(logit - max)) from which a backward pass can recompute alpha per edge.
 * Deterministic (no atomics).  Softmax sums are accumulated with rescaling, so alpha differs from
 * the reference's two-pass evaluation only by fp32 rounding (tests: <= 1e-5 relative on out).
 * ---------------------------------------------------------------------------------------------- */
size_t pglamd_gat_aggregate_workspace_bytes(int64_t num_edges, int64_t heads, int64_t head_dim);
/* drop_p in [0,1): attention dropout applied to alpha (pgl/nn/conv.py:337-338): edge e keeps head h with the factor
 * drop_e below and loses it otherwise, out[v,h,:] = sum_e drop_e alpha_e feature[u,h,:] with alpha the UNDROPPED softmax.
 * Nothing is stored: the forward and every backward walk regenerate the factor from (seed, eid, head).  Needs eid (the
 * dst-sorted sorted_eid) when drop_p > 0.  The mask, exactly (all integer arithmetic in uint32, wrapping):
 *     h = seed ^ (uint32(eid) * 0x9E3779B1) ^ (uint32(head) * 0x85EBCA77 + 0xC2B2AE3D)
 *     h ^= h >> 16;  h *= 0x7FEB352D;  h ^= h >> 15;  h *= 0x846CA68B;  h ^= h >> 16
 *     u = float(h >> 8) * 2^-24                                  (exact in fp32: a 24-bit integer times a power of two)
 *     drop_e = u >= drop_p ? 1.f / (1.f - drop_p) : 0            (the compare in fp32; the factor rounded once in fp32)
 *   eid   the ORIGINAL edge id (what eid[] holds at the edge's position), not its position in a sorted stream
 *   head  the head's index inside this launch, 0 .. heads-1 (a caller that sends its heads in groups restarts at 0)
 *   seed  uint32; the Python front end reduces an integer seed modulo 2^32
 * tests/grad_defs.py attention_keep restates it; tests/test_gat_dropout_gpu.py holds the kernels to it bit by bit.
 *   out_pos, sum_pos   optional (both or neither; training): [out_rows, H*D] and [out_rows, H] positive-part statistics
 *                      consumed by pglamd_gat_backward (see there).  Under dropout out_pos carries drop_e, sum_pos does not.
 *   n_csr_rows         rows of the index (indptr has n_csr_rows + 1 entries); out_rows may be smaller (rows >= out_rows are
 *                      walked but never stored) or larger (rows >= n_csr_rows are zero).
 * Operand layout: feature, out and the workspace are walked in lanes of VEC floats, VEC the smallest of 1, 2, 4 with
 * heads * head_dim <= 64 * VEC that divides head_dim and to whose 4 * VEC bytes all three are aligned; PGLAMD_E_SHAPE when there
 * is none (heads * head_dim > 64 with a 4-byte aligned feature), nothing is written.  out_pos: 16-byte aligned (PGLAMD_E_ARG).
 * attn_src, attn_dst, row_max, row_sum, sum_pos: one float at a time.
 */
int32_t pglamd_gat_aggregate(const float* feature, const float* attn_src, const float* attn_dst,
                             int64_t heads, int64_t head_dim, float negative_slope, float drop_p,
                             uint32_t seed, const int32_t* row, const int32_t* col,
                             const int32_t* eid, const int64_t* indptr, int64_t num_edges,
                             int64_t n_csr_rows, int64_t out_rows, float* out, float* row_max,
                             float* row_sum, float* out_pos, float* sum_pos, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Backward of pglamd_gat_aggregate (row "next" f1: fused backward), alpha recomputed per edge from
 * the forward's statistics; nothing of size [E,H] or [E,H,D] is materialised:
 *   grad_feature[u,h,:] = sum_{e=(u->v)} drop_e alpha_e grad_out[v,h,:]
 *   grad_attn_src[u,h]  = sum_{e=(u->v)} d pre_e          (both from ONE walk of the src-sorted CSR)
 *   grad_attn_dst[v,h]  = sum_{e=(u->v)} d pre_e          (one walk of the dst-sorted CSR)
 *   grad_pre (optional) : when non-NULL the src-sorted walk also writes d pre_e to grad_pre[E,H], row p = the p-th edge of
 *                         the SRC-SORTED stream (src_row / src_col), and the dst-sorted walk is skipped; the caller then
 *                         takes grad_attn_dst as the segment sum of grad_pre by destination (pglamd_aggregate over the
 *                         dst-sorted CSR with col = the src-sorted position of each edge): 1.3 ms faster at C3 for
 *                         4*E*H bytes of scratch.  grad_attn_dst may be NULL in that case.
 *   out_pos, sum_pos (optional, from pglamd_gat_aggregate): the forward's positive-part statistics -- out_pos[v,h,:] = the part
 *                         of out[v] contributed by edges with pre_e > 0, sum_pos[v,h] = their softmax mass.  With them
 *                         grad_attn_dst[v,h] = <g,out_pos> + slope <g,out - out_pos> - t (sum_pos + slope (1 - sum_pos)) is
 *                         evaluated per (node, head) inside the pack kernel: no per-edge buffer (grad_pre is ignored) and
 *                         no dst-sorted walk -- the round-2 default of pgl_amd (0.8 ms less at C3 for one more [N,H*D]
 *                         tensor kept from the forward).
 *   d pre_e = alpha_e (drop_e <grad_out[v,h,:], feature[u,h,:]> - t[v,h]) * leaky_relu'(attn_src[u,h] + attn_dst[v,h])
 *   t[v,h]  = sum_d grad_out[v,h,d] * out[v,h,d]  (out = the forward's output; computed here).
 *   dst_* / src_*  the dst-sorted and src-sorted CSRs (int32 row / col / eid, int64 indptr).
 * Replaces the backward of the four-op composition at pgl/nn/conv.py:331-339 (send_uv -> leaky_relu ->
 * edge_softmax -> send_ue_recv).  Workspace (256-byte aligned): pglamd_gat_backward_workspace_bytes.  Same shape
 * limits as the forward, and head_dim / VEC must be a power of two (per-head dot products are shuffle reductions).
 * Operand layout: feature, grad_out and grad_feature in lanes of VEC floats chosen as in the forward from THEIR addresses;
 * grad_out and out also in 16-byte lanes by the kernel that packs t[v,h]: both 16-byte aligned at every width; the workspace
 * (which holds the packed 16-byte records) 256-byte aligned -- PGLAMD_E_SHAPE otherwise; out_pos 16-byte aligned (PGLAMD_E_ARG).
 * Nothing is written on a refusal.  attn_*, row_max, row_sum, sum_pos, grad_attn_*, grad_pre: one float at a time. */
size_t pglamd_gat_backward_workspace_bytes(int64_t num_edges, int64_t num_nodes, int64_t heads,
                                           int64_t head_dim);
int32_t pglamd_gat_backward(const float* grad_out, const float* feature, const float* attn_src,
                            const float* attn_dst, const float* row_max, const float* row_sum,
                            const float* out, int64_t heads, int64_t head_dim, float negative_slope,
                            float drop_p, uint32_t seed, const int32_t* dst_row,
                            const int32_t* dst_col, const int32_t* dst_eid, const int64_t* dst_indptr,
                            const int32_t* src_row, const int32_t* src_col, const int32_t* src_eid,
                            const int64_t* src_indptr, int64_t num_edges, int64_t num_nodes,
                            float* grad_feature, float* grad_attn_src, float* grad_attn_dst,
                            float* grad_pre, const float* out_pos, const float* sum_pos,
                            void* workspace, size_t workspace_bytes, void* stream);

/* The two entries above on 16-bit rows: the attention aggregation of GATConv (pgl/nn/conv.py:331-339) and its backward with
 * feature, out, out_pos, grad_out and grad_feature STORED as T = fp16 (dtype PGLAMD_F16) or bf16 (PGLAMD_BF16) -- the void*
 * parameters -- and everything else as in the fp32 entries, argument by argument: attn_src, attn_dst, row_max, row_sum, sum_pos,
 * grad_attn_src, grad_attn_dst and grad_pre are fp32, and so is every accumulator, the packed per-(node, head) records and the
 * split-row partials.  A stored value is converted to fp32 when it is loaded; a result is rounded to T once, to nearest even, on
 * its final store (a row split over chunks: after its fp32 partials are merged).  Lane width, edge order, chunk size and merge order
 * are the fp32 entries', so a call returns the fp32 entry's result on the up-cast operands, rounded to T -- bit for bit
 * (tests/test_gat16_gpu.py) -- and the fp32 outputs with the fp32 entry's bits.  Dropout mask: as defined above.
 * Workspace: the fp32 entries' sizes, pglamd_gat_aggregate_workspace_bytes and pglamd_gat_backward_workspace_bytes (the partials
 * are fp32 whatever T is).
 * Operand layout, in bytes of T (sizeof(T) = 2): forward -- feature and out in lanes of VEC elements, VEC the smallest of 1, 2, 4
 * with heads * head_dim <= 64 * VEC that divides head_dim and to whose sizeof(T) * VEC bytes both are aligned; the workspace
 * 16-byte aligned; PGLAMD_E_SHAPE when there is no such VEC; out_pos aligned to 4 * sizeof(T) = 8 bytes (PGLAMD_E_ARG).  Backward
 * -- feature, grad_out and grad_feature in lanes of VEC elements chosen the same way from THEIR addresses, with head_dim / VEC a
 * power of two; grad_out and out also in groups of four elements (8 bytes) by the kernel that packs t[v,h]: both 8-byte aligned at
 * every width; the workspace 256-byte aligned -- PGLAMD_E_SHAPE otherwise; out_pos 8-byte aligned (PGLAMD_E_ARG).
 * PGLAMD_E_ARG for any other dtype, PGLAMD_E_WORKSPACE for a workspace that is too small.  Nothing is written on a refusal. */
int32_t pglamd_gat_aggregate_16(int32_t dtype, const void* feature, const float* attn_src,
                                const float* attn_dst, int64_t heads, int64_t head_dim,
                                float negative_slope, float drop_p, uint32_t seed, const int32_t* row,
                                const int32_t* col, const int32_t* eid, const int64_t* indptr,
                                int64_t num_edges, int64_t n_csr_rows, int64_t out_rows, void* out,
                                float* row_max, float* row_sum, void* out_pos, float* sum_pos,
                                void* workspace, size_t workspace_bytes, void* stream);
int32_t pglamd_gat_backward_16(int32_t dtype, const void* grad_out, const void* feature,
                               const float* attn_src, const float* attn_dst, const float* row_max,
                               const float* row_sum, const void* out, int64_t heads, int64_t head_dim,
                               float negative_slope, float drop_p, uint32_t seed, const int32_t* dst_row,
                               const int32_t* dst_col, const int32_t* dst_eid, const int64_t* dst_indptr,
                               const int32_t* src_row, const int32_t* src_col, const int32_t* src_eid,
                               const int64_t* src_indptr, int64_t num_edges, int64_t num_nodes,
                               void* grad_feature, float* grad_attn_src, float* grad_attn_dst,
                               float* grad_pre, const void* out_pos, const float* sum_pos,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Scaled dot-product attention over the graph (TransformerConv called without edge features, pgl/nn/conv.py:796-847; with them:
 * pglamd_dot_attention_edge below) in ONE pass over
 * the dst-sorted edges, with an online softmax per (row, head):
 *     s_e,h      = scale * <q[v,h,:], k[u,h,:]>                         e = (u -> v)
 *     alpha_e,h  = softmax over the in-edges of v of s_e,h
 *     out[v,h,:] = sum_{e=(u->v)} drop_e alpha_e,h v[u,h,:]
 * == sddmm -> edge_softmax(by dst) -> dropout -> send_ue_recv("mul","sum"), without materialising any [E,H] tensor.  F32,
 * heads*head_dim <= 256, head_dim / VEC a power of two (per-head dot products are lane-group sums).
 *   q, k, v [num_nodes, heads, head_dim]; row/col/eid/indptr: the dst-sorted CSR over num_nodes rows
 *   out [num_nodes, heads, head_dim]; a row without in-edges is 0, and so are its statistics
 *   row_max,row_sum  optional (both or neither) [num_nodes, heads]: max score and sum of exp(score - max), from which
 *                    pglamd_dot_attention_backward recomputes alpha per edge
 *   drop_p in [0,1), seed: attention dropout, drop_e EXACTLY as defined next to pglamd_gat_aggregate above (the same hash of
 *                    (seed, original edge id, head)); needs eid when drop_p > 0 (PGLAMD_E_ARG without it)
 * Deterministic (no atomic sums; a row split over chunks is merged in a fixed order).  num_edges == 0: out and the statistics
 * are zeroed; num_nodes == 0: nothing is done.
 * Operand layout: q, k, v, out and the workspace are walked in lanes of VEC floats, VEC the smallest of 1, 2, 4 with
 * heads * head_dim <= 64 * VEC that divides head_dim, leaves head_dim / VEC a power of two and to whose 4 * VEC bytes all five
 * are aligned; PGLAMD_E_SHAPE when there is none, nothing is written.  row_max, row_sum: one float at a time.
 * Workspace: pglamd_dot_attention_workspace_bytes (PGLAMD_E_WORKSPACE when smaller).
 * ---------------------------------------------------------------------------------------------- */
size_t pglamd_dot_attention_workspace_bytes(int64_t num_edges, int64_t heads, int64_t head_dim);
int32_t pglamd_dot_attention(const float* q, const float* k, const float* v, int64_t heads,
                             int64_t head_dim, float scale, float drop_p, uint32_t seed,
                             const int32_t* row, const int32_t* col, const int32_t* eid,
                             const int64_t* indptr, int64_t num_edges, int64_t num_nodes, float* out,
                             float* row_max, float* row_sum, void* workspace, size_t workspace_bytes,
                             void* stream);

/* Backward of pglamd_dot_attention, alpha_e = exp(s_e - row_max[v]) / row_sum[v] recomputed per edge from the forward's
 * statistics; nothing of size [E,H] or [E,H,D] is materialised.  With g = grad_out, t[v,h] = <g[v,h,:], out[v,h,:]> (computed
 * here) and ds_e = alpha_e (drop_e <g[v,h,:], v[u,h,:]> - t[v,h]):
 *   grad_q[v,h,:] = scale * sum_{e=(u->v)} ds_e k[u,h,:]                (one walk of the dst-sorted CSR)
 *   grad_k[u,h,:] = scale * sum_{e=(u->v)} ds_e q[v,h,:]                (one walk of the src-sorted CSR, which also gives)
 *   grad_v[u,h,:] =         sum_{e=(u->v)} drop_e alpha_e g[v,h,:]
 *   out, row_max, row_sum: what the forward returned; drop_p, seed, scale: what it ran with (drop_e as in the forward; both eid
 *   arrays are needed when drop_p > 0, PGLAMD_E_ARG without them).  dst_* / src_*: the dst-sorted and src-sorted CSRs.
 * Deterministic.  num_edges == 0: the three gradients are zeroed; num_nodes == 0: nothing is done.
 * Operand layout: grad_out, q, k, v and the three gradients in lanes of VEC floats chosen as in the forward from THEIR
 * addresses; grad_out and out also in 16-byte lanes by the kernel that packs t[v,h] when head_dim % 4 == 0; the workspace (which
 * holds the packed 16-byte records) 256-byte aligned -- PGLAMD_E_SHAPE otherwise, nothing is written.  row_max, row_sum: one
 * float at a time.  Workspace: pglamd_dot_attention_backward_workspace_bytes (PGLAMD_E_WORKSPACE when smaller). */
size_t pglamd_dot_attention_backward_workspace_bytes(int64_t num_edges, int64_t num_nodes,
                                                     int64_t heads, int64_t head_dim);
int32_t pglamd_dot_attention_backward(const float* grad_out, const float* q, const float* k,
                                      const float* v, const float* out, const float* row_max,
                                      const float* row_sum, int64_t heads, int64_t head_dim,
                                      float scale, float drop_p, uint32_t seed,
                                      const int32_t* dst_row, const int32_t* dst_col,
                                      const int32_t* dst_eid, const int64_t* dst_indptr,
                                      const int32_t* src_row, const int32_t* src_col,
                                      const int32_t* src_eid, const int64_t* src_indptr,
                                      int64_t num_edges, int64_t num_nodes, float* grad_q,
                                      float* grad_k, float* grad_v, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * pglamd_dot_attention with a per-edge feature added to the key and to the value (TransformerConv with edge_feat, the message
 * function of pgl/nn/conv.py:808-815), the same single pass:
 *     s_e,h      = scale * <q[v,h,:], k[u,h,:] + ef[e,h,:]>             e = (u -> v)
 *     alpha_e,h  = softmax over the in-edges of v of s_e,h
 *     out[v,h,:] = sum_{e=(u->v)} drop_e alpha_e,h (v[u,h,:] + ef[e,h,:])          a row without in-edges is 0
 *   edge_feat [num_edges, heads, head_dim]: position p of the stream reads row eid[p] (eid NULL: row p) -- for the index of a
 *                    graph, original edge order.  Required when num_edges > 0 (PGLAMD_E_ARG without it).
 * Every other argument, the statistics, dropout (eid is needed when drop_p > 0), num_edges == 0 / num_nodes == 0, determinism and
 * every error as pglamd_dot_attention; edge_feat counts among the operands whose alignment chooses VEC.  The workspace is
 * pglamd_dot_attention's (the partials hold the same columns).
 *
 * pglamd_dot_attention_edge_backward: with g = grad_out, t[v,h] = <g[v,h,:], out[v,h,:]>, w_e = drop_e alpha_e and
 * ds_e = alpha_e (drop_e <g[v,h,:], v[u,h,:] + ef[e,h,:]> - t[v,h]):
 *   grad_q[v,h,:]         = scale * sum_{e=(u->v)} ds_e (k[u,h,:] + ef[e,h,:])     (the walk of the dst-sorted CSR)
 *   grad_k[u,h,:]         = scale * sum_{e=(u->v)} ds_e q[v,h,:]                   (the walk of the src-sorted CSR, which also gives)
 *   grad_v[u,h,:]         =         sum_{e=(u->v)} w_e g[v,h,:]
 *   grad_edge_feat[e,h,:] = scale * ds_e q[v,h,:] + w_e g[v,h,:]                   edge e's own term of grad_k[u] + grad_v[u]
 *   grad_edge_feat [num_edges, heads, head_dim] or NULL (not wanted: nothing is stored): one row per edge, addressed through
 *   src_eid as edge_feat is (src_eid NULL: the position), each written exactly once by a plain store -- no atomics, deterministic.
 *   Both walks read edge_feat through their own eid array, so dst_eid and src_eid must name the same rows for the same edge.
 * Every other argument and error as pglamd_dot_attention_backward; edge_feat and grad_edge_feat count among the operands whose
 * alignment chooses VEC.  num_edges == 0: the three node gradients are zeroed (grad_edge_feat has no rows).  Workspace:
 * pglamd_dot_attention_edge_backward_workspace_bytes (= pglamd_dot_attention_backward_workspace_bytes).
 * ---------------------------------------------------------------------------------------------- */
size_t pglamd_dot_attention_edge_workspace_bytes(int64_t num_edges, int64_t heads, int64_t head_dim);
int32_t pglamd_dot_attention_edge(const float* q, const float* k, const float* v,
                                  const float* edge_feat, int64_t heads, int64_t head_dim,
                                  float scale, float drop_p, uint32_t seed, const int32_t* row,
                                  const int32_t* col, const int32_t* eid, const int64_t* indptr,
                                  int64_t num_edges, int64_t num_nodes, float* out, float* row_max,
                                  float* row_sum, void* workspace, size_t workspace_bytes,
                                  void* stream);
size_t pglamd_dot_attention_edge_backward_workspace_bytes(int64_t num_edges, int64_t num_nodes,
                                                          int64_t heads, int64_t head_dim);
int32_t pglamd_dot_attention_edge_backward(const float* grad_out, const float* q, const float* k,
                                           const float* v, const float* edge_feat, const float* out,
                                           const float* row_max, const float* row_sum,
                                           int64_t heads, int64_t head_dim, float scale,
                                           float drop_p, uint32_t seed, const int32_t* dst_row,
                                           const int32_t* dst_col, const int32_t* dst_eid,
                                           const int64_t* dst_indptr, const int32_t* src_row,
                                           const int32_t* src_col, const int32_t* src_eid,
                                           const int64_t* src_indptr, int64_t num_edges,
                                           int64_t num_nodes, float* grad_q, float* grad_k,
                                           float* grad_v, float* grad_edge_feat, void* workspace,
                                           size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * GATv2's attention over the graph (GATv2Conv, pgl/nn/conv.py:419-430; PGL uses ONE projection for score and value) in ONE pass
 * over the dst-sorted edges, with an online softmax per (row, head):
 *     z_e,h,d    = x_src[u,h,d] + x_dst[v,h,d]                          e = (u -> v)
 *     s_e,h      = sum_d attn[h,d] * leaky_relu(z_e,h,d; negative_slope)
 *     alpha_e,h  = softmax over the in-edges of v of s_e,h
 *     out[v,h,:] = sum_{e=(u->v)} drop_e alpha_e,h x_src[u,h,:]
 * == send_uv(add) -> leaky_relu -> (. * attn).sum(-1) -> edge_softmax(by dst) -> dropout -> send_ue_recv("mul","sum"), without
 * materialising any [E,H] or [E,H,D] tensor; every edge gathers x_src[u] once, for the score and for the value.  F32,
 * heads*head_dim <= 256, head_dim / VEC a power of two (per-head sums are lane-group sums).
 *   x_src, x_dst [num_nodes, heads, head_dim] (the layer passes one tensor twice); attn [heads, head_dim];
 *   row/col/eid/indptr: the dst-sorted CSR over num_nodes rows
 *   out [num_nodes, heads, head_dim]; a row without in-edges is 0, and so are its statistics
 *   row_max,row_sum  optional (both or neither) [num_nodes, heads]: max score and sum of exp(score - max), from which
 *                    pglamd_gatv2_attention_backward recomputes alpha per edge
 *   drop_p in [0,1), seed: attention dropout, drop_e EXACTLY as defined next to pglamd_gat_aggregate above (the same hash of
 *                    (seed, original edge id, head)); needs eid when drop_p > 0 (PGLAMD_E_ARG without it)
 * Deterministic (no atomic sums; a row split over chunks is merged in a fixed order).  num_edges == 0: out and the statistics
 * are zeroed; num_nodes == 0: nothing is done.
 * Operand layout: x_src, x_dst, attn, out and the workspace are walked in lanes of VEC floats, VEC the smallest of 1, 2, 4 with
 * heads * head_dim <= 64 * VEC that divides head_dim, leaves head_dim / VEC a power of two and to whose 4 * VEC bytes all five
 * are aligned; PGLAMD_E_SHAPE when there is none, nothing is written.  row_max, row_sum: one float at a time.
 * Workspace: pglamd_gatv2_attention_workspace_bytes (PGLAMD_E_WORKSPACE when smaller).
 * ---------------------------------------------------------------------------------------------- */
size_t pglamd_gatv2_attention_workspace_bytes(int64_t num_edges, int64_t heads, int64_t head_dim);
int32_t pglamd_gatv2_attention(const float* x_src, const float* x_dst, const float* attn,
                               int64_t heads, int64_t head_dim, float negative_slope, float drop_p,
                               uint32_t seed, const int32_t* row, const int32_t* col,
                               const int32_t* eid, const int64_t* indptr, int64_t num_edges,
                               int64_t num_nodes, float* out, float* row_max, float* row_sum,
                               void* workspace, size_t workspace_bytes, void* stream);

/* Backward of pglamd_gatv2_attention, alpha_e = exp(s_e - row_max[v]) / row_sum[v] recomputed per edge from the forward's
 * statistics; nothing of size [E,H] or [E,H,D] is materialised.  With g = grad_out, t[v,h] = <g[v,h,:], out[v,h,:]> (computed
 * here), T_e = <g[v,h,:], x_src[u,h,:]>, ds_e = alpha_e (drop_e T_e - t[v,h]) and L' = leaky_relu' (negative_slope at z == 0, as
 * pglamd_add_score_backward and torch take it):
 *   grad_x_dst[v,h,d] = sum_{e=(u->v)} ds_e attn[h,d] L'(z_e,h,d)                            (one walk of the dst-sorted CSR)
 *   grad_attn[h,d]    = sum_e ds_e leaky_relu(z_e,h,d)     (the same walk: one partial per chunk of edges, the partials summed
 *                                                            in a fixed order by a reduce kernel)
 *   grad_x_src[u,h,d] = sum_{e=(u->v)} drop_e alpha_e g[v,h,d] + ds_e attn[h,d] L'(z_e,h,d)  (one walk of the src-sorted CSR)
 *   out, row_max, row_sum: what the forward returned; drop_p, seed, negative_slope: what it ran with (drop_e as in the forward;
 *   both eid arrays are needed when drop_p > 0, PGLAMD_E_ARG without them).  dst_* / src_*: the dst-sorted and src-sorted CSRs.
 *   When x_src and x_dst are one tensor its gradient is grad_x_src + grad_x_dst (the caller adds them).
 * Deterministic, grad_attn included.  num_edges == 0: the three gradients are zeroed; num_nodes == 0: grad_attn is zeroed.
 * Operand layout: grad_out, x_src, x_dst, attn and the two row gradients in lanes of VEC floats chosen as in the forward from
 * THEIR addresses; grad_out and out also in 16-byte lanes by the kernel that packs t[v,h] when head_dim % 4 == 0; the workspace
 * (which holds the packed 16-byte records) 256-byte aligned -- PGLAMD_E_SHAPE otherwise, nothing is written.  row_max, row_sum,
 * grad_attn: one float at a time.  Workspace: pglamd_gatv2_attention_backward_workspace_bytes (PGLAMD_E_WORKSPACE when smaller). */
size_t pglamd_gatv2_attention_backward_workspace_bytes(int64_t num_edges, int64_t num_nodes,
                                                       int64_t heads, int64_t head_dim);
int32_t pglamd_gatv2_attention_backward(const float* grad_out, const float* x_src,
                                        const float* x_dst, const float* attn, const float* out,
                                        const float* row_max, const float* row_sum, int64_t heads,
                                        int64_t head_dim, float negative_slope, float drop_p,
                                        uint32_t seed, const int32_t* dst_row, const int32_t* dst_col,
                                        const int32_t* dst_eid, const int64_t* dst_indptr,
                                        const int32_t* src_row, const int32_t* src_col,
                                        const int32_t* src_eid, const int64_t* src_indptr,
                                        int64_t num_edges, int64_t num_nodes, float* grad_x_src,
                                        float* grad_x_dst, float* grad_attn, void* workspace,
                                        size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FAGCN's frequency-adaptive attention over the graph (FAConv, pgl/nn/conv.py:1306-1339: the gate
 * tanh(Linear([h_u ; h_v])) * d_u * d_v, dropout, the weighted sum) in ONE pass over the dst-sorted edges.  The gate is signed and
 * has no softmax, so there are no row statistics:
 *     t_e,h      = tanh(p_src[u,h] + p_dst[v,h])                        e = (u -> v)
 *     w_e,h      = t_e,h * s_src[u] * s_dst[v]
 *     out[v,h,:] = sum_{e=(u->v)} drop_e w_e,h x[u,h,:]                 a row without in-edges is 0
 * == send_uv(add) -> tanh -> * send_uv(mul) -> dropout -> send_ue_recv("mul","sum") without any [E,H] tensor.  F32, heads*head_dim
 * <= 256, head_dim / VEC a power of two.  tanh is the device library's tanhf.
 *   x [num_nodes, heads, head_dim]; p_src, p_dst [num_nodes, heads]: the two halves of the gate's pre-activation (the layer:
 *   p_src = x . w[:hs] + b, p_dst = x . w[hs:]); s_src, s_dst [num_nodes] or NULL (= 1): constant scales, the layer's degree norms
 *   row/col/eid/indptr: the dst-sorted CSR over num_nodes rows;  out [num_nodes, heads, head_dim]
 *   drop_p in [0,1), seed: attention dropout, drop_e EXACTLY as defined next to pglamd_gat_aggregate above (the same hash of
 *                    (seed, original edge id, head)); needs eid when drop_p > 0 (PGLAMD_E_ARG without it)
 * Deterministic (no atomic sums; a row split over chunks is added up in chunk order).  num_edges == 0: out is zeroed;
 * num_nodes == 0: nothing is done.
 * Operand layout: x, out and the workspace are walked in lanes of VEC floats, VEC the smallest of 1, 2, 4 with heads * head_dim
 * <= 64 * VEC that divides head_dim, leaves head_dim / VEC a power of two and to whose 4 * VEC bytes all three are aligned;
 * PGLAMD_E_SHAPE when there is none, nothing is written.  p_src, p_dst, s_src, s_dst: one float at a time.
 * Workspace: pglamd_fa_aggregate_workspace_bytes (PGLAMD_E_WORKSPACE when smaller).
 * ---------------------------------------------------------------------------------------------- */
size_t pglamd_fa_aggregate_workspace_bytes(int64_t num_edges, int64_t heads, int64_t head_dim);
int32_t pglamd_fa_aggregate(const float* x, const float* p_src, const float* p_dst,
                            const float* s_src, const float* s_dst, int64_t heads, int64_t head_dim,
                            float drop_p, uint32_t seed, const int32_t* row, const int32_t* col,
                            const int32_t* eid, const int64_t* indptr, int64_t num_edges,
                            int64_t num_nodes, float* out, void* workspace, size_t workspace_bytes,
                            void* stream);

/* Backward of pglamd_fa_aggregate, one walk of the SRC-sorted CSR (row = u; FAConv, pgl/nn/conv.py:1306-1339).  With g = grad_out,
 * c_e,h = drop_e <g[v,h,:], x[u,h,:]> and r_e,h = c_e,h s_src[u] s_dst[v] (1 - t_e,h^2):
 *   grad_x[u,h,:]    = sum_{e=(u->v)} drop_e w_e,h g[v,h,:]
 *   grad_p_src[u,h]  = sum_{e=(u->v)} r_e,h
 *   grad_edge[p,h]   = r_e,h of the edge at position p of THIS (src-sorted) stream, each written once by a plain store;
 *                      grad_p_dst[v,h] = sum_{e=(u->v)} r_e,h is the caller's sum of these rows by destination
 *   grad_x [num_nodes, heads, head_dim] or NULL (not wanted: not stored); grad_p_src [num_nodes, heads] or NULL (then neither it
 *   nor grad_edge is formed; grad_edge without grad_p_src and a call that wants nothing are PGLAMD_E_ARG); grad_edge [num_edges,
 *   heads] or NULL.  Whatever is asked for has the same bits whatever else is.  s_src, s_dst take no gradient.
 *   drop_p, seed: what the forward ran with (src_eid is needed when drop_p > 0, PGLAMD_E_ARG without it).
 * Deterministic.  num_edges == 0: grad_x and grad_p_src are zeroed; num_nodes == 0: nothing is done.
 * Operand layout: grad_out, x, grad_x and the workspace in lanes of VEC floats chosen as in the forward from THEIR addresses
 * (PGLAMD_E_SHAPE when no width fits, nothing is written); everything else one float at a time.
 * Workspace: pglamd_fa_backward_workspace_bytes (PGLAMD_E_WORKSPACE when smaller). */
size_t pglamd_fa_backward_workspace_bytes(int64_t num_edges, int64_t heads, int64_t head_dim);
int32_t pglamd_fa_backward(const float* grad_out, const float* x, const float* p_src,
                           const float* p_dst, const float* s_src, const float* s_dst, int64_t heads,
                           int64_t head_dim, float drop_p, uint32_t seed, const int32_t* src_row,
                           const int32_t* src_col, const int32_t* src_eid, const int64_t* src_indptr,
                           int64_t num_edges, int64_t num_nodes, float* grad_x, float* grad_p_src,
                           float* grad_edge, void* workspace, size_t workspace_bytes, void* stream);

/* Additive attention score over a sorted edge stream (GATv2Conv, pgl/nn/conv.py:421-424: send_uv(f, f, "add") ->
 * leaky_relu -> (alpha * attn).sum(-1), which materialises two [E,H,D] tensors):
 *   out[eid[p], h] = sum_d w[h,d] * leaky_relu( x_by_col[col[p],h,d] + y_by_row[row[p],h,d] )      (eid NULL: out[p,h])
 * F32, heads*head_dim <= 256, head_dim/VEC a power of two.
 * Operand layout: x_by_col, y_by_row and w in lanes of VEC floats (chosen as in pglamd_gat_aggregate from these three
 * addresses; PGLAMD_E_SHAPE when no width fits, nothing is written); out one float at a time. */
int32_t pglamd_add_score(const float* x_by_col, const float* y_by_row, const float* w, int64_t heads,
                         int64_t head_dim, float negative_slope, const int32_t* row, const int32_t* col,
                         const int32_t* eid, int64_t num_edges, float* out, void* stream);

/* Backward of pglamd_add_score w.r.t. the ROW node's operand and (optionally) w, one walk of the sorted stream:
 *   grad_rows[r,h,d]          = sum_{p in row r} grad_score[gi_p,h] * w[h,d] * leaky_relu'(x_by_col[col_p] + y_by_row[r])
 *   grad_w_partials[c, h*D+d] = sum_{p in chunk c} grad_score[gi_p,h] * leaky_relu(x_by_col[col_p] + y_by_row[r])
 * with gi_p = eid[p] (p when eid is NULL) and c over pglamd_add_score_chunks(num_edges) chunks (the caller sums the
 * partials over c; NULL skips them).  The gradient w.r.t. the COLUMN node's operand is the same call on the transposed
 * index with the two operands swapped.  Workspace: pglamd_gat_aggregate_workspace_bytes.
 * Operand layout: x_by_col, y_by_row and grad_rows in lanes of VEC floats (chosen from these three addresses); w, the workspace
 * and grad_w_partials 16-byte aligned at every width -- PGLAMD_E_SHAPE otherwise, nothing is written.  grad_score: one float
 * at a time. */
int64_t pglamd_add_score_chunks(int64_t num_edges);
int32_t pglamd_add_score_backward(const float* x_by_col, const float* y_by_row, const float* w,
                                  const float* grad_score, int64_t heads, int64_t head_dim,
                                  float negative_slope, const int32_t* row, const int32_t* col,
                                  const int32_t* eid, const int64_t* indptr, int64_t num_edges,
                                  int64_t num_rows, float* grad_rows, float* grad_w_partials,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* SDDMM over a sorted edge stream:  out[eid[p], h] = < x_by_col[col[p], h, :], y_by_row[row[p], h, :] >
 * (eid NULL: out[p, h]).  With (row, col, eid) = the dst-sorted CSR, x = node features and
 * y = the incoming gradient this is d loss / d edge_feature of Graph.send_ue_recv(x, e, "mul", "sum")
 * for e of shape [E, H, 1] (pgl/graph.py:929-937 backward) without materialising [E,H,D].  F32,
 * heads*head_dim <= 256, head_dim/VEC a power of two.
 * Operand layout: x_by_col and y_by_row in lanes of VEC floats (chosen as in pglamd_gat_aggregate from these two addresses;
 * PGLAMD_E_SHAPE when no width fits, nothing is written); out one float at a time. */
int32_t pglamd_sddmm(const float* x_by_col, const float* y_by_row, int64_t heads, int64_t head_dim,
                     const int32_t* row, const int32_t* col, const int32_t* eid, int64_t num_edges,
                     float* out, void* stream);

/* out[i] = in[0] + ... + in[i-1] (int64; out may alias in).  The prefix sums the reference takes with paddle.cumsum
 * (pgl/utils/edge_index.py:54 indptr from degrees; the offsets of a sampled block's neighbour lists, pgl/sampling/sage.py:144-147)
 * as three small in-tree kernels (csrc/scan.hpp) -- no library primitive sits on the mini-batch path. */
size_t pglamd_exclusive_scan_i64_workspace_bytes(int64_t n);
int32_t pglamd_exclusive_scan_i64(const int64_t* in, int64_t n, int64_t* out, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* K4'  segment boundaries from sorted ids: seg_ptr[n_seg+1] (int64), n_seg = ids[E-1]+1 given by
 * the caller.  Used when segment_softmax is called with raw ids (pgl.math API). */
int32_t pglamd_seg_ptr_from_ids(const void* ids, int32_t ids_i64, int64_t num_rows, int64_t n_seg,
                                int64_t* seg_ptr, void* stream);

/* ------------------------------------------------------------------------------------------------
 * K6 / K7  row gather / scatter.  Replace paddle.gather (pgl/utils/op.py:45 read_rows / RowReader,
 * pgl/message.py:157 edge_expand, pgl/graph.py:822) and paddle.scatter(overwrite=True)
 * (pgl/graph.py:828-830 recv epilogue).  index int32 (index_i64 = 0) or int64 (= 1).
 *   gather : out[i, :] = x[index[i], :]          out [n_index, d]
 *   scatter: out[index[i], :] = x[i, :]          (indices unique; out pre-initialised by caller)
 * elem_bytes = size of one element (1,2,4,8): these are pure byte moves.
 * ---------------------------------------------------------------------------------------------- */
int32_t pglamd_gather_rows(const void* x, int64_t d, int32_t elem_bytes, const void* index,
                           int32_t index_i64, int64_t n_index, void* out, void* stream);
int32_t pglamd_scatter_rows(const void* x, int64_t d, int32_t elem_bytes, const void* index,
                            int32_t index_i64, int64_t n_index, void* out, void* stream);

/* K6w  row gather with a dtype change -- the wire pack / unpack of the halo exchange (16-bit wire for fp32 features):
 *   out[i, :] = cast(x[index[i], :]),  index int32 [n_index] or NULL (identity: a row-wise conversion of n_index rows).
 *   (x_dtype, out_dtype): F32 -> F16 | BF16 | F32, F16 | BF16 -> F32, F16 -> F16, BF16 -> BF16 (a plain pack of a column block).
 *   Stands where the reference would paddle.gather + cast.
 *   ldx: row stride of x in elements (0 = d): packs a column block of a wider matrix; out is dense [n_index, d]. */
int32_t pglamd_gather_rows_cast(const void* x, int32_t x_dtype, int64_t d, int64_t ldx, const int32_t* index,
                                int64_t n_index, void* out, int32_t out_dtype, void* stream);

/* K9  degree_norm.  Replaces cast/clip/pow in GF.degree_norm (pgl/nn/functional/graph_op.py:46-55):
 *     out[i] = max((float)degree[i], 1) ** -0.5      out F32 (out_f64 = 0) or F64 (= 1)           */
int32_t pglamd_degree_norm(const int64_t* degree, int64_t n, void* out, int32_t out_f64,
                           void* stream);

/* ------------------------------------------------------------------------------------------------
 * Neighbour sampling + relabel on the GPU ("next" row f3; the step before the hot path in the
 * GraphSAGE mini-batch loop).  Replaces paddle.geometric.sample_neighbors / reindex_graph as used
 * by pgl.sampling.NeighborSampler (pgl/sampling/sage.py:130-155) and the CPU path
 * Graph.sample_predecessor -> graph_kernel.sample_subset(_with_eid) (pgl/graph_kernel.pyx:266-339).
 *   count:  count[i] = min(degree(nodes[i]), k)   (k < 0: all neighbours)
 *   fill :  neighbours of nodes[i] written at offsets[i] (exclusive scan of count, made by the
 *           caller): all of them if degree <= k, else k uniformly WITHOUT replacement (Floyd),
 *           randomness = hash(seed, node, draw).  indptr/col/eid = the dst-sorted CSR; k <= 64.
 *   reindex: out_nodes = nodes, then every new neighbour id in order of first appearance;
 *           reindex_src[j] = new id of neighbors[j]; *num_out = len(out_nodes).  Deterministic.
 * ---------------------------------------------------------------------------------------------- */
int32_t pglamd_sample_neighbors_count(const int64_t* indptr, const int64_t* nodes, int64_t n,
                                      int64_t k, int64_t* count, void* stream);
int32_t pglamd_sample_neighbors_fill(const int64_t* indptr, const int32_t* col, const int32_t* eid,
                                     const int64_t* nodes, int64_t n, int64_t k, uint64_t seed,
                                     const int64_t* offsets, int64_t* out_neighbors,
                                     int64_t* out_eids, void* stream);
size_t pglamd_reindex_workspace_bytes(int64_t num_nodes, int64_t num_neighbors);
int32_t pglamd_reindex(const int64_t* nodes, int64_t num_nodes, const int64_t* neighbors,
                       int64_t num_neighbors, int64_t* reindex_src, int64_t* out_nodes,
                       int64_t* num_out, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Layer epilogue (row f1, "SpMM -> GEMM epilogue fusion"): the element passes after the dense X.W of
 * GraphSageConv (self + neigh + biases -> act -> F.normalize, pgl/nn/conv.py:99-115) and GCNConv (+ bias -> activation,
 * pgl/nn/conv.py:250-254) as ONE row kernel forward and one backward.  float32, rows contiguous.
 *   y[r,:] = normalize_L2( act( z[r,:] + bias ) )     act 0 none / 1 relu; normalize 0/1 (x / max(||x||, eps));
 *            y may alias z; inv_norm[n_rows] (written when normalize) is what the backward needs besides y.
 *   backward: dz = act'( normalize ? (dy - y <dy,y>) * inv_norm : dy ); col_partials[pglamd_row_epilogue_partials(n_rows), d]
 *            (optional) receives per-wave column sums of dz -- summed over rows they are the bias gradient.
 * Operand layout: the row operands -- z and y forward; dy, y, dz and col_partials backward -- are walked in lanes of 16 bytes
 * when d % 4 == 0, of 8 when d % 2 == 0, else of 4, and must be aligned to that lane: PGLAMD_E_ARG otherwise, nothing is
 * written.  bias and inv_norm: one float at a time.
 * ---------------------------------------------------------------------------------------------- */
int64_t pglamd_row_epilogue_partials(int64_t n_rows);
int32_t pglamd_row_epilogue(const float* z, const float* bias, int64_t n_rows, int64_t d, int32_t act,
                            int32_t normalize, float eps, float* y, float* inv_norm, void* stream);
int32_t pglamd_row_epilogue_backward(const float* dy, const float* y, const float* inv_norm,
                                     int64_t n_rows, int64_t d, int32_t act, int32_t normalize,
                                     float* dz, float* col_partials, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Multi-GPU exchange step of the row-partitioned path.  Replaces the collective of the reference's
 * DistGPUGraph -- all_reduce_sum_with_grad of the whole [N, d] output after every aggregation
 * (pgl/graph.py:1517-1553 -> pgl/utils/op.py:90-122, c_allreduce_sum) -- with one all-to-all-v of halo rows:
 *   pglamd_comm_unique_id   rank 0 fills id_out[PGLAMD_COMM_ID_BYTES]; the caller hands it to every rank by any means
 *                           (the reference's launcher broadcasts endpoints the same way: paddle.distributed.init_parallel_env)
 *   pglamd_comm_init        one RCCL communicator per process + a library-owned side stream + two events
 *   pglamd_halo_exchange_start   send_buf = rows for peer 0, 1, ... (send_rows[q] rows of row_bytes each), recv_buf
 *                           likewise.  Everything already queued on compute_stream (the pack kernel) is ordered before
 *                           the transfers by an event; the call returns at once, the caller keeps launching the
 *                           local-source aggregation on compute_stream -- the overlap.
 *   pglamd_halo_exchange_wait    makes compute_stream wait (on the GPU, no host sync) until recv_buf is complete.
 * RCCL is opened with dlopen at the first call: PGLAMD_E_UNAVAILABLE without librccl.so, PGLAMD_E_RCCL on RCCL errors.
 * The plan (which rows go where) is pglamd_halo_plan_* below.  pgl_amd.distributed uses torch.distributed's RCCL
 * all_to_all_single by default and this transport with PGLAMD_TRANSPORT=abi; a caller without torch has only this one.
 * ---------------------------------------------------------------------------------------------- */
#define PGLAMD_COMM_ID_BYTES 128
int32_t pglamd_comm_unique_id(void* id_out);
int32_t pglamd_comm_init(int32_t rank, int32_t world, const void* unique_id, void** comm_out);
int32_t pglamd_comm_destroy(void* comm);
int32_t pglamd_halo_exchange_start(void* comm, const void* send_buf, const int64_t* send_rows,
                                   void* recv_buf, const int64_t* recv_rows, int64_t row_bytes,
                                   void* compute_stream);
int32_t pglamd_halo_exchange_wait(void* comm, void* compute_stream);
/* The exchange WITHOUT a send buffer (ABI 3): with the owner's rows ordered by the set of peers that pull them
 * (pgl_amd.distributed.HaloPlan(row_order="peers")) every peer's rows are a few contiguous ranges of the feature matrix `x` itself;
 * they are sent from where they lie (one ncclSend per range) into the matching ranges of recv_buf -- no pack launch, no send-buffer
 * traffic.  send_ptr / recv_ptr [world + 1] delimit each peer's ranges in send_first / send_cnt (rows of x) and recv_first /
 * recv_cnt (rows of recv_buf); range k of a pair has the same length on both ends.  Several exchanges (up to 8) may be in flight;
 * pglamd_halo_exchange_wait retires them in start order. */
int32_t pglamd_halo_exchange_start_ranges(void* comm, const void* x, const int64_t* send_ptr,
                                          const int64_t* send_first, const int64_t* send_cnt, void* recv_buf,
                                          const int64_t* recv_ptr, const int64_t* recv_first,
                                          const int64_t* recv_cnt, int64_t row_bytes, void* compute_stream);

/* Halo plan of one rank (HOST pointers; every rank derives its own share from the global edge list and the part vector,
 * so no negotiation is needed).  Relabelling and layout follow apps/GNNAutoScale/graph_partition.py:70-101 (owned ids
 * contiguous per part, ascending original id inside a part) and apps/GNNAutoScale/dataset.py:196-209 ([owned | halo]).
 *   pglamd_halo_plan_sizes  -> sizes[5] = n_own, n_local_source_edges, n_halo_source_edges, n_halo_rows, n_send_rows
 *   pglamd_halo_plan_fill   offsets[world+1] first relabelled id of every part; own_global[n_own] original id of local row i;
 *                           (loc_rows, loc_cols)[n_loc] local dst row / local src row of the edges with both ends owned;
 *                           (hal_rows, hal_cols)[n_hal] local dst row / position in the halo block of the other in-edges;
 *                           halo_global[n_halo] relabelled ids of the halo rows, ascending = grouped by owner;
 *                           send_idx[n_send] owned rows to pack, grouped by destination rank; halo_splits / pull_splits[world]
 *                           rows received from / sent to each rank (the recv_rows / send_rows of pglamd_halo_exchange_start);
 *                           in_degree / out_degree[n_own] GLOBAL degrees of the owned nodes (DistGPUGraph.indegree/outdegree,
 *                           pgl/graph.py:1524-1532); edge_global[n_loc + n_hal] original edge id of local edge k
 *                           (order: local-source edges, then halo-source edges) -- where edge features are sliced.
 *   Any output pointer except offsets / halo_splits / pull_splits may be NULL.  Bit-identical to pgl_amd.distributed.HaloPlan. */
int32_t pglamd_halo_plan_sizes(const int64_t* src, int64_t src_stride, const int64_t* dst,
                               int64_t dst_stride, int64_t num_edges, int64_t num_nodes,
                               const int64_t* part, int32_t rank, int32_t world, int64_t* sizes);
int32_t pglamd_halo_plan_fill(const int64_t* src, int64_t src_stride, const int64_t* dst,
                              int64_t dst_stride, int64_t num_edges, int64_t num_nodes,
                              const int64_t* part, int32_t rank, int32_t world, int64_t* offsets,
                              int64_t* own_global, int64_t* loc_rows, int64_t* loc_cols,
                              int64_t* hal_rows, int64_t* hal_cols, int64_t* halo_global,
                              int64_t* send_idx, int64_t* halo_splits, int64_t* pull_splits,
                              int64_t* in_degree, int64_t* out_degree, int64_t* edge_global);

/* ------------------------------------------------------------------------------------------------
 * Host-side (CPU) helpers.  Pointers here are HOST pointers.
 * pglamd_map_ids replaces graph_kernel.map_edges / map_nodes (pgl/graph_kernel.pyx:104-138):
 *     out[i] = value of key in[i] in the (keys -> vals) dictionary; missing key -> 0, like
 *     std::unordered_map::operator[] in the reference.
 * pglamd_partition_kway stands behind pgl.partition.metis_partition (pgl/partition.py:37-91 ->
 * graph_kernel.metis_partition, pgl/graph_kernel.pyx:434-472).  No METIS code is built into or opened by
 * this library (round 5: the round-3/4 opt-in bridge pglamd_partition_metis / libpglamd_metis.so was removed from
 * the product; the reference's METIS lives only in the test oracle, oracle/_ref).
 * It is the engine's own multilevel k-way partitioner.  Same inputs as METIS_PartGraphKway as the reference calls it (CSR xadj/adjncy
 * int64, optional positive int64 vertex / edge weights), same output (part[N] int64 in
 * [0, nparts)); its ids are NOT METIS's -- parity there is on balance and edge cut.
 * ---------------------------------------------------------------------------------------------- */
/* ------------------------------------------------------------------------------------------------
 * Random walks and skip-gram pairs.  Replace pgl.sampling.random_walk / node2vec_walk / node2vec_walk_plus
 * (pgl/sampling/walk.py:23-185; their per-walker samplers graph_kernel.node2vec_sample / node2vec_plus_sample,
 * pgl/graph_kernel.pyx:140-224) and graph_kernel.skip_gram_gen_pair (pgl/graph_kernel.pyx:341-364).
 *   indptr [N+1] / col [E]  successor index (key = src) whose rows are sorted ascending by dst
 *   starts [W] int64        walk starts; ids outside [0, N) set *range_flag (if not NULL; the pglamd_csr_build
 *                           convention) and leave a walk of the start alone
 *   mode                    0 = uniform, 1 = node2vec (weights 1/p, 1, 1/q against succ(prev)), 2 = node2vec-plus
 *                           (the set is the union of succ(walk[0 .. t-1]))
 *   thr_return / thr_in / thr_out   acceptance thresholds floor(2^32 * w / max(1/p, 1, 1/q)) of the weights 1/p, 1, 1/q,
 *                           each in [0, 2^32] (modes 1 and 2; the step from the start is uniform)
 *   max_trials              rejection trials per step before one exact weighted scan (0 = scan only; <= 2^20 - 1)
 *   paths [W, num_steps+1]  row-major walks, -1 after a dead end; lengths [W] = nodes per walk (>= 1)
 * Every random number is a hash of (seed, walker, step, trial): the result does not depend on the launch, and
 * pglamd_random_walk_host (host pointers, threads <= 0: up to 16) returns the same arrays bit for bit (it returns
 * PGLAMD_E_RANGE for a start outside [0, N)).  No workspace.
 * Skip-gram: count[W * (num_steps+1)] = pairs of each (walker, position); the caller's exclusive scan of count gives
 * offsets for fill, which writes src / dst (int64) walker by walker, position by position, j ascending: position i of
 * a walk of length l pairs walk[i] with every walk[j] != walk[i], j in [max(0, i-r), min(l-1, i+r)], r = a hash of
 * (seed, walker, i) in [1, win_size].
 * ---------------------------------------------------------------------------------------------- */
int32_t pglamd_random_walk(const int64_t* indptr, const int32_t* col, int64_t num_nodes,
                           const int64_t* starts, int64_t num_walkers, int64_t num_steps, int32_t mode,
                           uint64_t thr_return, uint64_t thr_in, uint64_t thr_out, int32_t max_trials,
                           uint64_t seed, int64_t* paths, int64_t* lengths, int32_t* range_flag,
                           void* stream);
int32_t pglamd_random_walk_host(const int64_t* indptr, const int32_t* col, int64_t num_nodes,
                                const int64_t* starts, int64_t num_walkers, int64_t num_steps,
                                int32_t mode, uint64_t thr_return, uint64_t thr_in, uint64_t thr_out,
                                int32_t max_trials, uint64_t seed, int32_t threads, int64_t* paths,
                                int64_t* lengths);
int32_t pglamd_skip_gram_count(const int64_t* paths, const int64_t* lengths, int64_t num_walkers,
                               int64_t width, int64_t win_size, uint64_t seed, int64_t* count,
                               void* stream);
int32_t pglamd_skip_gram_fill(const int64_t* paths, const int64_t* lengths, int64_t num_walkers,
                              int64_t width, int64_t win_size, uint64_t seed, const int64_t* offsets,
                              int64_t* src, int64_t* dst, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Edge-weighted sampling.  The reference draws uniformly everywhere (graph_kernel.alias_sample_build_table,
 * pgl/graph_kernel.pyx:366-392, is exported and never called); these stand beside pglamd_random_walk,
 * pglamd_sample_neighbors_count / _fill and the torch.randint negatives of a skip-gram loop.  Every weighted draw is integer-exact.
 *
 * pglamd_edge_weight_table (device) / pglamd_edge_weight_table_host (HOST pointers, no row / workspace / stream): the table all
 * weighted draws read.
 *   indptr [N+1] int64      the index (dst-sorted for the sampler, the sorted successor index for walks)
 *   row [E] int32           the row of every position (ops.CSR.row32); NULL only for a single-row table (N == 1: a plain vector)
 *   eid [E] int32 or NULL   the row of `weight` position j reads (NULL: j itself)
 *   weight [num_weights]    fp32 (weight_f64 = 0) or fp64 (= 1)
 *   cum [E] int64, npos [N] int64, flag int32 (outputs)
 * Row v with positions b .. b+deg-1 and maximum weight m:  q[j] = 0 if w[j] == 0 or m == 0, else
 * max(1, floor((double)w[j] / (double)m * 2^32)) -- one fp64 division, one exact multiply; q in [0, 2^32], a row's total < 2^63.
 * cum[j] = q[b] + .. + q[j] (inclusive, within the row); npos[v] = positions of the row with q > 0.  A relative weight below
 * 2^-32 of the row maximum is rounded UP to one quantum (it stays drawable); a zero weight is never drawn; a row of zero weights
 * behaves like an empty row.  *flag = OR of PGLAMD_WEIGHT_* over all positions (NaN, negative, infinite weight; an eid or row
 * outside its table -- never dereferenced): the outputs are unspecified when it is not 0.  The result does not depend on the
 * launch (maximum and integer sums are order-independent) and is bit-identical between the two entry points.
 *
 * pglamd_random_walk_weighted(_host): pglamd_random_walk's uniform mode with every step drawn by weight: at cur with row
 * b .. b+deg-1 of the successor index and T = cum[b+deg-1]:  deg == 0 or T == 0 is a dead end; else r = scale64(draw(key, t+1, 0), T)
 * (walk_core.hpp) and the next node is col[j] for the smallest j with cum[j] > r.  No rejection, no trial counter; paths, lengths,
 * range_flag and the bit-identical host twin as pglamd_random_walk.  (Weights together with node2vec's p / q are not provided:
 * the exact fallback scan would need 128-bit sums of q * thr.)
 *
 * pglamd_sample_neighbors_weighted_count / _fill: the pair above over the dst-sorted index and its table.
 *   count[i] = npos[v] when k < 0 or npos[v] <= k, else k (v = nodes[i]); k <= 64.
 *   fill: the whole positive set in row order (no draw) in the first case; else draws c = 0 .. k-1 of successive sampling:
 *   R_c = the row total minus the q of the positions already chosen, r = scale64(mix64(seed ^ mix64(v * 0x100000001B3 + c)), R_c),
 *   the pick is the smallest not-yet-chosen position j whose running sum of q over the not-yet-chosen positions <= j exceeds r.
 *   Output in draw order (neighbour ids, optionally edge ids), a pure function of (seed, node id, draw).
 *
 * pglamd_sample_from_table: `count` independent draws WITH replacement from a single-row table cum[n]:
 *   out[i] = the smallest j with cum[j] > scale64(mix64(seed ^ mix64(i)), cum[n-1]);  -1 for every draw when cum[n-1] == 0.
 * ---------------------------------------------------------------------------------------------- */
#define PGLAMD_WEIGHT_NAN 1
#define PGLAMD_WEIGHT_NEGATIVE 2
#define PGLAMD_WEIGHT_INF 4
#define PGLAMD_WEIGHT_BAD_EID 8
size_t pglamd_edge_weight_table_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int32_t pglamd_edge_weight_table(const int64_t* indptr, const int32_t* row, const int32_t* eid,
                                 const void* weight, int32_t weight_f64, int64_t num_nodes,
                                 int64_t num_edges, int64_t num_weights, int64_t* cum, int64_t* npos,
                                 int32_t* flag, void* workspace, size_t workspace_bytes, void* stream);
int32_t pglamd_edge_weight_table_host(const int64_t* indptr, const int32_t* eid, const void* weight,
                                      int32_t weight_f64, int64_t num_nodes, int64_t num_edges,
                                      int64_t num_weights, int64_t* cum, int64_t* npos, int32_t* flag);
int32_t pglamd_random_walk_weighted(const int64_t* indptr, const int32_t* col, const int64_t* cum,
                                    int64_t num_nodes, const int64_t* starts, int64_t num_walkers,
                                    int64_t num_steps, uint64_t seed, int64_t* paths, int64_t* lengths,
                                    int32_t* range_flag, void* stream);
int32_t pglamd_random_walk_weighted_host(const int64_t* indptr, const int32_t* col, const int64_t* cum,
                                         int64_t num_nodes, const int64_t* starts, int64_t num_walkers,
                                         int64_t num_steps, uint64_t seed, int32_t threads,
                                         int64_t* paths, int64_t* lengths);
int32_t pglamd_sample_neighbors_weighted_count(const int64_t* npos, const int64_t* nodes, int64_t n,
                                               int64_t k, int64_t* count, void* stream);
int32_t pglamd_sample_neighbors_weighted_fill(const int64_t* indptr, const int32_t* col,
                                              const int32_t* eid, const int64_t* cum, const int64_t* npos,
                                              const int64_t* nodes, int64_t n, int64_t k, uint64_t seed,
                                              const int64_t* offsets, int64_t* out_neighbors,
                                              int64_t* out_eids, void* stream);
int32_t pglamd_sample_from_table(const int64_t* cum, int64_t n, int64_t count, uint64_t seed,
                                 int64_t* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Negative sampling checked against the graph: absent edges and BPR triples.  Replaces the per-user Python loop
 * UniformSample_original_python of the reference's LightGCN example (examples/lightgcn/utils.py: a uniform positive, then
 * `while True: negitem = randint(...)` until the item is not in posForUser; examples/ngcf/utils.py does the same) and stands beside
 * the unchecked negatives of a skip-gram loop (torch.randint / pglamd_sample_from_table: a "negative" may be a true neighbour).
 *   indptr [N+1] / col [E]  successor index (key = src) whose rows are sorted ascending by dst, multi-edges allowed, as for
 *                           pglamd_random_walk (a predecessor index sorted by src corrupts the HEAD of an edge instead)
 *   cum [hi] int64 or NULL  NULL: uniform candidates; else the prefix sums of a single-row pglamd_edge_weight_table (the noise
 *                           distribution); then lo must be 0 and hi the table's length (PGLAMD_E_RANGE otherwise)
 *   lo, hi                  the candidate range [lo, hi): 0 <= lo, hi <= N (PGLAMD_E_RANGE), lo < hi (PGLAMD_E_SHAPE)
 *   src [n] int64           the sources; num_neg = K >= 1 and 0 <= max_trials <= 2^20 - 1 (PGLAMD_E_ARG); n * K <= 2^40
 *   neg [n, K] int64        row-major; pos [n] int64 or NULL; flags int32 or NULL, zeroed by the caller, OR-ed into
 * Excluded set X_i of position i: the distinct entries of row src[i] inside [lo, hi) (successors outside the range are ignored),
 * plus src[i] itself when exclude_self != 0 and src[i] lies in the range.  key_i = walker_key(seed, i) (walk_core.hpp): the POSITION,
 * not the node id, so a source listed twice gets different negatives.  Negative k of position i:
 *   trials tr = 0 .. max_trials-1: r = draw(key_i, k, tr); x = lo + scale64(r, hi - lo), or with cum and T = cum[hi-1] > 0 the
 *   smallest x with cum[x] > scale64(r, T); the first x outside X_i is the answer (one binary search of the row per trial);
 *   then one exact draw with r = draw(key_i, k, max_trials): uniform: t = scale64(r, C), C = (hi - lo) - |X_i|, the t-th id of
 *   [lo, hi) outside X_i in ascending order; weighted: t = scale64(r, R), R = T - the weight of X_i, the id at which the prefix
 *   sums of the weights with X_i's set to zero first exceed t.  C == 0 / R == 0 answers -1 and sets PGLAMD_NEG_EMPTY.
 * pos[i] = col[b + scale64(draw(key_i, K, 0), deg)], a uniform position of the row (a multi-edge counts twice), -1 for an empty
 * row; the range does not apply to it.  A source outside [0, N) is never dereferenced: PGLAMD_NEG_RANGE, its outputs are -1.
 * Every output is a pure function of the arguments (negative_core.hpp has the definition in full).  One launch, no workspace, no
 * host read.  pglamd_sample_negatives_host (HOST pointers, threads <= 0: up to 16) returns the same arrays bit for bit whatever the
 * thread count; it returns PGLAMD_E_RANGE for a source outside [0, N).
 * ---------------------------------------------------------------------------------------------- */
#define PGLAMD_NEG_RANGE 1
#define PGLAMD_NEG_EMPTY 2
int32_t pglamd_sample_negatives(const int64_t* indptr, const int32_t* col, int64_t num_nodes,
                                const int64_t* cum, int64_t lo, int64_t hi, const int64_t* src,
                                int64_t n, int64_t num_neg, int32_t exclude_self, int32_t max_trials,
                                uint64_t seed, int64_t* neg, int64_t* pos, int32_t* flags,
                                void* stream);
int32_t pglamd_sample_negatives_host(const int64_t* indptr, const int32_t* col, int64_t num_nodes,
                                     const int64_t* cum, int64_t lo, int64_t hi, const int64_t* src,
                                     int64_t n, int64_t num_neg, int32_t exclude_self,
                                     int32_t max_trials, uint64_t seed, int32_t threads, int64_t* neg,
                                     int64_t* pos, int32_t* flags);

/* ------------------------------------------------------------------------------------------------
 * Metapath random walks over the relations of a heterogeneous graph.  Replace metapath_randomwalk / metapath_randomwalk_with_walktimes
 * of the reference's metapath2vec example (examples/metapath2vec/datasets/sampling.py:285-398, the same file under apps/Graph4Rec: a
 * Python loop with one sample_successor call per step and one list append per walker).  One launch for every step of every walker.
 *   indptr [R * (N+1)] int64  the relation-stacked successor index: block r = relation r's indptr (rows sorted ascending by dst, as
 *                             for pglamd_random_walk) plus the number of edges of relations 0 .. r-1 -- absolute positions of col
 *   col [sum E_r] int32       the relations' col arrays concatenated in the same order
 *   cum [sum E_r] int64 or NULL   NULL: uniform steps (multi-edges count with their multiplicity); else the relations'
 *                             pglamd_edge_weight_table prefix sums concatenated (they are sums WITHIN a row: nothing to rebase)
 *   metapath [L] int32, HOST  relation numbers in [0, R), 1 <= L <= 64; 0 <= phase < L (PGLAMD_E_ARG otherwise).  Copied into the
 *                             kernel's argument block: no device allocation or copy inside the call (graph capture as its siblings)
 *   starts / paths / lengths / range_flag   as pglamd_random_walk
 * Walker w stands at starts[w] at position 0; the step from position t to t + 1 draws from the successors of the current node under
 * relation metapath[(phase + t) % L]: walk_core.hpp's uniform_step / weighted_step with the (walker_key(seed, w), t) arguments of
 * pglamd_random_walk (mode 0) / pglamd_random_walk_weighted.  So L == 1, phase == 0 returns bit for bit what those return over
 * that relation's own index with the same seed.  An empty row under the step's relation, or a row of zero weights, is a dead end.
 * pglamd_metapath_walk_host (HOST pointers, threads <= 0: up to 16; *range_flag is OR-ed, not an error) returns the same arrays bit
 * for bit, independent of the thread count.  No workspace.
 * ---------------------------------------------------------------------------------------------- */
int32_t pglamd_metapath_walk(const int64_t* indptr, const int32_t* col, const int64_t* cum,
                             int64_t num_nodes, int32_t num_relations, const int32_t* metapath,
                             int32_t metapath_len, int32_t phase, const int64_t* starts,
                             int64_t num_walkers, int64_t num_steps, uint64_t seed, int64_t* paths,
                             int64_t* lengths, int32_t* range_flag, void* stream);
int32_t pglamd_metapath_walk_host(const int64_t* indptr, const int32_t* col, const int64_t* cum,
                                  int64_t num_nodes, int32_t num_relations, const int32_t* metapath,
                                  int32_t metapath_len, int32_t phase, const int64_t* starts,
                                  int64_t num_walkers, int64_t num_steps, uint64_t seed,
                                  int32_t threads, int64_t* paths, int64_t* lengths,
                                  int32_t* range_flag);

/* ------------------------------------------------------------------------------------------------
 * Relation-wise neighbour sampling over the relations of a heterogeneous graph: the mini-batch step of RGCN / R-UniMP.  Replaces
 * the loop of the reference's MAG240M example (examples/NeurIPS2022-OGB-Challenge/MAG240M/dataset/new_dataset_p2p.py:163-193: one
 * paddle.geometric.sample_neighbors call per edge type per layer, then reindex_heter_graph and an edge_split array) and stands
 * where pgl.sampling.HeteroNeighborSampler is declared and left unimplemented (pgl/sampling/sage.py:158-162).
 *   indptr [R * (N+1)] int64  the relation-stacked PREDECESSOR index: block r = relation r's dst-sorted indptr plus the number of
 *                             edges of relations 0 .. r-1 -- absolute positions of col / eid
 *   col [sum E_r] int32       the relations' sources by position, concatenated in the same order
 *   eid [sum E_r] int32       the relation-LOCAL original edge ids by position, concatenated (may be NULL when out_eids is)
 *   fanouts [R] int64, HOST   per relation: < 0 the whole row, 0 nothing, else at most that many (<= 64: PGLAMD_E_SHAPE);
 *                             1 <= R <= PGLAMD_SAMPLE_MAX_RELATIONS (PGLAMD_E_SHAPE).  Copied into the kernel's argument block: no
 *                             device allocation or copy inside the call
 *   nodes [n] int64           the seeds, inside [0, N) (the caller checks; the host twin does: PGLAMD_E_SHAPE)
 * Slot r * n + i holds what pglamd_sample_neighbors_count / _fill return for nodes[i] over relation r's own index with fan-out
 * fanouts[r] and seed mix64(seed ^ mix64(r)) (mix64: the splitmix64 finaliser of sampling.hip): the same Floyd draws in the same
 * order, the same whole-row copy.  The seed is mixed per relation because a draw is a function of (seed, node id, draw number).
 *   count [R * n] int64       written by _count; the caller scans it (pglamd_exclusive_scan_i64) into offsets [R * n]
 *   out_neighbors / out_dst / out_eids [T] int64   relation-major, then seed position, then draw order: the sampled source, the
 *                             seed POSITION i of the slot, the relation-local edge id (out_eids may be NULL)
 * Relation r owns [offsets[r * n], offsets[(r + 1) * n]) of the outputs.  One lane per (relation, seed); no workspace.
 * pglamd_sample_relations_host (HOST pointers, threads <= 0: up to 16) returns the same arrays bit for bit, independent of the
 * thread count: it writes count and edge_split [R + 1] (relation r owns [edge_split[r], edge_split[r + 1])) on every call and,
 * when out_neighbors is not NULL, the outputs of num_out == edge_split[R] entries (PGLAMD_E_ARG otherwise).
 * ---------------------------------------------------------------------------------------------- */
#define PGLAMD_SAMPLE_MAX_RELATIONS 64
int32_t pglamd_sample_relations_count(const int64_t* indptr, int64_t num_nodes, int32_t num_relations,
                                      const int64_t* fanouts, const int64_t* nodes, int64_t n,
                                      int64_t* count, void* stream);
int32_t pglamd_sample_relations_fill(const int64_t* indptr, const int32_t* col, const int32_t* eid,
                                     int64_t num_nodes, int32_t num_relations, const int64_t* fanouts,
                                     const int64_t* nodes, int64_t n, uint64_t seed,
                                     const int64_t* offsets, int64_t* out_neighbors, int64_t* out_dst,
                                     int64_t* out_eids, void* stream);
int32_t pglamd_sample_relations_host(const int64_t* indptr, const int32_t* col, const int32_t* eid,
                                     int64_t num_nodes, int32_t num_relations, const int64_t* fanouts,
                                     const int64_t* nodes, int64_t n, uint64_t seed, int32_t threads,
                                     int64_t* count, int64_t* edge_split, int64_t* out_neighbors,
                                     int64_t* out_dst, int64_t* out_eids, int64_t num_out);

/* ------------------------------------------------------------------------------------------------
 * Relational aggregation: every edge type of a heterogeneous graph in one launch.  Replaces the aggregation side of the
 * reference's RGCNConv loop (pgl/nn/conv.py:1014-1019: per edge type one matmul over all source rows, one
 * send_recv(.., "mean") and one add).  fp32 only.
 *   indptr      int64, relation r's row at indptr + r * indptr_rel_stride, out_rows + 1 entries read: absolute positions of col
 *               (the layout of the relation-stacked index above; a flat [R * n + 1] table is the same under a stride of n)
 *   col         int32: the row of x an edge position reads.  A column outside [0, x_rows) contributes nothing
 *   x           relation r reads x + r * x_rel_stride (0: one shared table); row c at + c * x_row_stride; d floats per row
 *   col_scale   NULL, or c[r, col] at col_scale + r * col_scale_rel_stride + col: a factor per (relation, column)
 *   out         out_rel_stride == 0: out[v] = sum over r of S[r, v] at out + v * out_row_stride;
 *               else S[r, v] at out + v * out_row_stride + r * out_rel_stride.  Every element of rows [0, out_rows) is written
 *   S[r, v, :] = s_r(v) * sum over e in [indptr[r, v], indptr[r, v + 1]) of c[r, col[e]] * x_r[col[e], :], the edges in ascending
 *   position order, s_r(v) = 1 (PGLAMD_SUM) or 1 / the segment's length (PGLAMD_MEAN); an empty segment gives +0.0, the
 *   relations are added in ascending order.  No atomics: the result is a pure function of the arguments.
 *   long_row / long_rows / n_long_rows   long_rows [n_long_rows] int64 lists every row v < out_rows that owns a segment longer
 *               than long_row (>= 1) edges, each once (rows >= out_rows may be listed; they are ignored).  Those segments are
 *               summed by a second launch, one workgroup per listed row, in 256 / G fixed contiguous slices combined in slice
 *               order.  n_long_rows == 0: the caller vouches that there is no such segment; one launch, long_row is not read.
 * Any d >= 1: 16-byte loads where d % 4 == 0 and x, out and all their strides are 16-byte aligned, 4-byte loads otherwise.
 * PGLAMD_E_ARG for another reduce_op, a NULL pointer or long_row < 1; PGLAMD_E_SHAPE for num_relations < 1 or a row stride
 * below d.  No workspace, no host read.
 * ---------------------------------------------------------------------------------------------- */
int32_t pglamd_aggregate_relations(const float* x, int64_t x_rows, int64_t x_row_stride,
                                   int64_t x_rel_stride, const int64_t* indptr,
                                   int64_t indptr_rel_stride, const int32_t* col,
                                   const float* col_scale, int64_t col_scale_rel_stride,
                                   int32_t num_relations, int64_t out_rows, int64_t d,
                                   int32_t reduce_op, float* out, int64_t out_row_stride,
                                   int64_t out_rel_stride, int64_t long_row, const int64_t* long_rows,
                                   int64_t n_long_rows, void* stream);

/* ------------------------------------------------------------------------------------------------
 * PinSAGE neighbourhoods: per seed, the top_k nodes most often visited by num_walks random walks of num_steps steps from it,
 * with their visit counts -- what pgl.nn.PinSageConv's edge weights are defined from (the reference has the layer and no
 * sampler).  One launch; no path is written to memory.
 *   indptr [N+1] / col [E]  successor index whose rows are sorted ascending by dst, as for pglamd_random_walk
 *   cum [E] int64 or NULL   NULL: uniform steps; else the prefix sums of pglamd_edge_weight_table over THAT index: weighted steps
 *   seeds [S] int64         a seed outside [0, N) sets *range_flag (if not NULL); its row is all -1 / 0 and its num is 0
 *   num_walks R, num_steps L, top_k T   each >= 1 (PGLAMD_E_ARG); R * L <= PGLAMD_VISIT_MAX and T <= PGLAMD_VISIT_MAX_TOPK
 *                           (PGLAMD_E_RANGE: nothing is ever truncated silently); N and S <= INT32_MAX
 *   nbr [S, T] int64 (padding -1), cnt [S, T] int32 (padding 0), num [S] int32 = min(T, distinct visited nodes)
 * Walker w = s * R + r (r in [0, R)) starts at seeds[s] and takes exactly the walk that row w of pglamd_random_walk (mode 0; with
 * cum: pglamd_random_walk_weighted) holds for starts = every seed repeated R times and the same `seed`: the same walker_key, the
 * same uniform_step / weighted_step (walk_core.hpp), the same dead ends (an empty row, a row of zero weights).  The visits of
 * seed s are positions 1 .. len-1 of its R walks, without the entries equal to seeds[s] (the layer has its own self term).  They
 * are counted per distinct node, ordered by (count descending, node id ascending) and cut at T; the filled entries are a prefix
 * of each row.  All integer: the result is a pure function of the arguments -- independent of the launch and of repeated seeds
 * (which get different walkers, hence different walks) -- and pglamd_walk_visit_topk_host (HOST pointers, threads <= 0: up to
 * 16; *range_flag is OR-ed, not an error) returns the same three arrays bit for bit.  No workspace.
 * R * L <= 256 runs one wave per seed, larger shapes one workgroup per seed (walk_visit.hip).
 * ---------------------------------------------------------------------------------------------- */
#define PGLAMD_VISIT_MAX 4096
#define PGLAMD_VISIT_MAX_TOPK 256
int32_t pglamd_walk_visit_topk(const int64_t* indptr, const int32_t* col, const int64_t* cum,
                               int64_t num_nodes, const int64_t* seeds, int64_t num_seeds,
                               int64_t num_walks, int64_t num_steps, int64_t top_k, uint64_t seed,
                               int64_t* nbr, int32_t* cnt, int32_t* num, int32_t* range_flag,
                               void* stream);
int32_t pglamd_walk_visit_topk_host(const int64_t* indptr, const int32_t* col, const int64_t* cum,
                                    int64_t num_nodes, const int64_t* seeds, int64_t num_seeds,
                                    int64_t num_walks, int64_t num_steps, int64_t top_k, uint64_t seed,
                                    int32_t threads, int64_t* nbr, int32_t* cnt, int32_t* num,
                                    int32_t* range_flag);

/* ------------------------------------------------------------------------------------------------
 * S2: the subgraph INDUCED by a node set (batch construction of Cluster-GCN / GraphSAINT style training).  Stands in for
 * graph_kernel.extract_edges_from_nodes (pgl/graph_kernel.pyx:394-432) and the relabel of pgl.sampling.custom.subgraph
 * (pgl/sampling/custom.py:23-83).  indptr / col / eid = the dst-sorted CSR (eid NULL: the edge id of a position is the
 * position); nodes[n] int64, distinct, inside [0, num_nodes).  With local[nodes[i]] = i and -1 elsewhere, the result lists
 * (local[col[j]], i, eid[j]) for i = 0 .. n-1 in the order given, j = indptr[nodes[i]] .. indptr[nodes[i] + 1] - 1 ascending,
 * wherever local[col[j]] >= 0: grouped by dst_local, non-decreasing; multi-edges and self-loops kept.  Deterministic.
 *   count   marks the table, counts the kept edges and writes status[4] (int64): status[0] = kept edges, status[1] = flags
 *           (bit 0: an id outside [0, num_nodes) -- never dereferenced; bit 1: a repeated id), status[2] = candidate
 *           positions (the sum of the selected rows' lengths).  The caller reads status ONCE, refuses a non-zero flag and
 *           allocates the three outputs of status[0] entries.
 *   fill    writes src_local / dst_local / eids (int64) from the SAME workspace count left behind (same arguments, same
 *           stream, nothing else queued on the workspace in between).  Not to be called when a flag is set or kept == 0.
 * Work is split by candidate position (tiles of 1024), not by row: time follows the sum of the rows' lengths, not the longest.
 * launch_threads: the largest number of lanes one launch starts (the kernels stride beyond it).
 * pglamd_induced_subgraph_host: the same three arrays from the same definition, HOST pointers, int64 col / eid (eid NULL as
 * above); *num_out = kept edges, outputs sized by the caller for the sum of the selected rows' lengths.  PGLAMD_E_ARG for a
 * repeated or out-of-range id.
 * ---------------------------------------------------------------------------------------------- */
int64_t pglamd_induced_subgraph_launch_threads(void);
size_t pglamd_induced_subgraph_workspace_bytes(int64_t num_nodes, int64_t n, int64_t num_edges);
int32_t pglamd_induced_subgraph_count(const int64_t* indptr, const int32_t* col, int64_t num_nodes,
                                      int64_t num_edges, const int64_t* nodes, int64_t n,
                                      int64_t* status, void* workspace, size_t workspace_bytes,
                                      void* stream);
int32_t pglamd_induced_subgraph_fill(const int64_t* indptr, const int32_t* col, const int32_t* eid,
                                     int64_t num_nodes, int64_t num_edges, const int64_t* nodes,
                                     int64_t n, int64_t* out_src, int64_t* out_dst, int64_t* out_eid,
                                     void* workspace, size_t workspace_bytes, void* stream);
int32_t pglamd_induced_subgraph_host(const int64_t* indptr, const int64_t* col, const int64_t* eid,
                                     int64_t num_nodes, const int64_t* nodes, int64_t n,
                                     int64_t* out_src, int64_t* out_dst, int64_t* out_eid,
                                     int64_t* num_out);

/* ------------------------------------------------------------------------------------------------
 * Graph pooling (pool.hip): the index work of SAGPool on the device.
 *
 * pglamd_segment_topk stands in for the ratio branch of pgl.math.segment_topk (pgl/math.py:276-364: scatter into a dense
 * [segments, max_len] matrix padded with -1e20, argsort of all of it, selection by a mask).
 *   scores [n] fp32; seg_ptr [S+1] int64: segment s is the positions seg_ptr[s] .. seg_ptr[s+1]-1 (contiguous segments);
 *   out_ptr [S+1] int64: k_s = out_ptr[s+1] - out_ptr[s] entries of perm belong to segment s; perm [out_ptr[S]] int64.
 * perm[out_ptr[s] + j] = the global position of the j-th element of segment s in the order (score descending, position
 * ascending), j < k_s.  Equality is IEEE equality (-0.0 ties with +0.0); every NaN is greater than every number and ties with
 * every other NaN.  For scores >= -1e20 this is what the reference's stable descending argsort of the padded matrix selects;
 * below it (and for -inf) the reference sorts scores behind its padding -- here the order stays inside the segment.
 *   *status (device int64, bits are OR-ed in: the caller clears it): bit 0 = a segment with a negative length or longer than
 *   PGLAMD_TOPK_MAX_SEG, bit 1 = a k_s outside [0, len_s].  Such a segment is skipped: nothing of it is read or written.
 * One wave64 per segment up to 256 elements, one workgroup per longer one (its sort table is PGLAMD_TOPK_MAX_SEG 64-bit words of
 * LDS = 32 KiB: five workgroups per CU; 8192 would leave two).  Two launches, no workspace, no host read; a pure function of
 * the arguments.  pglamd_segment_topk_host: HOST pointers (status too), the same perm and the same bits.
 *
 * pglamd_filter_edges_* stand in for pgl.utils.transform.filter_adj (pgl/utils/transform.py:138-168).
 *   edges [E, 2] int64, row r at edges + r * edge_stride (edge_stride >= 2, in elements); perm [m] int64, distinct ids inside
 *   [0, num_nodes).  With new_id[perm[i]] = i and -1 elsewhere, edge e is kept iff both its ends have new_id >= 0;
 *   out_edges [kept, 2] = the kept edges' relabelled ends, out_pos [kept] = their positions e, both in input order.
 *   count   builds the table, counts per tile of 1024 positions and writes status[2] (int64): status[0] = kept, status[1] =
 *           flags (bit 0: an id of perm or an edge end outside [0, num_nodes) -- never dereferenced; bit 1: a repeated id in
 *           perm).  The caller reads status ONCE, refuses a flag and allocates the outputs.
 *   fill    writes out_edges / out_pos from the SAME workspace count left behind (same arguments, same stream, nothing else
 *           queued on the workspace in between).  Not to be called when a flag is set or kept == 0.
 * launch_threads: the largest number of lanes one launch starts (the kernels stride beyond it).
 * pglamd_filter_edges_host: HOST pointers, the same arrays and the same status pair; out_edges / out_pos sized by the caller for
 * E edges (both NULL: count only).  A flag is reported in status[1], not as an error.
 * ---------------------------------------------------------------------------------------------- */
#define PGLAMD_TOPK_MAX_SEG 4096
int32_t pglamd_segment_topk(const float* scores, const int64_t* seg_ptr, const int64_t* out_ptr,
                            int64_t num_segments, int64_t* perm, int64_t* status, void* stream);
int32_t pglamd_segment_topk_host(const float* scores, const int64_t* seg_ptr, const int64_t* out_ptr,
                                 int64_t num_segments, int64_t* perm, int64_t* status);
int64_t pglamd_filter_edges_launch_threads(void);
size_t pglamd_filter_edges_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int32_t pglamd_filter_edges_count(const int64_t* edges, int64_t edge_stride, int64_t num_edges,
                                  const int64_t* perm, int64_t m, int64_t num_nodes, int64_t* status,
                                  void* workspace, size_t workspace_bytes, void* stream);
int32_t pglamd_filter_edges_fill(const int64_t* edges, int64_t edge_stride, int64_t num_edges,
                                 int64_t num_nodes, int64_t* out_edges, int64_t* out_pos,
                                 void* workspace, size_t workspace_bytes, void* stream);
int32_t pglamd_filter_edges_host(const int64_t* edges, int64_t edge_stride, int64_t num_edges,
                                 const int64_t* perm, int64_t m, int64_t num_nodes, int64_t* out_edges,
                                 int64_t* out_pos, int64_t* status);

/* ------------------------------------------------------------------------------------------------
 * Attention read-out (readout.hip): a softmax-weighted sum over the contiguous rows of each segment, one streaming pass.
 *
 * pglamd_attention_readout stands in for the read-out of GlobalAttention (pgl/nn/pool.py:174-178: segment softmax of the gate,
 * the product with the features, the segment sum; mode PGLAMD_READOUT_GATE) and for the last round's read-out of Set2Set
 * (pgl/nn/pool.py:139-142: the gathered query, the row dot, the segment softmax, the product, the segment sum; mode
 * PGLAMD_READOUT_QUERY).  With x [num_rows, d] fp32 (rows contiguous, d <= 512), segment g = rows seg_ptr[g] .. seg_ptr[g+1]-1:
 *     s_i    = operand[i]                       gate mode:  operand = score [num_rows]
 *     s_i    = <x[i, :], operand[g, :]>         query mode: operand = q [num_segments, d]
 *     a_i    = exp(s_i - max_g s) / sum_{j in g} exp(s_j - max_g s)
 *     out[g] = sum_{i in g} a_i x[i, :]         out [num_segments, d];  stats[g] = (max_g s, the sum)   [num_segments, 2]
 * An empty segment gives out = exactly 0 and stats = (-inf, 0), written by the kernel (no memset is needed).
 * pglamd_attention_readout_backward, from grad_out [num_segments, d] and the forward's out and stats, with
 * c_g = <grad_out[g], out[g]>, t_i = <grad_out[g], x[i]>, ds_i = a_i (t_i - c_g) and a_i recomputed from stats:
 *     grad_x[i]       = a_i grad_out[g]  (+ ds_i q[g] in query mode)           when need_x
 *     grad_operand[i] = ds_i                        (gate mode,  [num_rows])     when need_operand
 *     grad_operand[g] = sum_{i in g} ds_i x[i]      (query mode, [num_segments, d]; exactly 0 for an empty segment)
 *   A gradient that is not needed is not stored (its pointer may be NULL); the others' bits do not depend on it.
 * The plan (host arithmetic on seg_ptr, pgl_amd/readout_ops.py: host_pieces), device int64 like seg_ptr [num_segments + 1]:
 *   pieces [num_pieces, 4] = (segment, first row, rows <= PGLAMD_READOUT_PIECE, part): consecutive runs of one segment's rows; every
 *       segment has at least one piece (an empty one a piece of 0 rows).  part = -1 for the only piece of its segment, else the
 *       piece's slot in the workspace, 0 <= part < num_long_pieces.
 *   long_segs [num_long, 3] = (segment, first part, parts) of the segments of more than one piece, parts consecutive.
 *   An entry that does not fit seg_ptr, num_rows or the counts is skipped: nothing outside the operands is read or written.
 * Launches: one, plus one merge launch when num_long > 0 (in the backward: and query mode with need_operand).  Atomic-free, fixed
 * order: a pure function of the arguments, bit for bit.  The forward writes no [num_rows, .] array.
 * Alignment: rows are walked in 16-byte lanes when d % 4 == 0 and x, out, grad_out, grad_x, the workspace and (query mode) q and
 * its gradient are 16-byte aligned; otherwise one float at a time in the same lane layout -- the same bits.  score, its
 * gradient and stats: one float at a time.
 * Non-finite scores: a -inf score is a weight of exactly 0 (also as a segment's first row and as a whole piece); a segment whose
 * scores are all -inf, or that holds a +inf or a NaN score, has NaN in its own rows of out and of the gradients, and only there.
 * PGLAMD_E_ARG for d outside [1, 512], another mode, a NULL operand or bad counts; PGLAMD_E_WORKSPACE when num_long > 0 and the
 * workspace is smaller than pglamd_attention_readout_workspace_bytes (one size for both directions).  Nothing is written on a
 * refusal.
 * ---------------------------------------------------------------------------------------------- */
#define PGLAMD_READOUT_PIECE 256
#define PGLAMD_READOUT_GATE 0
#define PGLAMD_READOUT_QUERY 1
size_t pglamd_attention_readout_workspace_bytes(int64_t num_long_pieces, int64_t d);
int32_t pglamd_attention_readout(const float* x, int64_t num_rows, int64_t d, int32_t mode,
                                 const float* operand, const int64_t* seg_ptr, int64_t num_segments,
                                 const int64_t* pieces, int64_t num_pieces, const int64_t* long_segs,
                                 int64_t num_long, int64_t num_long_pieces, float* out, float* stats,
                                 void* workspace, size_t workspace_bytes, void* stream);
int32_t pglamd_attention_readout_backward(const float* grad_out, const float* x, int64_t num_rows,
                                          int64_t d, int32_t mode, const float* operand,
                                          const float* out, const float* stats, const int64_t* seg_ptr,
                                          int64_t num_segments, const int64_t* pieces,
                                          int64_t num_pieces, const int64_t* long_segs,
                                          int64_t num_long, int64_t num_long_pieces, int32_t need_x,
                                          int32_t need_operand, float* grad_x, float* grad_operand,
                                          void* workspace, size_t workspace_bytes, void* stream);

/* Host twin of pglamd_csr_build for numpy-mode graphs (Graph.indegree()/sorted_edges() before
 * Graph.tensor(), as examples/gcn/train.py:83 does): same outputs, same order, HOST pointers.
 * Replaces graph_kernel.build_index (pgl/graph_kernel.pyx:59-88) on the CPU side. */
int32_t pglamd_build_index_host(const int64_t* u, int64_t u_stride, const int64_t* v,
                                int64_t v_stride, int64_t num_edges, int64_t num_nodes,
                                int64_t* degree, int64_t* sorted_v, int64_t* sorted_u,
                                int64_t* sorted_eid, int64_t* indptr);
int32_t pglamd_map_ids(const int64_t* keys, const int64_t* vals, int64_t n_keys, const int64_t* in,
                       int64_t n_in, int64_t* out);
int32_t pglamd_partition_kway(int64_t num_nodes, const int64_t* xadj, const int64_t* adjncy,
                              const int64_t* vwgt, const int64_t* adjwgt, int64_t nparts,
                              uint64_t seed, int64_t* part, int64_t* edgecut);
/* The same partitioner with what a row-partitioned aggregation needs: a SECOND balance constraint (vwgt2, e.g. 1 per row next to
 * vwgt = in-degree + 1: a rank's time follows its edges, its row-wise kernels and its memory follow its rows), explicit imbalance
 * bounds ub / ub2 (<= 1: 1.03) and a thread count (0: $PGLAMD_THREADS, else min(cores, 16)).  Parallel and deterministic: the
 * parts depend on (graph, weights, nparts, seed) only, not on the thread count.  pglamd_partition_edges takes the DIRECTED edge
 * list as it is (strided int64 src / dst) and builds the symmetrised adjacency itself, in parallel. */
int32_t pglamd_partition_kway2(int64_t num_nodes, const int64_t* xadj, const int64_t* adjncy,
                               const int64_t* vwgt, const int64_t* vwgt2, const int64_t* adjwgt,
                               int64_t nparts, double ub, double ub2, uint64_t seed, int32_t threads,
                               int64_t* part, int64_t* edgecut);
int32_t pglamd_partition_edges(const int64_t* src, int64_t src_stride, const int64_t* dst,
                               int64_t dst_stride, int64_t num_edges, int64_t num_nodes,
                               const int64_t* vwgt, const int64_t* vwgt2, int64_t nparts, double ub,
                               double ub2, uint64_t seed, int32_t threads, int64_t* part,
                               int64_t* edgecut);

#ifdef __cplusplus
}
#endif
#endif /* PGL_AMD_H_ */
