// readout.hip -- the attention read-outs of pgl.nn (GlobalAttention, pgl/nn/pool.py:174-178; Set2Set, pgl/nn/pool.py:139-142) as one
// streaming pass: a softmax-weighted sum over CONTIGUOUS rows.  No index, no gather: not a variant of the CSR attention kernels.
// tests/readout_defs.py restates the definition in plain torch.
//
//   s_i    = score[i]  (gate mode)   |   <x[i, :], q[g, :]>  (query mode)            i in segment g = rows seg_ptr[g] .. seg_ptr[g+1]-1
//   a_i    = exp(s_i - max_g s) / sum_{j in g} exp(s_j - max_g s)
//   out[g] = sum_{i in g} a_i x[i, :]                     stats[g] = (max_g s, the sum); an empty segment: out = 0, stats = (-inf, 0)
// backward, with c_g = <d out[g], out[g]>, t_i = <d out[g], x[i]>, ds_i = a_i (t_i - c_g), a_i recomputed from stats:
//   d x[i] = a_i d out[g] (+ ds_i q[g]),   d score[i] = ds_i,   d q[g] = sum_{i in g} ds_i x[i]  (0 for an empty segment)
//
// Unit of work: a PIECE, at most PGLAMD_READOUT_PIECE consecutive rows of one segment, listed by the host plan (pgl_amd/readout_ops.py:
// host_pieces) as (segment, first row, rows, part).  Every segment has at least one piece -- an empty one a piece of 0 rows -- so
// every row of out / d q is written by a kernel, never by a memset.  One wave64 per piece, kWavesPerBlock pieces per workgroup,
// workgroups capped and striding over the pieces; no barrier and no LDS in the piece kernels.
//   lanes     a group of G lanes owns a row: G = ceil(d / 4) rounded up to a power of two (<= 64); lane j of the group holds the
//             columns 4 (j + G c) .. + 3, c < C = ceil(d / (4 G)) (C = 2 only for 256 < d <= 512).  64 / G rows go per pass: one
//             pass of the wave is ONE contiguous run of (64 / G) d floats, read in 16-byte lanes when d % 4 == 0 and every operand is
//             16-byte aligned (VEC), else one float at a time in the same layout -- so the two paths give the same bits.
//   softmax   every row slot keeps its own online (m, l, acc[4 C]); the slots are merged at the end by a butterfly whose two
//             sides evaluate the SAME expression (the lower lane's state is always the left operand): fixed order, same bits in
//             every lane.  A query-mode score is a group-wide dot by the same butterfly; the backward takes both of its dots
//             (s_i and t_i) from the one load of the row.
//   -inf      a factor exp(m - m') whose m is -inf is taken as exactly 0 (never exp(-inf - -inf) = exp(NaN)): a -inf score is a
//             weight of exactly 0, as first row and as a whole piece.  A segment whose scores are all -inf ends with l = 0 and
//             gives 0 / 0 = NaN; a +inf gives exp(inf - inf), a NaN score goes through exp: NaN in that segment's rows only.
//   long      a piece of a multi-piece segment (part >= 0) writes its (m, l, acc) -- in the backward its partial d q -- to the
//             workspace at `part`; a merge kernel, one workgroup per long segment, combines them: the segment's parts in sixteen
//             consecutive runs, one per wave, each run in part order, then the sixteen runs in order; lanes over columns.  Fixed
//             order, no atomics.  The launcher skips the merge launch when the plan has no long segment.
// Addresses are int64 (row * d).  Every loop is bounded by the piece's rows, d, or a table count; a table entry that does not
// fit its segment, the row count or the part count is skipped, so a bad table reads and writes nothing outside the operands.
#include "common.hpp"

#include <cmath>

// Every multiply-add below is written out (fmaf) and the compiler forms none of its own: the 16-byte and the one-float
// instantiations of a kernel then round alike, which is what makes their results the same bits.
#pragma clang fp contract(off)

namespace pglamd {
namespace {

constexpr int kReadoutMaxD = 512;
constexpr int64_t kReadoutGridCap = 256 * 8;        // workgroups per launch; the kernels stride beyond it
constexpr int kMergeBlock = 1024;                   // the merge kernel: one workgroup of 16 waves per long segment (a graph of 2^20 rows
constexpr int kMergeWaves = kMergeBlock / kWave;    // has 4096 parts: 256 per wave, read eight at a time)

struct ReadoutArgs {
    const float* x; const float* opnd;               // opnd: score [N] (gate) or q [S, d] (query)
    const int64_t* seg_ptr; const int64_t* pieces; const int64_t* longs;
    int64_t num_rows, num_segments, num_pieces, num_long, num_parts;
    int d, g_shift;
    float* out; float* stats;                        // forward: written; backward: read
    const float* grad_out; float* grad_x; float* grad_opnd;     // backward only (grad_x / grad_opnd NULL: not stored)
    float* ws_stats; float* ws_rows;                 // [parts, 2], [parts, d]
};

struct Piece { int64_t seg, row0, part; int len; bool ok; };

// Entry p of the piece table, checked against everything it indexes (wave-uniform: table values only).
__device__ __forceinline__ Piece load_piece(const ReadoutArgs& a, int64_t p) {
    Piece r;
    r.seg = a.pieces[4 * p]; r.row0 = a.pieces[4 * p + 1]; r.part = a.pieces[4 * p + 3];
    const int64_t len = a.pieces[4 * p + 2];
    r.len = 0;
    r.ok = r.seg >= 0 && r.seg < a.num_segments && len >= 0 && len <= PGLAMD_READOUT_PIECE && r.part >= -1 && r.part < a.num_parts;
    if (r.ok) {
        const int64_t b = a.seg_ptr[r.seg], e = a.seg_ptr[r.seg + 1];
        r.ok = r.row0 >= 0 && r.row0 >= b && r.row0 + len <= e && e <= a.num_rows;
        r.len = (int)len;
    }
    return r;
}

template <bool VEC> __device__ __forceinline__ float4 load4(const float* row, int col, int d) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (VEC) {
        if (col < d) v = *reinterpret_cast<const float4*>(row + col);
    } else {
        if (col < d) v.x = row[col];
        if (col + 1 < d) v.y = row[col + 1];
        if (col + 2 < d) v.z = row[col + 2];
        if (col + 3 < d) v.w = row[col + 3];
    }
    return v;
}

template <bool VEC> __device__ __forceinline__ void store4(float* row, int col, int d, float4 v) {
    if (VEC) {
        if (col < d) *reinterpret_cast<float4*>(row + col) = v;
    } else {
        if (col < d) row[col] = v.x;
        if (col + 1 < d) row[col + 1] = v.y;
        if (col + 2 < d) row[col + 2] = v.z;
        if (col + 3 < d) row[col + 3] = v.w;
    }
}

template <int C, bool VEC> __device__ __forceinline__ void load_row(float4 (&v)[C], const float* row, int j, int g_shift, int d) {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = load4<VEC>(row, 4 * (j + (c << g_shift)), d);
}

template <int C, bool VEC> __device__ __forceinline__ void store_row(float* row, int j, int g_shift, int d, const float4 (&v)[C]) {
#pragma unroll
    for (int c = 0; c < C; ++c) store4<VEC>(row, 4 * (j + (c << g_shift)), d, v[c]);
}

// <a, b> over the group's row: the lane's own columns in a fixed order, then a butterfly over the group (a + b == b + a bit for
// bit, so every lane of the group ends with the same value).
template <int C> __device__ __forceinline__ float group_dot(const float4 (&a)[C], const float4 (&b)[C], int G) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) s = fmaf(a[c].w, b[c].w, fmaf(a[c].z, b[c].z, fmaf(a[c].y, b[c].y, fmaf(a[c].x, b[c].x, s))));
    for (int off = 1; off < G; off <<= 1) s += __shfl_xor(s, off, kWave);
    return s;
}

__device__ __forceinline__ float4 shfl_xor4(float4 v, int off) {
    return make_float4(__shfl_xor(v.x, off, kWave), __shfl_xor(v.y, off, kWave), __shfl_xor(v.z, off, kWave), __shfl_xor(v.w, off, kWave));
}

// exp(m - m_new), exactly 0 for m = -inf (where m_new may be -inf too)
__device__ __forceinline__ float rescale(float m, float m_new) { return m == -INFINITY ? 0.f : expf(m - m_new); }

__device__ __forceinline__ float4 axpby(float fa, float4 a, float fb, float4 b) {
    return make_float4(fmaf(a.x, fa, b.x * fb), fmaf(a.y, fa, b.y * fb), fmaf(a.z, fa, b.z * fb), fmaf(a.w, fa, b.w * fb));
}

// a + f b
__device__ __forceinline__ float4 axpy(float4 a, float f, float4 b) {
    return make_float4(fmaf(b.x, f, a.x), fmaf(b.y, f, a.y), fmaf(b.z, f, a.z), fmaf(b.w, f, a.w));
}

template <int C, bool VEC, bool QUERY>
__global__ __launch_bounds__(kBlock) void readout_forward_kernel(ReadoutArgs a) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int G = 1 << a.g_shift, j = lane & (G - 1), slot = lane >> a.g_shift, R = kWave >> a.g_shift, d = a.d;
    for (int64_t p = (int64_t)blockIdx.x * kWavesPerBlock + wave; p < a.num_pieces; p += (int64_t)gridDim.x * kWavesPerBlock) {
        const Piece pc = load_piece(a, p);
        if (!pc.ok) continue;
        float4 q[C], acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = q[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (QUERY) load_row<C, VEC>(q, a.opnd + pc.seg * (int64_t)d, j, a.g_shift, d);
        float m = -INFINITY, l = 0.f;
        const int passes = (pc.len + R - 1) >> (6 - a.g_shift);
#pragma unroll 2
        for (int t = 0; t < passes; ++t) {
            const int r = t * R + slot;
            const bool valid = r < pc.len;
            const int64_t row = pc.row0 + (valid ? r : pc.len - 1);          // (passes > 0 only when len > 0)
            float4 xv[C];
            load_row<C, VEC>(xv, a.x + row * (int64_t)d, j, a.g_shift, d);
            const float s = QUERY ? group_dot<C>(xv, q, G) : a.opnd[row];
            if (valid) {
                const float m_new = fmaxf(m, s);
                const float f = rescale(m, m_new), w = rescale(s, m_new);     // (a NaN or +inf score: w = NaN)
                l = fmaf(l, f, w);
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = axpby(f, acc[c], w, xv[c]);
                m = m_new;
            }
        }
        for (int off = G; off < kWave; off <<= 1) {                          // the row slots, lower lane's state on the left
            const float mo = __shfl_xor(m, off, kWave), lo = __shfl_xor(l, off, kWave);
            const bool up = lane & off;
            const float ma = up ? mo : m, mb = up ? m : mo, la = up ? lo : l, lb = up ? l : lo;
            const float m_new = fmaxf(ma, mb);
            const float fa = rescale(ma, m_new), fb = rescale(mb, m_new);
            l = fmaf(la, fa, lb * fb);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float4 o = shfl_xor4(acc[c], off);
                acc[c] = axpby(fa, up ? o : acc[c], fb, up ? acc[c] : o);
            }
            m = m_new;
        }
        if (slot != 0) continue;
        if (pc.part >= 0) {
            if (j == 0) { a.ws_stats[2 * pc.part] = m; a.ws_stats[2 * pc.part + 1] = l; }
            store_row<C, VEC>(a.ws_rows + pc.part * (int64_t)d, j, a.g_shift, d, acc);
        } else {
            if (pc.len > 0) {
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = make_float4(acc[c].x / l, acc[c].y / l, acc[c].z / l, acc[c].w / l);
            }
            if (j == 0) { a.stats[2 * pc.seg] = m; a.stats[2 * pc.seg + 1] = l; }
            store_row<C, VEC>(a.out + pc.seg * (int64_t)d, j, a.g_shift, d, acc);
        }
    }
}

template <int C, bool VEC, bool QUERY>
__global__ __launch_bounds__(kBlock) void readout_backward_kernel(ReadoutArgs a) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int G = 1 << a.g_shift, j = lane & (G - 1), slot = lane >> a.g_shift, R = kWave >> a.g_shift, d = a.d;
    for (int64_t p = (int64_t)blockIdx.x * kWavesPerBlock + wave; p < a.num_pieces; p += (int64_t)gridDim.x * kWavesPerBlock) {
        const Piece pc = load_piece(a, p);
        if (!pc.ok) continue;
        float4 go[C], q[C], dq[C];
#pragma unroll
        for (int c = 0; c < C; ++c) dq[c] = q[c] = make_float4(0.f, 0.f, 0.f, 0.f);
        load_row<C, VEC>(go, a.grad_out + pc.seg * (int64_t)d, j, a.g_shift, d);
        if (QUERY) load_row<C, VEC>(q, a.opnd + pc.seg * (int64_t)d, j, a.g_shift, d);
        float cg;
        {
            float4 o[C];
            load_row<C, VEC>(o, a.out + pc.seg * (int64_t)d, j, a.g_shift, d);
            cg = group_dot<C>(go, o, G);
        }
        const float m = a.stats[2 * pc.seg], l = a.stats[2 * pc.seg + 1];
        const int passes = (pc.len + R - 1) >> (6 - a.g_shift);
#pragma unroll 2
        for (int t = 0; t < passes; ++t) {
            const int r = t * R + slot;
            const bool valid = r < pc.len;
            const int64_t row = pc.row0 + (valid ? r : pc.len - 1);
            float4 xv[C];
            load_row<C, VEC>(xv, a.x + row * (int64_t)d, j, a.g_shift, d);
            const float ti = group_dot<C>(go, xv, G);
            const float s = QUERY ? group_dot<C>(xv, q, G) : a.opnd[row];     // (the forward's expression: the same bits)
            if (valid) {
                const float ai = expf(s - m) / l;
                const float ds = ai * (ti - cg);
                if (a.grad_x) {
                    float4 dx[C];
#pragma unroll
                    for (int c = 0; c < C; ++c) dx[c] = QUERY ? axpby(ai, go[c], ds, q[c]) : make_float4(ai * go[c].x, ai * go[c].y, ai * go[c].z, ai * go[c].w);
                    store_row<C, VEC>(a.grad_x + row * (int64_t)d, j, a.g_shift, d, dx);
                }
                if (QUERY) {
#pragma unroll
                    for (int c = 0; c < C; ++c) dq[c] = axpy(dq[c], ds, xv[c]);
                } else if (a.grad_opnd && j == 0) {
                    a.grad_opnd[row] = ds;
                }
            }
        }
        if (!QUERY || !a.grad_opnd) continue;
        for (int off = G; off < kWave; off <<= 1) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float4 o = shfl_xor4(dq[c], off);
                dq[c] = make_float4(dq[c].x + o.x, dq[c].y + o.y, dq[c].z + o.z, dq[c].w + o.w);
            }
        }
        if (slot != 0) continue;
        float* dst = pc.part >= 0 ? a.ws_rows + pc.part * (int64_t)d : a.grad_opnd + pc.seg * (int64_t)d;
        store_row<C, VEC>(dst, j, a.g_shift, d, dq);
    }
}

// One workgroup per long segment.  SOFTMAX: out[seg] / stats[seg] from the parts' (m, l, acc); else dst[seg] = the sum of the
// parts' rows (d q).  Wave w takes the w-th run of ceil(n / 16) consecutive parts, in order; the sixteen runs are then
// combined in order.  Every condition around a barrier depends on the table alone: uniform over the workgroup.
template <bool SOFTMAX>
__global__ __launch_bounds__(kMergeBlock) void readout_merge_kernel(ReadoutArgs a, float* dst) {
    __shared__ float s_rows[kMergeWaves][kReadoutMaxD];
    __shared__ float s_m[kMergeWaves], s_l[kMergeWaves];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6, d = a.d;
    for (int64_t i = blockIdx.x; i < a.num_long; i += gridDim.x) {
        const int64_t seg = a.longs[3 * i], p0 = a.longs[3 * i + 1], n = a.longs[3 * i + 2];
        if (seg < 0 || seg >= a.num_segments || p0 < 0 || n < 1 || n > a.num_parts || p0 > a.num_parts - n) continue;
        float M = -INFINITY;
        if (SOFTMAX) {
            for (int64_t k = threadIdx.x; k < n; k += kMergeBlock) M = fmaxf(M, a.ws_stats[2 * (p0 + k)]);
            for (int off = 1; off < kWave; off <<= 1) M = fmaxf(M, __shfl_xor(M, off, kWave));      // (max is exact: any order)
            if (lane == 0) s_m[wave] = M;
            __syncthreads();
            for (int w = 0; w < kMergeWaves; ++w) M = fmaxf(M, s_m[w]);
        }
        const int64_t run = (n + kMergeWaves - 1) / kMergeWaves;
        const int64_t k0 = wave * run < n ? wave * run : n, k1 = k0 + run < n ? k0 + run : n;
        float lsum = 0.f, acc[kReadoutMaxD / kWave];
#pragma unroll
        for (int c = 0; c < kReadoutMaxD / kWave; ++c) acc[c] = 0.f;
#pragma unroll 8
        for (int64_t k = k0; k < k1; ++k) {
            float f = 1.f;
            if (SOFTMAX) {
                f = rescale(a.ws_stats[2 * (p0 + k)], M);
                lsum = fmaf(a.ws_stats[2 * (p0 + k) + 1], f, lsum);
            }
            const float* row = a.ws_rows + (p0 + k) * (int64_t)d;
#pragma unroll
            for (int c = 0; c < kReadoutMaxD / kWave; ++c) {
                const int col = lane + c * kWave;
                if (col < d) acc[c] = fmaf(row[col], f, acc[c]);
            }
        }
#pragma unroll
        for (int c = 0; c < kReadoutMaxD / kWave; ++c) s_rows[wave][lane + c * kWave] = acc[c];
        if (lane == 0) s_l[wave] = lsum;
        __syncthreads();
        float L = 0.f;
        if (SOFTMAX) {
            for (int w = 0; w < kMergeWaves; ++w) L += s_l[w];
            if (threadIdx.x == 0) { a.stats[2 * seg] = M; a.stats[2 * seg + 1] = L; }
        }
        for (int col = threadIdx.x; col < d; col += kMergeBlock) {
            float v = 0.f;
            for (int w = 0; w < kMergeWaves; ++w) v += s_rows[w][col];
            dst[seg * (int64_t)d + col] = SOFTMAX ? v / L : v;
        }
        __syncthreads();                                                     // (the LDS rows are rewritten by the next segment)
    }
}

unsigned capped_grid(int64_t work_items) {
    const int64_t g = work_items > 0 ? work_items : 1;
    return (unsigned)(g < kReadoutGridCap ? g : kReadoutGridCap);
}

int group_shift(int64_t d) {            // G = ceil(d / 4) rounded up to a power of two, at most 64
    int s = 0;
    while (s < 6 && (4ll << s) < d) ++s;
    return s;
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct ReadoutWs {
    float* stats; float* rows; bool ok;
    ReadoutWs(void* ws, size_t bytes, int64_t parts, int64_t d) {
        Carver cv(ws, bytes);
        stats = cv.take<float>((size_t)(parts > 0 ? parts : 1) * 2);
        rows = cv.take<float>((size_t)(parts > 0 ? parts : 1) * (size_t)d);
        ok = cv.ok();
    }
};

template <bool BACKWARD, int C, bool VEC>
void launch_pieces(const ReadoutArgs& a, bool query, hipStream_t st) {
    const dim3 grid(capped_grid(ceil_div(a.num_pieces, kWavesPerBlock))), block(kBlock);
    if (BACKWARD) {
        if (query) hipLaunchKernelGGL((readout_backward_kernel<C, VEC, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((readout_backward_kernel<C, VEC, false>), grid, block, 0, st, a);
    } else {
        if (query) hipLaunchKernelGGL((readout_forward_kernel<C, VEC, true>), grid, block, 0, st, a);
        else hipLaunchKernelGGL((readout_forward_kernel<C, VEC, false>), grid, block, 0, st, a);
    }
}

template <bool BACKWARD>
void launch_pieces(const ReadoutArgs& a, bool query, bool vec, hipStream_t st) {
    const bool two = a.d > 4 * kWave;
    if (two) { if (vec) launch_pieces<BACKWARD, 2, true>(a, query, st); else launch_pieces<BACKWARD, 2, false>(a, query, st); }
    else     { if (vec) launch_pieces<BACKWARD, 1, true>(a, query, st); else launch_pieces<BACKWARD, 1, false>(a, query, st); }
}

// The checks both entry points share; fills the table half of `a`.
int32_t readout_common(const char* what, ReadoutArgs& a, const float* x, int64_t num_rows, int64_t d, int32_t mode, const float* opnd,
                       const int64_t* seg_ptr, int64_t num_segments, const int64_t* pieces, int64_t num_pieces, const int64_t* long_segs,
                       int64_t num_long, int64_t num_long_pieces, void* workspace, size_t workspace_bytes) {
    if (d < 1 || d > kReadoutMaxD) return fail(PGLAMD_E_ARG, "%s: d = %lld outside [1, %d]", what, (long long)d, kReadoutMaxD);
    if (mode != PGLAMD_READOUT_GATE && mode != PGLAMD_READOUT_QUERY) return fail(PGLAMD_E_ARG, "%s: mode must be 0 (gate) or 1 (query)", what);
    if (num_rows < 0 || num_segments < 1 || num_pieces < num_segments || num_long < 0 || num_long_pieces < 0 || num_long > num_long_pieces)
        return fail(PGLAMD_E_ARG, "%s: bad counts (rows >= 0, segments >= 1, pieces >= segments, 0 <= long segments <= long pieces)", what);
    if (!seg_ptr || !pieces || (num_long > 0 && !long_segs) || (num_rows > 0 && (!x || (mode == PGLAMD_READOUT_GATE && !opnd))) ||
        (mode == PGLAMD_READOUT_QUERY && !opnd))
        return fail(PGLAMD_E_ARG, "%s: NULL operand", what);
    if (num_long > 0) {
        if (!workspace || workspace_bytes < pglamd_attention_readout_workspace_bytes(num_long_pieces, d))
            return fail(PGLAMD_E_WORKSPACE, "%s: workspace too small", what);
        ReadoutWs ws(workspace, workspace_bytes, num_long_pieces, d);
        if (!ws.ok) return fail(PGLAMD_E_WORKSPACE, "%s: workspace too small", what);
        a.ws_stats = ws.stats; a.ws_rows = ws.rows;
    } else {
        a.ws_stats = a.ws_rows = nullptr;
        num_long_pieces = 0;                          // no part of the table may point into a workspace that is not there
    }
    a.x = x; a.opnd = opnd; a.seg_ptr = seg_ptr; a.pieces = pieces; a.longs = long_segs;
    a.num_rows = num_rows; a.num_segments = num_segments; a.num_pieces = num_pieces; a.num_long = num_long; a.num_parts = num_long_pieces;
    a.d = (int)d; a.g_shift = group_shift(d);
    return PGLAMD_OK;
}

}  // namespace
}  // namespace pglamd

using namespace pglamd;

extern "C" size_t pglamd_attention_readout_workspace_bytes(int64_t num_long_pieces, int64_t d) {
    if (num_long_pieces < 0 || d < 1 || d > kReadoutMaxD) return 0;
    const size_t parts = (size_t)(num_long_pieces > 0 ? num_long_pieces : 1);
    return align_up(parts * 2 * sizeof(float), 256) + align_up(parts * (size_t)d * sizeof(float), 256) + 256;
}

extern "C" int32_t pglamd_attention_readout(const float* x, int64_t num_rows, int64_t d, int32_t mode, const float* operand,
                                            const int64_t* seg_ptr, int64_t num_segments, const int64_t* pieces, int64_t num_pieces,
                                            const int64_t* long_segs, int64_t num_long, int64_t num_long_pieces, float* out, float* stats,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    ReadoutArgs a{};
    PGLAMD_TRY(readout_common("attention_readout", a, x, num_rows, d, mode, operand, seg_ptr, num_segments, pieces, num_pieces, long_segs,
                              num_long, num_long_pieces, workspace, workspace_bytes));
    if (!out || !stats) return fail(PGLAMD_E_ARG, "attention_readout: out / stats NULL");
    a.out = out; a.stats = stats;
    const bool query = mode == PGLAMD_READOUT_QUERY;
    const bool vec = d % 4 == 0 && aligned16(x) && aligned16(out) && aligned16(a.ws_rows) && (!query || aligned16(operand));
    hipStream_t st = static_cast<hipStream_t>(stream);
    launch_pieces<false>(a, query, vec, st);
    PGLAMD_LAUNCH_CHECK();
    if (num_long > 0) {
        hipLaunchKernelGGL((readout_merge_kernel<true>), dim3(capped_grid(num_long)), dim3(kMergeBlock), 0, st, a, out);
        PGLAMD_LAUNCH_CHECK();
    }
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_attention_readout_backward(const float* grad_out, const float* x, int64_t num_rows, int64_t d, int32_t mode,
                                                     const float* operand, const float* out, const float* stats, const int64_t* seg_ptr,
                                                     int64_t num_segments, const int64_t* pieces, int64_t num_pieces,
                                                     const int64_t* long_segs, int64_t num_long, int64_t num_long_pieces, int32_t need_x,
                                                     int32_t need_operand, float* grad_x, float* grad_operand, void* workspace,
                                                     size_t workspace_bytes, void* stream) {
    ReadoutArgs a{};
    PGLAMD_TRY(readout_common("attention_readout_backward", a, x, num_rows, d, mode, operand, seg_ptr, num_segments, pieces, num_pieces,
                              long_segs, num_long, num_long_pieces, workspace, workspace_bytes));
    const bool query = mode == PGLAMD_READOUT_QUERY;
    if (!grad_out || !out || !stats) return fail(PGLAMD_E_ARG, "attention_readout_backward: grad_out / out / stats NULL");
    if ((need_x && num_rows > 0 && !grad_x) || (need_operand && !grad_operand && (query || num_rows > 0)))
        return fail(PGLAMD_E_ARG, "attention_readout_backward: a gradient that is needed has no buffer");
    if (!need_x && !need_operand) return fail(PGLAMD_E_ARG, "attention_readout_backward: no gradient is needed");
    a.out = const_cast<float*>(out); a.stats = const_cast<float*>(stats);       // (read only in the backward kernels)
    a.grad_out = grad_out; a.grad_x = need_x ? grad_x : nullptr; a.grad_opnd = need_operand ? grad_operand : nullptr;
    const bool vec = d % 4 == 0 && aligned16(x) && aligned16(out) && aligned16(grad_out) && aligned16(a.grad_x) && aligned16(a.ws_rows) &&
                     (!query || (aligned16(operand) && aligned16(a.grad_opnd)));
    hipStream_t st = static_cast<hipStream_t>(stream);
    launch_pieces<true>(a, query, vec, st);
    PGLAMD_LAUNCH_CHECK();
    if (query && a.grad_opnd && num_long > 0) {
        hipLaunchKernelGGL((readout_merge_kernel<false>), dim3(capped_grid(num_long)), dim3(kMergeBlock), 0, st, a, a.grad_opnd);
        PGLAMD_LAUNCH_CHECK();
    }
    return PGLAMD_OK;
}
