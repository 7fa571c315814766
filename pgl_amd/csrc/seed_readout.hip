// seed_readout.hip -- the pooling attention of GraphMultisetTransformer (PMA: pgl/nn/gmt_pool.py:160-199 over MAB, :28-112) as one
// streaming pass over CONTIGUOUS rows: k learned seeds, shared by all graphs, attend over each graph's nodes, and the softmax runs over
// the SEED axis (pgl/nn/gmt_pool.py:97-100).  The weights of a node therefore depend on that node alone: no running maximum, no
// per-segment statistics, nothing saved for the backward -- what is left is a segment sum of k weighted copies of each V row.
//
//   s[n,j,h] = key_bias[n] + scale <Q[j, head h], K[n, head h]>           head h = columns h hd .. (h + 1) hd - 1, hd = dim / H
//   A[n,j,h] = exp(s[n,j,h] - max_j' s[n,j',h]) / sum_j' exp(s[n,j',h] - max_j')
//   out[g,j, head h] = residual Q[j, head h] + sum_{n in g} A[n,j,h] V[n, head h]          an empty graph: out[g] = residual Q
// backward from G = d out, A recomputed by the forward's own expression (the same bits), t[n,j,h] = <G[g,j, head h], V[n, head h]>,
// ds[n,j,h] = A (t - sum_j' A[n,j',h] t[n,j',h]):
//   dV[n] = sum_j A G[g,j]    dK[n] = scale sum_j ds Q[j]    dQ[j] = residual sum_g G[g,j] + scale sum_n ds K[n]    d key_bias[n] = sum_{j,h} ds
//
// Unit of work: a PIECE of the read-out plan (readout.hip; pgl_amd/readout_ops.py: host_pieces), one wave64 per piece.
//   lanes    a group of Gl = pow2(dim / 4) lanes owns a row, lane jl of it the 16-byte column quad 4 jl .. 4 jl + 3 (lanes past dim idle:
//            dim = 12, 24, 48, ...); 64 / Gl rows go per pass.  A head is hd / 4 consecutive lanes, so the per-head dots are butterflies
//            over those lanes only, both sides evaluating the same sum: every lane of a head holds the same score, and no LDS round
//            trip happens per row.
//   seeds    compile-time tiers KT = 1 / 4 / 8 / 16 / 32; a seed j >= k of the tier has the weight exactly 0 and is never read or
//            written.  A lane keeps KT weights and KT float4 accumulators in VGPRs (128 floats at the top tier: why k stops at 32).
//   Q        staged in LDS once per workgroup (<= 32 KiB), one barrier before the piece loop, read from LDS per row.
//   G        (backward) the piece's graph's cotangent [k, dim] in a per-wave LDS tile, loaded when the piece opens: Q and four tiles
//            are 5 k dim 4 bytes <= 160 KiB.
//   end      the 64 / Gl row slots are added by a butterfly (a + b == b + a bit for bit); the piece writes out[g] (residual added
//            there) or its partial [k, dim] to the workspace at `part`; one merge launch, only when the plan has a long segment,
//            adds a segment's parts in sixteen consecutive runs, each in part order, then the runs in order, then the residual.
//   dQ       W = min(num_pieces, 1024) waves; wave w walks the pieces w, w + W, ... and carries d Q in registers, writes one partial
//            [k, dim]; a second launch adds the W partials (sixteen runs, in order) and residual sum_g G[g] (the same way, in g
//            order).  W is part of the definition of the bits and does not depend on the device.
// No atomics; every multiply-add is written out (fmaf) and the compiler forms none: results are a pure function of the arguments,
// bit for bit, and a gradient's bits do not depend on which other gradients were asked for.  Addresses are int64; every loop is
// bounded by the piece's rows or a table count; a table entry that does not fit its segment, num_rows or num_long_pieces is skipped.
#include "common.hpp"

#include <cmath>

#pragma clang fp contract(off)

namespace pglamd {
namespace {

constexpr int kSeedMaxK = 32;
constexpr int kSeedMinDim = 4, kSeedMaxDim = 256;
constexpr int64_t kSeedGridCap = 256 * 8;           // workgroups per forward launch; the kernel strides beyond it
constexpr int kSeedDqWaves = 1024;                  // W: the waves of a backward launch (fixed: it orders the d Q sum)
constexpr int kSumRuns = 16, kSumCols = 64;         // the ordered-sum kernels: sixteen runs of items over 64 columns per workgroup
constexpr int kSumBlock = kSumRuns * kSumCols;
constexpr size_t kSeedLdsMax = 160 * 1024;

struct SeedArgs {
    const float* K; const float* V; const float* Q; const float* bias;         // bias NULL: nothing is added
    const int64_t* seg_ptr; const int64_t* pieces; const int64_t* longs;
    int64_t num_rows, num_segments, num_pieces, num_long, num_parts;
    int k, dim, g_shift, head_lanes, residual, dq_waves;
    float scale;
    float* out; float* ws;                           // ws: forward [parts, k, dim]; backward [dq_waves, k, dim]
    const float* grad_out; float* grad_K; float* grad_V; float* grad_Q; float* grad_bias;     // a NULL gradient is not stored
};

struct Piece { int64_t seg, row0, part; int len; bool ok; };

// Entry p of the piece table, checked against everything it indexes (wave-uniform: table values only).
__device__ __forceinline__ Piece load_piece(const SeedArgs& a, int64_t p) {
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

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ float4 shfl_xor4(float4 v, int off) {
    return make_float4(__shfl_xor(v.x, off, kWave), __shfl_xor(v.y, off, kWave), __shfl_xor(v.z, off, kWave), __shfl_xor(v.w, off, kWave));
}

// a + f b
__device__ __forceinline__ float4 axpy(float4 a, float f, float4 b) {
    return make_float4(fmaf(b.x, f, a.x), fmaf(b.y, f, a.y), fmaf(b.z, f, a.z), fmaf(b.w, f, a.w));
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// d[j] = <m[j, head of this lane], v[head of this lane]>, j < k: the lane's quad in a fixed order, then a butterfly over the head's
// lanes (every lane of the head ends with the same bits).  m: the lane's column of a [k, dim] matrix in LDS, rows dq4 float4 apart.
template <int KT>
__device__ __forceinline__ void head_dots(float (&d)[KT], const float4* m, int dq4, float4 v, int k, int head_lanes) {
#pragma unroll
    for (int j = 0; j < KT; ++j) {
        d[j] = 0.f;
        if (j < k) {
            const float4 q = m[j * dq4];
            d[j] = fmaf(q.w, v.w, fmaf(q.z, v.z, fmaf(q.y, v.y, q.x * v.x)));
        }
    }
    for (int off = 1; off < head_lanes; off <<= 1) {
#pragma unroll
        for (int j = 0; j < KT; ++j)
            if (j < k) d[j] += __shfl_xor(d[j], off, kWave);
    }
}

// The raw dots d[j] -> the softmax over the k seeds of bias + scale d[j]; a seed j >= k of the tier: exactly 0.
template <int KT>
__device__ __forceinline__ void seed_softmax(float (&d)[KT], float bias, float scale, int k) {
    float m = -INFINITY, l = 0.f;
#pragma unroll
    for (int j = 0; j < KT; ++j)
        if (j < k) { d[j] = fmaf(scale, d[j], bias); m = fmaxf(m, d[j]); }
#pragma unroll
    for (int j = 0; j < KT; ++j)
        if (j < k) { d[j] = expf(d[j] - m); l += d[j]; }
    const float inv = 1.f / l;
#pragma unroll
    for (int j = 0; j < KT; ++j) d[j] = j < k ? d[j] * inv : 0.f;
}

// Q [k, dim] -> LDS, by the whole workgroup; the caller's barrier follows.
__device__ __forceinline__ void stage_q(float4* s_q, const SeedArgs& a) {
    const float4* src = reinterpret_cast<const float4*>(a.Q);
    for (int i = threadIdx.x; i < a.k * (a.dim >> 2); i += blockDim.x) s_q[i] = src[i];
}

template <int KT>
__global__ __launch_bounds__(kBlock) void seed_forward_kernel(SeedArgs a) {
    __shared__ float4 s_q[KT * kSeedMaxDim / 4];
    stage_q(s_q, a);
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int G = 1 << a.g_shift, jl = lane & (G - 1), slot = lane >> a.g_shift, R = kWave >> a.g_shift;
    const int dim = a.dim, k = a.k, dq4 = dim >> 2;
    const bool col_ok = jl < dq4;
    const float4* q = s_q + (col_ok ? jl : 0);
    const int64_t kd = (int64_t)k * dim;
    for (int64_t p = (int64_t)blockIdx.x * kWavesPerBlock + wave; p < a.num_pieces; p += (int64_t)gridDim.x * kWavesPerBlock) {
        const Piece pc = load_piece(a, p);
        if (!pc.ok) continue;
        float4 acc[KT];
#pragma unroll
        for (int j = 0; j < KT; ++j) acc[j] = zero4();
        const int passes = (pc.len + R - 1) >> (6 - a.g_shift);
        for (int t = 0; t < passes; ++t) {
            const int r = t * R + slot;
            const bool valid = r < pc.len;
            const int64_t row = pc.row0 + (valid ? r : pc.len - 1);          // (passes > 0 only when len > 0)
            float4 kv = zero4(), vv = zero4();
            if (col_ok) {
                kv = *reinterpret_cast<const float4*>(a.K + row * (int64_t)dim + 4 * jl);
                if (valid) vv = *reinterpret_cast<const float4*>(a.V + row * (int64_t)dim + 4 * jl);
            }
            const float b = a.bias ? a.bias[row] : 0.f;
            float w[KT];
            head_dots<KT>(w, q, dq4, kv, k, a.head_lanes);
            seed_softmax<KT>(w, b, a.scale, k);
#pragma unroll
            for (int j = 0; j < KT; ++j)
                if (j < k) acc[j] = axpy(acc[j], w[j], vv);                  // (a slot past the piece's end adds w * 0)
        }
        for (int off = G; off < kWave; off <<= 1) {                          // the row slots
#pragma unroll
            for (int j = 0; j < KT; ++j)
                if (j < k) acc[j] = add4(acc[j], shfl_xor4(acc[j], off));
        }
        if (slot != 0 || !col_ok) continue;
        float* dst = pc.part >= 0 ? a.ws + pc.part * kd : a.out + pc.seg * kd;
        const bool res = pc.part < 0 && a.residual;
#pragma unroll
        for (int j = 0; j < KT; ++j)
            if (j < k) *reinterpret_cast<float4*>(dst + j * dim + 4 * jl) = res ? add4(q[j * dq4], acc[j]) : acc[j];
    }
}

// One wave per piece again, but wave w of the launch's dq_waves walks the pieces w, w + dq_waves, ...: its d Q stays in registers.
// LDS: Q, then one [k, dim] tile per wave for the cotangent of the piece's graph.
template <int KT>
__global__ __launch_bounds__(kBlock) void seed_backward_kernel(SeedArgs a) {
    extern __shared__ __align__(16) float4 s_seed[];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int G = 1 << a.g_shift, jl = lane & (G - 1), slot = lane >> a.g_shift, R = kWave >> a.g_shift;
    const int dim = a.dim, k = a.k, dq4 = dim >> 2, kd4 = k * dq4;
    stage_q(s_seed, a);
    __syncthreads();
    const bool col_ok = jl < dq4;
    float4* s_g = s_seed + kd4 * (1 + wave);
    const float4* q = s_seed + (col_ok ? jl : 0);
    const float4* gq = s_g + (col_ok ? jl : 0);
    const int64_t kd = (int64_t)k * dim;
    const int64_t w = (int64_t)blockIdx.x * kWavesPerBlock + wave;
    if (w >= a.dq_waves) return;                                             // (after the only barrier)
    float4 dq[KT];
#pragma unroll
    for (int j = 0; j < KT; ++j) dq[j] = zero4();
    for (int64_t p = w; p < a.num_pieces; p += a.dq_waves) {
        const Piece pc = load_piece(a, p);
        if (!pc.ok) continue;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");               // (the last piece's reads of the tile are done)
        const float4* gsrc = reinterpret_cast<const float4*>(a.grad_out + pc.seg * kd);
        for (int i = lane; i < kd4; i += kWave) s_g[i] = gsrc[i];
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        const int passes = (pc.len + R - 1) >> (6 - a.g_shift);
        for (int t = 0; t < passes; ++t) {
            const int r = t * R + slot;
            const bool valid = r < pc.len;
            const int64_t row = pc.row0 + (valid ? r : pc.len - 1);
            float4 kv = zero4(), vv = zero4();
            if (col_ok) {
                kv = *reinterpret_cast<const float4*>(a.K + row * (int64_t)dim + 4 * jl);
                vv = *reinterpret_cast<const float4*>(a.V + row * (int64_t)dim + 4 * jl);
            }
            const float b = a.bias ? a.bias[row] : 0.f;
            float s[KT], tt[KT];
            head_dots<KT>(s, q, dq4, kv, k, a.head_lanes);                   // (the forward's expressions: the same bits)
            seed_softmax<KT>(s, b, a.scale, k);
            head_dots<KT>(tt, gq, dq4, vv, k, a.head_lanes);
            float c = 0.f;
#pragma unroll
            for (int j = 0; j < KT; ++j)
                if (j < k) c = fmaf(s[j], tt[j], c);
            const float4 kq = valid ? kv : zero4();                          // (a slot past the piece's end adds ds * 0 to d Q)
            float4 dv = zero4(), dk = zero4();
            float dsum = 0.f;
#pragma unroll
            for (int j = 0; j < KT; ++j) {
                if (j < k) {
                    const float ds = s[j] * (tt[j] - c);
                    dv = axpy(dv, s[j], gq[j * dq4]);
                    dk = axpy(dk, ds, q[j * dq4]);
                    if (a.grad_Q) dq[j] = axpy(dq[j], ds, kq);
                    dsum += ds;
                }
            }
            if (valid && col_ok) {
                if (a.grad_V) *reinterpret_cast<float4*>(a.grad_V + row * (int64_t)dim + 4 * jl) = dv;
                if (a.grad_K)
                    *reinterpret_cast<float4*>(a.grad_K + row * (int64_t)dim + 4 * jl) =
                        make_float4(a.scale * dk.x, a.scale * dk.y, a.scale * dk.z, a.scale * dk.w);
            }
            if (a.grad_bias) {                                               // one lane per head carries the head's sum over the seeds
                float x = (col_ok && (jl & (a.head_lanes - 1)) == 0) ? dsum : 0.f;
                for (int off = 1; off < G; off <<= 1) x += __shfl_xor(x, off, kWave);
                if (valid && jl == 0) a.grad_bias[row] = x;
            }
        }
    }
    if (!a.grad_Q) return;
    for (int off = G; off < kWave; off <<= 1) {
#pragma unroll
        for (int j = 0; j < KT; ++j)
            if (j < k) dq[j] = add4(dq[j], shfl_xor4(dq[j], off));
    }
    if (slot != 0 || !col_ok) return;
    float* dst = a.ws + w * kd;
#pragma unroll
    for (int j = 0; j < KT; ++j)
        if (j < k) *reinterpret_cast<float4*>(dst + j * dim + 4 * jl) = dq[j];
}

// sum_{i < n} src[i * stride + e] for this thread's column e (e_ok: inside the row), by the whole workgroup of kSumBlock threads: run r
// (threadIdx / 64) adds the r-th of sixteen consecutive runs of ceil(n / 16) items in order, then every thread adds the sixteen runs
// in order.  n is uniform over the workgroup (it reaches two barriers).
__device__ __forceinline__ float ordered_sum(const float* src, int64_t n, int64_t stride, int64_t e, bool e_ok, float (*s_runs)[kSumCols]) {
    const int run = threadIdx.x >> 6, col = threadIdx.x & (kSumCols - 1);
    const int64_t per = (n + kSumRuns - 1) / kSumRuns;
    const int64_t i0 = run * per < n ? run * per : n, i1 = i0 + per < n ? i0 + per : n;
    float v = 0.f;
    if (e_ok) {
#pragma unroll 8
        for (int64_t i = i0; i < i1; ++i) v += src[i * stride + e];
    }
    s_runs[run][col] = v;
    __syncthreads();
    float t = 0.f;
    for (int r = 0; r < kSumRuns; ++r) t += s_runs[r][col];
    __syncthreads();                                                         // (the runs are rewritten by the next sum)
    return t;
}

// out[seg] = residual Q + the sum of a long segment's parts; one workgroup per (long segment, 64 columns of [k, dim]).
__global__ __launch_bounds__(kSumBlock) void seed_merge_kernel(SeedArgs a) {
    __shared__ float s_runs[kSumRuns][kSumCols];
    const int64_t kd = (int64_t)a.k * a.dim, cblocks = (kd + kSumCols - 1) / kSumCols;
    for (int64_t item = blockIdx.x; item < a.num_long * cblocks; item += gridDim.x) {
        const int64_t i = item / cblocks, e = (item % cblocks) * kSumCols + (threadIdx.x & (kSumCols - 1));
        const int64_t seg = a.longs[3 * i], p0 = a.longs[3 * i + 1], n = a.longs[3 * i + 2];
        if (seg < 0 || seg >= a.num_segments || p0 < 0 || n < 1 || n > a.num_parts || p0 > a.num_parts - n) continue;
        const float v = ordered_sum(a.ws + p0 * kd, n, kd, e, e < kd, s_runs);
        if (threadIdx.x < kSumCols && e < kd) a.out[seg * kd + e] = a.residual ? a.Q[e] + v : v;
    }
}

// d Q = residual sum_g G[g] + scale (the sum of the dq_waves partials); one workgroup per 64 columns of [k, dim].
__global__ __launch_bounds__(kSumBlock) void seed_dq_kernel(SeedArgs a) {
    __shared__ float s_runs[kSumRuns][kSumCols];
    const int64_t kd = (int64_t)a.k * a.dim;
    const int64_t e = (int64_t)blockIdx.x * kSumCols + (threadIdx.x & (kSumCols - 1));
    const float v = ordered_sum(a.ws, a.dq_waves, kd, e, e < kd, s_runs);
    const float g = a.residual ? ordered_sum(a.grad_out, a.num_segments, kd, e, e < kd, s_runs) : 0.f;
    if (threadIdx.x < kSumCols && e < kd) a.grad_Q[e] = fmaf(a.scale, v, g);
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

bool shape_ok(int64_t k, int64_t dim, int64_t heads) {
    if (k < 1 || k > kSeedMaxK || dim < kSeedMinDim || dim > kSeedMaxDim || heads < 1 || dim % heads != 0) return false;
    const int64_t hd = dim / heads;
    return hd >= 4 && (hd & (hd - 1)) == 0;
}

int64_t dq_waves(int64_t num_pieces) { return num_pieces < kSeedDqWaves ? num_pieces : kSeedDqWaves; }

size_t ws_bytes(int64_t num_pieces, int64_t num_long_pieces, int64_t k, int64_t dim) {
    const int64_t slots = std::max<int64_t>(std::max<int64_t>(num_long_pieces, dq_waves(num_pieces)), 1);
    return align_up((size_t)slots * (size_t)k * (size_t)dim * sizeof(float), 256) + 256;
}

// The checks both entry points share; fills everything of `a` but the outputs.
int32_t seed_common(const char* what, SeedArgs& a, const float* K, const float* V, int64_t num_rows, int64_t dim, const float* Q, int64_t k,
                    int64_t heads, const float* key_bias, const int64_t* seg_ptr, int64_t num_segments, const int64_t* pieces,
                    int64_t num_pieces, const int64_t* long_segs, int64_t num_long, int64_t num_long_pieces, void* workspace,
                    size_t workspace_bytes, bool needs_ws) {
    if (!shape_ok(k, dim, heads))
        return fail(PGLAMD_E_ARG, "%s: (k, dim, heads) = (%lld, %lld, %lld) outside 1 <= k <= %d, %d <= dim <= %d, dim %% heads == 0, dim / heads a power of two >= 4",
                    what, (long long)k, (long long)dim, (long long)heads, kSeedMaxK, kSeedMinDim, kSeedMaxDim);
    if (num_rows < 0 || num_segments < 1 || num_pieces < num_segments || num_long < 0 || num_long_pieces < 0 || num_long > num_long_pieces)
        return fail(PGLAMD_E_ARG, "%s: bad counts (rows >= 0, segments >= 1, pieces >= segments, 0 <= long segments <= long pieces)", what);
    if (!seg_ptr || !pieces || !Q || (num_long > 0 && !long_segs) || (num_rows > 0 && (!K || !V))) return fail(PGLAMD_E_ARG, "%s: NULL operand", what);
    if (!aligned16(K) || !aligned16(V) || !aligned16(Q)) return fail(PGLAMD_E_ARG, "%s: K, V and Q must be 16-byte aligned", what);
    a.ws = nullptr;
    if (needs_ws) {
        if (!workspace || workspace_bytes < ws_bytes(num_pieces, num_long_pieces, k, dim)) return fail(PGLAMD_E_WORKSPACE, "%s: workspace too small", what);
        Carver cv(workspace, workspace_bytes);
        a.ws = cv.take<float>((size_t)std::max<int64_t>(std::max<int64_t>(num_long_pieces, dq_waves(num_pieces)), 1) * (size_t)k * (size_t)dim);
        if (!cv.ok()) return fail(PGLAMD_E_WORKSPACE, "%s: workspace too small", what);
    }
    a.K = K; a.V = V; a.Q = Q; a.bias = key_bias;
    a.seg_ptr = seg_ptr; a.pieces = pieces; a.longs = long_segs;
    a.num_rows = num_rows; a.num_segments = num_segments; a.num_pieces = num_pieces; a.num_long = num_long;
    a.num_parts = num_long > 0 ? num_long_pieces : 0;        // no part of the table may point into a workspace that is not there
    a.k = (int)k; a.dim = (int)dim; a.head_lanes = (int)(dim / heads / 4); a.dq_waves = (int)dq_waves(num_pieces);
    a.g_shift = 0;
    while ((4ll << a.g_shift) < dim) ++a.g_shift;
    a.scale = 1.0f / sqrtf((float)dim);
    return PGLAMD_OK;
}

template <int KT> int32_t launch_forward(const SeedArgs& a, hipStream_t st) {
    const int64_t blocks = std::min<int64_t>(ceil_div(a.num_pieces, kWavesPerBlock), kSeedGridCap);
    hipLaunchKernelGGL((seed_forward_kernel<KT>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

template <int KT> int32_t launch_backward(const SeedArgs& a, hipStream_t st) {
    const size_t lds = (size_t)(1 + kWavesPerBlock) * a.k * a.dim * sizeof(float);          // <= 160 KiB
    static bool attr_set = false;                             // (per instantiation; idempotent, so a race only repeats it)
    if (!attr_set) {
        PGLAMD_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&seed_backward_kernel<KT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)kSeedLdsMax));
        attr_set = true;
    }
    hipLaunchKernelGGL((seed_backward_kernel<KT>), dim3((unsigned)ceil_div(a.dq_waves, kWavesPerBlock)), dim3(kBlock), lds, st, a);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}

template <bool BACKWARD> int32_t launch_tier(const SeedArgs& a, hipStream_t st) {
#define PGLAMD_SEED_TIER(KT) return BACKWARD ? launch_backward<KT>(a, st) : launch_forward<KT>(a, st)
    if (a.k <= 1) PGLAMD_SEED_TIER(1);
    if (a.k <= 4) PGLAMD_SEED_TIER(4);
    if (a.k <= 8) PGLAMD_SEED_TIER(8);
    if (a.k <= 16) PGLAMD_SEED_TIER(16);
    PGLAMD_SEED_TIER(32);
#undef PGLAMD_SEED_TIER
}

}  // namespace
}  // namespace pglamd

using namespace pglamd;

extern "C" size_t pglamd_seed_readout_workspace_bytes(int64_t num_pieces, int64_t num_long_pieces, int64_t k, int64_t dim) {
    if (num_pieces < 0 || num_long_pieces < 0 || k < 1 || k > kSeedMaxK || dim < kSeedMinDim || dim > kSeedMaxDim) return 0;
    return ws_bytes(num_pieces, num_long_pieces, k, dim);
}

extern "C" int32_t pglamd_seed_readout(const float* K, const float* V, int64_t num_rows, int64_t dim, const float* Q, int64_t k, int64_t heads,
                                       const float* key_bias, int32_t residual, const int64_t* seg_ptr, int64_t num_segments,
                                       const int64_t* pieces, int64_t num_pieces, const int64_t* long_segs, int64_t num_long,
                                       int64_t num_long_pieces, float* out, void* workspace, size_t workspace_bytes, void* stream) {
    SeedArgs a{};
    PGLAMD_TRY(seed_common("seed_readout", a, K, V, num_rows, dim, Q, k, heads, key_bias, seg_ptr, num_segments, pieces, num_pieces, long_segs,
                           num_long, num_long_pieces, workspace, workspace_bytes, num_long > 0));
    if (!out || !aligned16(out)) return fail(PGLAMD_E_ARG, "seed_readout: out NULL or not 16-byte aligned");
    a.out = out; a.residual = residual != 0;
    hipStream_t st = static_cast<hipStream_t>(stream);
    PGLAMD_TRY(launch_tier<false>(a, st));
    if (num_long > 0) {
        const int64_t items = num_long * ceil_div((int64_t)a.k * a.dim, kSumCols);
        hipLaunchKernelGGL(seed_merge_kernel, dim3((unsigned)std::min<int64_t>(items, kSeedGridCap)), dim3(kSumBlock), 0, st, a);
        PGLAMD_LAUNCH_CHECK();
    }
    return PGLAMD_OK;
}

extern "C" int32_t pglamd_seed_readout_backward(const float* grad_out, const float* K, const float* V, const float* Q, const float* key_bias,
                                                int64_t num_rows, int64_t dim, int64_t k, int64_t heads, int32_t residual,
                                                const int64_t* seg_ptr, int64_t num_segments, const int64_t* pieces, int64_t num_pieces,
                                                const int64_t* long_segs, int64_t num_long, int64_t num_long_pieces, int32_t need_k,
                                                int32_t need_v, int32_t need_q, int32_t need_bias, float* grad_K, float* grad_V,
                                                float* grad_Q, float* grad_bias, void* workspace, size_t workspace_bytes, void* stream) {
    SeedArgs a{};
    PGLAMD_TRY(seed_common("seed_readout_backward", a, K, V, num_rows, dim, Q, k, heads, key_bias, seg_ptr, num_segments, pieces, num_pieces,
                           long_segs, num_long, num_long_pieces, workspace, workspace_bytes, need_q != 0));
    if (!grad_out || !aligned16(grad_out)) return fail(PGLAMD_E_ARG, "seed_readout_backward: grad_out NULL or not 16-byte aligned");
    if (!need_k && !need_v && !need_q && !need_bias) return fail(PGLAMD_E_ARG, "seed_readout_backward: no gradient is needed");
    if ((num_rows > 0 && ((need_k && !grad_K) || (need_v && !grad_V) || (need_bias && !grad_bias))) || (need_q && !grad_Q))
        return fail(PGLAMD_E_ARG, "seed_readout_backward: a gradient that is needed has no buffer");
    if ((need_k && !aligned16(grad_K)) || (need_v && !aligned16(grad_V)))
        return fail(PGLAMD_E_ARG, "seed_readout_backward: grad_K and grad_V must be 16-byte aligned");
    a.grad_out = grad_out; a.residual = residual != 0;
    a.grad_K = need_k ? grad_K : nullptr; a.grad_V = need_v ? grad_V : nullptr;
    a.grad_Q = need_q ? grad_Q : nullptr; a.grad_bias = need_bias ? grad_bias : nullptr;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (num_rows > 0 || need_q) PGLAMD_TRY(launch_tier<true>(a, st));
    if (need_q) {
        hipLaunchKernelGGL(seed_dq_kernel, dim3((unsigned)ceil_div((int64_t)a.k * a.dim, kSumCols)), dim3(kSumBlock), 0, st, a);
        PGLAMD_LAUNCH_CHECK();
    }
    return PGLAMD_OK;
}
