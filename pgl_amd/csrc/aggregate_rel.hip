// aggregate_rel.hip -- relational aggregation: every edge type of a HeterGraph in one launch.  Stands in for the loop of the
// reference's RGCNConv (pgl/nn/conv.py:1014-1019: per edge type one matmul, one send_recv(.., "mean") and one add) on the
// aggregation side; the definition is in include/pgl_amd.h (pglamd_aggregate_relations) and tests/relation_aggregate_defs.py.
//
// The index is the relation-stacked CSR the relation-wise sampler reads (sampling_rel.hip): R indptr rows over ONE col array.
// Work mapping: a GROUP of G lanes owns one destination row; G is the smallest power of two that covers the row's 16-byte units
// (d / 4 float4 on the vector path, d floats on the scalar path), at most a wave.  A 256-byte row (d = 64) is 16 lanes, so one
// wave instruction gathers four source rows -- for four destinations -- and a 512-byte row two; rows wider than 1 KiB are walked
// in column tiles of one wave.  The group walks its R segments in relation order, each segment in edge order with U gathers in
// flight, into registers; it scales the segment (mean: one division by the segment's length) and either adds it to the row total
// (summed output) or stores it as the relation's slice (per-relation output).  One store per output element, no atomic, a fixed
// order: the result is a pure function of the arguments.
//
// Long rows.  No group walks a segment longer than long_row edges: one lane group would serialise a hub's thousands of gathers
// while the rest of its wave idles.  The row kernel skips such segments and a second launch, one workgroup per row that OWNS one
// (the list comes from the caller: built once per index), finishes them: the workgroup's 256 / G groups take fixed contiguous
// slices of the segment, park their partial sums in LDS, group 0 adds them in slice order, scales, and adds into the row (summed
// output: a read-modify-write of a row this workgroup alone owns, after the row kernel on the same stream) or stores the slice.
// Without a list the row kernel walks everything: the caller vouches that no segment is long (max_segment <= long_row).
//
// An edge whose column lies outside [0, x_rows) contributes nothing: the backward pass walks the successor-stacked index of the
// whole graph while the gradient has only out_size rows.
#include "common.hpp"

namespace pglamd {

namespace rel {

// Gathers in flight per group.  The walk is a chain of dependent loads (indptr, col, row) and is bound by how many row loads are
// outstanding, not by registers: 8 (92 VGPRs, 5 waves per SIMD) ran the RMAT-20 full graph 7-9 % faster than 4 (64 VGPRs, 8 waves)
// and 2 ran it 30 % slower (profiles/relation_aggregate/README.md).  -DPGLAMD_REL_UNROLL=n builds another one for such a sweep.
#ifndef PGLAMD_REL_UNROLL
#define PGLAMD_REL_UNROLL 8
#endif
constexpr int kUnroll = PGLAMD_REL_UNROLL;

struct Params {
    const float* x; int64_t x_rows, ldx, x_rel;
    const int64_t* indptr; int64_t ip_rel;
    const int32_t* col;
    const float* cs; int64_t cs_rel;
    int32_t R; int32_t mean;
    int64_t M; int32_t d; int32_t units;        // units = d / VEC
    float* out; int64_t ldo, o_rel;
    int64_t long_row;                           // segments longer than this are left to the long-row kernel (INT64_MAX: none)
    const int64_t* long_rows; int64_t n_long;
    int32_t G, g_shift;                         // lanes per group = 1 << g_shift
};

template <int VEC> struct Acc {
    float v[VEC];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int k = 0; k < VEC; ++k) v[k] = 0.f;
    }
};

template <int VEC> __device__ __forceinline__ Acc<VEC> load_units(const float* p) {
    Acc<VEC> a;
    if constexpr (VEC == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        a.v[0] = t.x; a.v[1] = t.y; a.v[2] = t.z; a.v[3] = t.w;
    } else {
        a.v[0] = *p;
    }
    return a;
}

template <int VEC> __device__ __forceinline__ void store_units(float* p, const Acc<VEC>& a) {
    if constexpr (VEC == 4) *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]);
    else *p = a.v[0];
}

// acc += sum over the edge positions [e0, e1), ascending, of cs[col] * x[col, j .. j + VEC): kUnroll gathers are issued before the
// first add, the adds keep the edge order.
template <int VEC>
__device__ __forceinline__ void walk(const Params& p, int r, int64_t e0, int64_t e1, int64_t j, Acc<VEC>& acc) {
    const float* __restrict__ xr = p.x + (int64_t)r * p.x_rel + j;
    const float* __restrict__ cs = p.cs ? p.cs + (int64_t)r * p.cs_rel : nullptr;
    for (int64_t e = e0; e < e1; e += kUnroll) {
        int32_t c[kUnroll]; bool ok[kUnroll]; Acc<VEC> xv[kUnroll]; float s[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            c[u] = e + u < e1 ? p.col[e + u] : -1;
            ok[u] = c[u] >= 0 && (int64_t)c[u] < p.x_rows;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (ok[u]) {
                xv[u] = load_units<VEC>(xr + (int64_t)c[u] * p.ldx);
                s[u] = cs ? cs[c[u]] : 1.f;
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (ok[u]) {
                if (cs) {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc.v[k] += s[u] * xv[u].v[k];
                } else {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) acc.v[k] += xv[u].v[k];
                }
            }
        }
    }
}

template <int VEC> __device__ __forceinline__ void scale_mean(const Params& p, int64_t len, Acc<VEC>& a) {
    if (p.mean) {
        const float n = (float)len;
#pragma unroll
        for (int k = 0; k < VEC; ++k) a.v[k] /= n;
    }
}

template <int VEC> __global__ __launch_bounds__(kBlock) void rel_rows_kernel(Params p) {
    const int g = threadIdx.x & (p.G - 1);
    const int64_t v = (int64_t)blockIdx.x * (kBlock >> p.g_shift) + (threadIdx.x >> p.g_shift);
    if (v >= p.M) return;
    for (int u0 = 0; u0 < p.units; u0 += p.G) {             // column tiles (one unless the row is wider than a wave)
        const int unit = u0 + g;
        if (unit >= p.units) continue;
        const int64_t j = (int64_t)unit * VEC;
        Acc<VEC> total; total.zero();
        for (int r = 0; r < p.R; ++r) {
            const int64_t* ip = p.indptr + (int64_t)r * p.ip_rel + v;
            const int64_t b = ip[0], len = ip[1] - b;
            Acc<VEC> a; a.zero();
            if (len > 0 && len <= p.long_row) {
                walk<VEC>(p, r, b, b + len, j, a);
                scale_mean<VEC>(p, len, a);
            }
            if (p.o_rel) {
                store_units<VEC>(p.out + v * p.ldo + (int64_t)r * p.o_rel + j, a);
            } else if (len > 0 && len <= p.long_row) {
#pragma unroll
                for (int k = 0; k < VEC; ++k) total.v[k] += a.v[k];
            }
        }
        if (!p.o_rel) store_units<VEC>(p.out + v * p.ldo + j, total);
    }
}

// One workgroup per row that owns a long segment; see the head of the file.
template <int VEC> __global__ __launch_bounds__(kBlock) void rel_long_kernel(Params p) {
    __shared__ float part[kBlock * VEC];                    // [slice][lane of the group][VEC]
    const int64_t v = p.long_rows[blockIdx.x];
    if (v < 0 || v >= p.M) return;                          // (block-uniform)
    const int g = threadIdx.x & (p.G - 1), s = threadIdx.x >> p.g_shift, n_slices = kBlock >> p.g_shift;
    for (int u0 = 0; u0 < p.units; u0 += p.G) {
        const int unit = u0 + g;
        const bool act = unit < p.units;
        const int64_t j = (int64_t)unit * VEC;
        Acc<VEC> total; total.zero();
        bool any = false;
        for (int r = 0; r < p.R; ++r) {
            const int64_t* ip = p.indptr + (int64_t)r * p.ip_rel + v;
            const int64_t b = ip[0], len = ip[1] - b;
            if (len <= p.long_row) continue;                // (block-uniform: every lane reads the same two entries)
            any = true;
            const int64_t per = (len + n_slices - 1) / n_slices;
            const int64_t e0 = b + (int64_t)s * per < b + len ? b + (int64_t)s * per : b + len;
            const int64_t e1 = e0 + per < b + len ? e0 + per : b + len;
            Acc<VEC> a; a.zero();
            if (act) walk<VEC>(p, r, e0, e1, j, a);
#pragma unroll
            for (int k = 0; k < VEC; ++k) part[threadIdx.x * VEC + k] = a.v[k];
            __syncthreads();
            if (s == 0 && act) {
                Acc<VEC> sum; sum.zero();
                for (int q = 0; q < n_slices; ++q)
#pragma unroll
                    for (int k = 0; k < VEC; ++k) sum.v[k] += part[((q << p.g_shift) + g) * VEC + k];
                scale_mean<VEC>(p, len, sum);
                if (p.o_rel) {
                    store_units<VEC>(p.out + v * p.ldo + (int64_t)r * p.o_rel + j, sum);
                } else {
#pragma unroll
                    for (int k = 0; k < VEC; ++k) total.v[k] += sum.v[k];
                }
            }
            __syncthreads();
        }
        if (!p.o_rel && any && s == 0 && act) {
            float* o = p.out + v * p.ldo + j;
            Acc<VEC> cur = load_units<VEC>(o);
#pragma unroll
            for (int k = 0; k < VEC; ++k) cur.v[k] += total.v[k];
            store_units<VEC>(o, cur);
        }
    }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace rel
}  // namespace pglamd

using namespace pglamd;

extern "C" int32_t pglamd_aggregate_relations(const float* x, int64_t x_rows, int64_t x_row_stride, int64_t x_rel_stride,
                                              const int64_t* indptr, int64_t indptr_rel_stride, const int32_t* col,
                                              const float* col_scale, int64_t col_scale_rel_stride, int32_t num_relations,
                                              int64_t out_rows, int64_t d, int32_t reduce_op, float* out, int64_t out_row_stride,
                                              int64_t out_rel_stride, int64_t long_row, const int64_t* long_rows, int64_t n_long_rows,
                                              void* stream) {
    const char* what = "aggregate_relations";
    if (reduce_op != PGLAMD_SUM && reduce_op != PGLAMD_MEAN) return fail(PGLAMD_E_ARG, "%s: reduce_op %d is neither sum nor mean", what, (int)reduce_op);
    if (num_relations < 1) return fail(PGLAMD_E_SHAPE, "%s: num_relations %d < 1", what, (int)num_relations);
    if (out_rows < 0 || x_rows < 0 || d < 1 || n_long_rows < 0 || long_row < 1)
        return fail(PGLAMD_E_ARG, "%s: bad argument (out_rows %lld, x_rows %lld, d %lld, long_row %lld)", what, (long long)out_rows,
                    (long long)x_rows, (long long)d, (long long)long_row);
    if (d > INT32_MAX / 2 || x_rows > INT32_MAX || out_rows > ((int64_t)1 << 40)) return fail(PGLAMD_E_RANGE, "%s: d / x_rows / out_rows out of range", what);
    if (x_row_stride < d || out_row_stride < d || x_rel_stride < 0 || out_rel_stride < 0 || indptr_rel_stride < 0 || col_scale_rel_stride < 0)
        return fail(PGLAMD_E_SHAPE, "%s: a row stride below d or a negative relation stride", what);
    if (out_rows == 0) return PGLAMD_OK;
    if (!indptr || !out || !col || (x_rows > 0 && !x) || (n_long_rows > 0 && !long_rows)) return fail(PGLAMD_E_ARG, "%s: NULL pointer", what);

    const bool vec = d % 4 == 0 && rel::aligned16(x) && rel::aligned16(out) && x_row_stride % 4 == 0 && x_rel_stride % 4 == 0 &&
                     out_row_stride % 4 == 0 && out_rel_stride % 4 == 0;
    rel::Params p;
    p.x = x; p.x_rows = x_rows; p.ldx = x_row_stride; p.x_rel = x_rel_stride;
    p.indptr = indptr; p.ip_rel = indptr_rel_stride; p.col = col;
    p.cs = col_scale; p.cs_rel = col_scale_rel_stride;
    p.R = num_relations; p.mean = reduce_op == PGLAMD_MEAN;
    p.M = out_rows; p.d = (int32_t)d; p.units = (int32_t)(vec ? d / 4 : d);
    p.out = out; p.ldo = out_row_stride; p.o_rel = out_rel_stride;
    p.long_row = n_long_rows > 0 ? long_row : INT64_MAX;
    p.long_rows = long_rows; p.n_long = n_long_rows;
    p.g_shift = 0;
    while ((1 << p.g_shift) < p.units && p.g_shift < 6) ++p.g_shift;
    p.G = 1 << p.g_shift;
    const int64_t rows_per_block = kBlock >> p.g_shift;
    const int64_t grid = ceil_div(out_rows, rows_per_block);
    if (grid > INT32_MAX || n_long_rows > INT32_MAX) return fail(PGLAMD_E_RANGE, "%s: grid out of range", what);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL(rel::rel_rows_kernel<4>, dim3((unsigned)grid), dim3(kBlock), 0, st, p);
    else hipLaunchKernelGGL(rel::rel_rows_kernel<1>, dim3((unsigned)grid), dim3(kBlock), 0, st, p);
    PGLAMD_LAUNCH_CHECK();
    if (n_long_rows > 0) {
        if (vec) hipLaunchKernelGGL(rel::rel_long_kernel<4>, dim3((unsigned)n_long_rows), dim3(kBlock), 0, st, p);
        else hipLaunchKernelGGL(rel::rel_long_kernel<1>, dim3((unsigned)n_long_rows), dim3(kBlock), 0, st, p);
        PGLAMD_LAUNCH_CHECK();
    }
    return PGLAMD_OK;
}
