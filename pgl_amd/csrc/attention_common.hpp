// attention_common.hpp -- what the fused attention families share (gat_fused.hip: additive GAT scores; dot_attention.hip: scaled
// dot-product scores): the lane vector, the per-head group sum, the dropout hash, the zero-fill role of a chunked producer, the lane
// geometry rule and the chunked launcher.  The parameter block is a template argument wherever one is read: a family brings its own
// (GatParams, DotParams) with the members named below.
#pragma once
#include "common.hpp"
#include "split_rows.hpp"

#include <type_traits>

namespace pglamd {

template <int VEC> struct alignas(4 * VEC) FV { float v[VEC]; };

// Sum over aligned groups of `group` lanes (a power of two <= 64), result in every lane of the group.  The first four
// steps are DPP lane permutes (VALU latency, no LDS round trip): quad_perm xor-1 / xor-2, then row_half_mirror and
// row_mirror -- once every lane of a quad (resp. 8-lane half row) holds the same partial sum, ANY lane of the
// neighbouring quad (half row) supplies the missing term.  Only groups wider than 16 lanes cross DPP rows (bpermute).
template <int CTRL> __device__ __forceinline__ float dpp_add(float v) {
    return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
__device__ __forceinline__ float group_sum(float v, int group) {
    float t;                                     // selects, not branches: the four DPP steps are always issued
    t = dpp_add<0xB1>(v);  v = group > 1 ? t : v;        // quad_perm [1,0,3,2]
    t = dpp_add<0x4E>(v);  v = group > 2 ? t : v;        // quad_perm [2,3,0,1]
    t = dpp_add<0x141>(v); v = group > 4 ? t : v;        // row_half_mirror
    t = dpp_add<0x140>(v); v = group > 8 ? t : v;        // row_mirror
    if (group > 16) v += __shfl_xor(v, 16);
    if (group > 32) v += __shfl_xor(v, 32);
    return v;
}

// keep-mask of attention dropout: stateless hash of (seed, original edge id, head) -> [0,1)
__device__ __forceinline__ float drop_factor(unsigned seed, int eid, int head, float p, float scale) {
    unsigned h = seed ^ ((unsigned)eid * 0x9E3779B1u) ^ ((unsigned)head * 0x85EBCA77u + 0xC2B2AE3Du);
    h ^= h >> 16; h *= 0x7FEB352Du; h ^= h >> 15; h *= 0x846CA68Bu; h ^= h >> 16;
    return ((h >> 8) * (1.0f / 16777216.0f)) >= p ? scale : 0.f;
}

// Zero-fill role of a chunked producer (its blocks past n_grid_chunks): the rows that receive no edge.  Every wave takes a slice of
// 64 rows, ballots the empty ones and clears them one after the other with all its lanes: clear(r) holds the kernel's own stores.
// P: n_grid_chunks, out_rows, n_csr_rows, indptr.
template <typename P, typename Clear>
__device__ __forceinline__ void zero_fill_role(const P& p, int lane, int wib, Clear clear) {
    const int64_t w = ((int64_t)blockIdx.x - p.n_grid_chunks) * kWavesPerBlock + wib;
    const int64_t r0 = w * kWave;
    if (r0 >= p.out_rows) return;
    const int64_t r = r0 + lane;
    bool empty = false;
    if (r < p.out_rows) empty = (r >= p.n_csr_rows) || (p.indptr[r] == p.indptr[r + 1]);
    unsigned long long mk = __ballot(empty);
    while (mk) {
        const int l = __builtin_ctzll(mk);
        mk &= mk - 1;
        clear(r0 + l);
    }
}

// lane geometry: one 64-lane tile covers all H*D columns, VEC elements of ONE head per lane (elem: bytes of one stored element --
// the operands are aligned to a lane's elem * VEC bytes)
static inline int gat_vec(int64_t heads, int64_t head_dim, const void* a, const void* b, const void* c, bool need_pow2, size_t elem = 4) {
    const int64_t d = heads * head_dim;
    const uintptr_t al = reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c);
    for (int v = 1; v <= 4; v <<= 1) {
        if (d % v || head_dim % v || d / v > kWave || al % (elem * v)) continue;
        const int64_t lph = head_dim / v;
        if (need_pow2 && (lph & (lph - 1))) continue;
        return v;
    }
    return 0;
}

// fn(std::integral_constant<int, VEC>) for the width gat_vec chose: inside fn VEC is a compile-time constant
template <typename Fn>
static int32_t with_vec(int vec, Fn&& fn) {
    switch (vec) {
        case 1: return fn(std::integral_constant<int, 1>{});
        case 2: return fn(std::integral_constant<int, 2>{});
        default: return fn(std::integral_constant<int, 4>{});
    }
}

// A chunked producer and what follows it: the grid (the blocks that walk edge chunks, then the zero-fill blocks), the counters, the
// producer itself -- producer(grid, p) launches it -- and fixups(p), the family's fix-up of the rows it left split.
// P: n_chunks, n_blocks, n_grid_chunks, out_rows and SplitWs's members.
template <typename P, typename Producer, typename Fixups>
static int32_t launch_chunked_rows(P p, hipStream_t st, Producer&& producer, Fixups&& fixups) {
    const int64_t nb = ceil_div(p.n_chunks, kWavesPerBlock);
    p.n_blocks = (int)nb;
    p.n_grid_chunks = (int)xcd_grid(nb);
    const int64_t zb = ceil_div(ceil_div(p.out_rows, kWave), kWavesPerBlock);
    if (p.n_chunks > 1) PGLAMD_TRY(reset_split_counters(p, st));
    producer(dim3((unsigned)(p.n_grid_chunks + zb)), p);
    PGLAMD_LAUNCH_CHECK();
    if (p.n_chunks > 1) PGLAMD_TRY(fixups(p));
    return PGLAMD_OK;
}

}  // namespace pglamd
