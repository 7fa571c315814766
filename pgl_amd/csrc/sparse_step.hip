// sparse_step.hip -- what follows the loss in embedding training: the gradient rows of a batch summed by id and the optimiser applied to
// the touched rows of the table alone (pgl/utils/shared_embedding.py:335-348: row-wise Adagrad and SGD over the batch's rows; the
// DeepWalk / node2vec / metapath2vec examples' Adam(lazy_mode=True); apps/Graph4KG/train.py:58-66: Adagrad, Adam, SGD).  The cost
// follows the number of entries M, never the table height N.
//
//     entries m = 0 .. M-1:  (id[m], col[m], w[m]);  gradient row of m = w[m] * rows[col[m]]
//       explicit form   rows [M, d], col = NULL (the entry's own position), w = NULL (1)
//       gathered form   rows = another table [R, d], col int64 [M] (outside [0, R): the entry adds a zero row), w fp32 [M]
//     the entries arrive SORTED BY ID: row [M] (the sorted ids, an id outside [0, N) filed under N = padding, which nothing is done for)
//     and eid [M] (each sorted position's entry), as pglamd_csr_build(key = id, col = arange) leaves them.  indptr is never read.
//     segment = a run of equal ids:  G = scale * sum_m w[m] rows[col[m]]   (fp32, sorted-position order)
//       PGLAMD_STEP_SGD              w -= lr G
//       PGLAMD_STEP_ADAGRAD          s += G^2;  w -= lr G / (sqrt(s) + eps)                             s [N, d]
//       PGLAMD_STEP_ROWWISE_ADAGRAD  s[id] += mean_k G_k^2;  w -= lr G / (sqrt(s[id]) + 1e-10)         s [N]
//       PGLAMD_STEP_LAZY_ADAM        m = b1 m + (1 - b1) G;  v = b2 v + (1 - b2) G^2;  w -= lr (m / c1) / (sqrt(v / c2) + eps)   m, v [N, d]
//       PGLAMD_STEP_STORE            out_rows[rank] = G, out_ids[rank] = id, rank = the number of segments before this one;
//                                    *out_count = U, the number of segments; out_ids[U ..] = -1
//
// ALIASING RULE.  An applying launch reads `rows` while other lane groups rewrite rows of `weight`: `rows` must not be the table being
// updated (the entry point refuses rows == weight).  The caller then stores the sums first and applies them in explicit form.
//
// THE WALK (sparse_walk_kernel).  The geometry of pair_loss.hip: a LANE GROUP of G = the next power of two >= d / 4 lanes (at most 64)
// holds a row as S float4 slices per lane (S = 1 up to d = 256, then 2 .. 4 on 64 lanes) and takes one chunk of kStepChunk = 32
// consecutive sorted entries, cut on the fixed grid 32 c (no indptr: nothing tells where a row ends but the next id).  Three stages
// deep: lanes 0 .. UB-1 fetch (id, col, w) of batch C while the rows of batch B are in flight and batch A is accumulated.  A new id
// closes the segment: one that lies inside the chunk is finished in registers (apply or store); one that came in from the chunk before
// leaves a HEAD partial H[c], one that goes on past the chunk's end a TAIL partial T[c] and a task, in the SplitWs layout.
// THE FIX-UP (sparse_fixup_kernel), one launch: task a = the row whose first piece is T[a]; its last entry is found by a binary search
// of the sorted ids (b = that entry's chunk).  At most kFixShort further pieces: one wave adds T[a], H[a+1], .., H[b] in that order.
// More: a block of kFixWaves waves, wave w adding its contiguous share of H[a+1 .. b] in order into LDS, wave 0 then T[a] + P_0 + ..
// + P_15 in order.  The same finish as the walk follows.  Which role a row gets depends on the ids alone: two calls give the same bits.
// STORE ranks by count -> scan -> fill: step_heads_kernel counts the segment heads of every chunk (and marks out_ids -1), scan.hpp
// turns them into chunk bases, the walk adds the heads it has met in its chunk; a split row's rank is base[a + 1] - 1.
// No floating-point atomic anywhere.
#include "scan.hpp"
#include "split_rows.hpp"

namespace pglamd {

constexpr int kStepChunk = 32;          // sorted entries per lane group
constexpr int kStepMaxD = 1024;
constexpr int kFixBlock = kFixWaves * kWave;

struct StepParams {
    float* weight; float* s0; float* s1;
    const float* rows; const int64_t* col; const float* w;
    const int* row; const int* eid;
    float* out_rows; int64_t* out_ids; int* out_count;
    int64_t* base;                              // [n_chunks + 1]: segment heads before chunk c (STORE)
    float* part_head; float* part_tail;         // [n_chunks, d]
    int* long_count; int* long_list; int* long_list2;
    int64_t N, R, cap;
    int M, n_chunks, d, kind, fix_short_blocks, fix_long_blocks;
    float scale, lr, eps, b1, b2, ob1, ob2, c1, c2;    // ob = 1 - b, rounded once from the caller's double
};

struct F4 { float v[4]; };
static_assert(sizeof(F4) == 16, "F4 is one 16-byte lane load");
__device__ __forceinline__ F4 ld4(const float* p) { return *reinterpret_cast<const F4*>(p); }
__device__ __forceinline__ void st4(float* p, const F4& x) { *reinterpret_cast<F4*>(p) = x; }

template <int G> __device__ __forceinline__ float lanes_sum(float v) {
#pragma unroll
    for (int o = 1; o < G; o <<= 1) v += __shfl_xor(v, o, G);
    return v;
}
template <int G, typename T> __device__ __forceinline__ T lane_of(T v, int i) {
    if constexpr (G == 1) return v;
    else return __shfl(v, i, G);
}

// The end of a segment whose sum lies in acc (unscaled), columns j0 + s * stride of the lane (those >= d are dead): store or apply.
// G lanes hold the row; `lead` is the one that writes the per-row scalars.
template <int G, int S, bool STORE>
__device__ __forceinline__ void finish_row(const StepParams& p, int id, int64_t rank, F4 (&acc)[S], int j0, int stride, bool lead) {
    const int d = p.d;
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[s].v[k] *= p.scale;
    if constexpr (STORE) {
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (j0 + s * stride < d) st4(p.out_rows + rank * d + j0 + s * stride, acc[s]);
        if (lead) p.out_ids[rank] = id;
    } else {
        float* wr = p.weight + (int64_t)id * d;
        if (p.kind == PGLAMD_STEP_ROWWISE_ADAGRAD) {
            const float s_old = p.s0[id];       // every lane reads before the lead lane writes (one wave, program order)
            float q = 0.f;
#pragma unroll
            for (int s = 0; s < S; ++s)
                if (j0 + s * stride < d)
#pragma unroll
                    for (int k = 0; k < 4; ++k) q = fmaf(acc[s].v[k], acc[s].v[k], q);
            q = lanes_sum<G>(q);
            const float s_new = s_old + q / (float)d;
            const float den = sqrtf(s_new) + 1e-10f;
            if (lead) p.s0[id] = s_new;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const int j = j0 + s * stride;
                if (j >= d) continue;
                F4 x = ld4(wr + j);
#pragma unroll
                for (int k = 0; k < 4; ++k) x.v[k] -= p.lr * acc[s].v[k] / den;
                st4(wr + j, x);
            }
            return;
        }
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int j = j0 + s * stride;
            if (j >= d) continue;
            F4 x = ld4(wr + j);
            if (p.kind == PGLAMD_STEP_SGD) {
#pragma unroll
                for (int k = 0; k < 4; ++k) x.v[k] -= p.lr * acc[s].v[k];
            } else if (p.kind == PGLAMD_STEP_ADAGRAD) {
                float* sr = p.s0 + (int64_t)id * d + j;
                F4 st = ld4(sr);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    st.v[k] = fmaf(acc[s].v[k], acc[s].v[k], st.v[k]);
                    x.v[k] -= p.lr * acc[s].v[k] / (sqrtf(st.v[k]) + p.eps);
                }
                st4(sr, st);
            } else {                            // PGLAMD_STEP_LAZY_ADAM
                float* mr = p.s0 + (int64_t)id * d + j;
                float* vr = p.s1 + (int64_t)id * d + j;
                F4 m = ld4(mr), v = ld4(vr);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float g = acc[s].v[k];
                    m.v[k] = fmaf(p.b1, m.v[k], p.ob1 * g);
                    v.v[k] = fmaf(p.b2, v.v[k], p.ob2 * g * g);
                    x.v[k] -= p.lr * (m.v[k] / p.c1) / (sqrtf(v.v[k] / p.c2) + p.eps);
                }
                st4(mr, m);
                st4(vr, v);
            }
            st4(wr + j, x);
        }
    }
}

// segment heads per chunk (a head: an in-range id that differs from the id before it), and the -1 marks of out_ids
__global__ __launch_bounds__(kBlock) void step_heads_kernel(StepParams p) {
    const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x, stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = t0; i < p.cap; i += stride) p.out_ids[i] = -1;
    for (int64_t t = t0; t <= p.n_chunks; t += stride) {
        int64_t heads = 0;
        if (t < p.n_chunks) {
            const int e0 = (int)t * kStepChunk, e1 = min(e0 + kStepChunk, p.M);
            int prev = e0 > 0 ? p.row[e0 - 1] : -1;
            for (int e = e0; e < e1; ++e) {
                const int r = p.row[e];
                heads += (r != prev && r < p.N) ? 1 : 0;
                prev = r;
            }
        }
        p.base[t] = heads;                      // (entry n_chunks: 0, so that the scan leaves the total there)
    }
}

template <int G, int S, bool STORE>
__global__ __launch_bounds__(kBlock) void sparse_walk_kernel(StepParams p) {
    constexpr int GPW = kWave / G;
    constexpr int UB = G < 8 ? G : (S == 1 ? 8 : (S == 2 ? 4 : 2));    // entries per batch: UB * S float4 per lane in flight, twice
    constexpr int STRIDE = G * 4;
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = threadIdx.x >> 6;
    const int gl = lane & (G - 1);
    const int j0 = gl * 4;
    const int d = p.d;
    if constexpr (STORE) {
        if (blockIdx.x == 0 && threadIdx.x == 0) *p.out_count = (int)p.base[p.n_chunks];
    }
    const int c = ((int)blockIdx.x * kWavesPerBlock + wib) * GPW + lane / G;
    if (c >= p.n_chunks) return;
    const int e0 = c * kStepChunk, e1 = min(e0 + kStepChunk, p.M);
    const float* __restrict__ rows = p.rows;

    struct Ent { int r, c; float w; };          // one entry as its fetching lane holds it: id, source row (-1: none), weight
    auto fetch = [&](int qb) {
        Ent en{0, -1, 0.f};
        const int q = qb + gl;
        if (gl < UB && q < e1) {
            en.r = p.row[q];
            const int pos = p.eid[q];
            const int64_t cc = p.col ? p.col[pos] : (int64_t)pos;
            en.c = (cc >= 0 && cc < p.R && en.r < p.N) ? (int)cc : -1;
            en.w = p.w ? p.w[pos] : 1.f;
        }
        return en;
    };
    auto load_rows = [&](const Ent& en, F4 (&x)[UB][S]) {
#pragma unroll
        for (int i = 0; i < UB; ++i) {
            const int id = lane_of<G>(en.c, i);
#pragma unroll
            for (int s = 0; s < S; ++s) {
                x[i][s] = F4{};
                if (id >= 0 && j0 + s * STRIDE < d) x[i][s] = ld4(rows + (int64_t)id * d + j0 + s * STRIDE);
            }
        }
    };

    int cur = p.row[e0];
    bool head_open = e0 > 0 && p.row[e0 - 1] == cur;
    int64_t rank = 0;
    if constexpr (STORE) rank = p.base[c] - 1 + ((!head_open && cur < p.N) ? 1 : 0);
    F4 acc[S];
#pragma unroll
    for (int s = 0; s < S; ++s) acc[s] = F4{};

    auto store_partial = [&](float* dst) {
#pragma unroll
        for (int s = 0; s < S; ++s)
            if (j0 + s * STRIDE < d) st4(dst + (int64_t)c * d + j0 + s * STRIDE, acc[s]);
    };
    auto close_row = [&](bool tail_open) {
        if (cur >= p.N) return;                 // padding: nothing is read, summed or written for it
        if (head_open) store_partial(p.part_head);
        else if (tail_open) {
            store_partial(p.part_tail);
            if (gl == 0) p.long_list[atomicAdd(p.long_count + kSplitCountList1, 1)] = c;
        } else finish_row<G, S, STORE>(p, cur, rank, acc, j0, STRIDE, gl == 0);
    };
    auto consume = [&](int r, float w, const F4 (&x)[S]) {
        if (r != cur) {                         // (uniform over the group)
            close_row(false);
            head_open = false;
            cur = r;
            if constexpr (STORE) rank += r < p.N ? 1 : 0;
#pragma unroll
            for (int s = 0; s < S; ++s) acc[s] = F4{};
        }
#pragma unroll
        for (int s = 0; s < S; ++s)
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[s].v[k] = fmaf(w, x[s].v[k], acc[s].v[k]);
    };

    // three stages deep: rows of batch A consumed, rows of batch B in flight, the entries of batch C being fetched
    int qb = e0;
    Ent enA = fetch(qb), enB = fetch(qb + UB);
    F4 xA[UB][S];
    load_rows(enA, xA);
    for (; qb < e1; qb += UB) {
        F4 xB[UB][S];
        load_rows(enB, xB);
        const Ent enC = fetch(qb + 2 * UB);
#pragma unroll
        for (int i = 0; i < UB; ++i)
            if (qb + i < e1) consume(lane_of<G>(enA.r, i), lane_of<G>(enA.w, i), xA[i]);
#pragma unroll
        for (int i = 0; i < UB; ++i)
#pragma unroll
            for (int s = 0; s < S; ++s) xA[i][s] = xB[i][s];
        enA = enB;
        enB = enC;
    }
    close_row(e1 < p.M && p.row[e1] == cur);
}

// One launch for the rows that straddle chunks: blocks [0, fix_short_blocks) run the short role (a task per wave), the rest the long
// role (a task per block).  A lane owns the float4 columns 4 lane + 256 s, s < 4.
template <bool STORE>
__global__ __launch_bounds__(kFixBlock) void sparse_fixup_kernel(StepParams p) {
    extern __shared__ float fix_lds[];          // long role: [kFixWaves, d]
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = wave_uniform((int)threadIdx.x >> 6);
    const int d = p.d;
    const int j0 = lane * 4;
    constexpr int STRIDE = kWave * 4;
    const int n_tasks = p.long_count[kSplitCountList1];
    const bool long_role = (int)blockIdx.x >= p.fix_short_blocks;
    const int first = long_role ? (int)blockIdx.x - p.fix_short_blocks : (int)blockIdx.x * kFixWaves + wib;
    const int step = long_role ? p.fix_long_blocks : p.fix_short_blocks * kFixWaves;
    auto add_piece = [&](F4 (&acc)[4], const float* src) {
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (j0 + s * STRIDE < d) {
                const F4 x = ld4(src + j0 + s * STRIDE);
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[s].v[k] += x.v[k];
            }
    };
    for (int t = first; t < n_tasks; t += step) {
        const int a = p.long_list[t];
        const int id = p.row[a * kStepChunk + kStepChunk - 1];     // the chunk's last entry: the row that goes on
        int lo = (a + 1) * kStepChunk, hi = p.M;                    // first position past the row, in (lo, hi]: row[lo] == id
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (p.row[mid] > id) hi = mid; else lo = mid + 1;
        }
        const int b = (lo - 1) / kStepChunk;
        if (fixup_is_long(a, b) != long_role) continue;             // (the same for every thread of a long-role block)
        const int64_t rank = STORE ? p.base[a + 1] - 1 : 0;
        F4 acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[s] = F4{};
        if (!long_role) {
            add_piece(acc, p.part_tail + (int64_t)a * d);
            for (int k = a + 1; k <= b; ++k) add_piece(acc, p.part_head + (int64_t)k * d);
            finish_row<kWave, 4, STORE>(p, id, rank, acc, j0, STRIDE, lane == 0);
            continue;
        }
        const int per = (b - a + kFixWaves - 1) / kFixWaves;
        const int k0 = a + 1 + wib * per, k1 = min(k0 + per, b + 1);
        for (int k = k0; k < k1; ++k) add_piece(acc, p.part_head + (int64_t)k * d);
#pragma unroll
        for (int s = 0; s < 4; ++s)
            if (j0 + s * STRIDE < d) st4(fix_lds + wib * d + j0 + s * STRIDE, acc[s]);
        __syncthreads();
        if (wib == 0) {
#pragma unroll
            for (int s = 0; s < 4; ++s) acc[s] = F4{};
            add_piece(acc, p.part_tail + (int64_t)a * d);
            for (int w = 0; w < kFixWaves; ++w) add_piece(acc, fix_lds + w * d);
            finish_row<kWave, 4, STORE>(p, id, rank, acc, j0, STRIDE, lane == 0);
        }
        __syncthreads();                        // the next task's partials overwrite the LDS rows
    }
}

static void step_geometry(int64_t d, int& G, int& S) {
    G = 1;
    while (G * 4 < d && G < kWave) G <<= 1;
    S = (int)ceil_div(d, (int64_t)G * 4);
}

template <bool STORE>
static void launch_step_walk(int G, int S, dim3 grid, hipStream_t st, const StepParams& p) {
#define PGLAMD_STEP_G(g, s) hipLaunchKernelGGL((sparse_walk_kernel<g, s, STORE>), grid, dim3(kBlock), 0, st, p)
    switch (G) {
        case 1: PGLAMD_STEP_G(1, 1); break;
        case 2: PGLAMD_STEP_G(2, 1); break;
        case 4: PGLAMD_STEP_G(4, 1); break;
        case 8: PGLAMD_STEP_G(8, 1); break;
        case 16: PGLAMD_STEP_G(16, 1); break;
        case 32: PGLAMD_STEP_G(32, 1); break;
        default:
            if (S == 1) PGLAMD_STEP_G(64, 1);
            else if (S == 2) PGLAMD_STEP_G(64, 2);
            else if (S == 3) PGLAMD_STEP_G(64, 3);
            else PGLAMD_STEP_G(64, 4);
            break;
    }
#undef PGLAMD_STEP_G
}

static size_t step_base_bytes(int64_t n_chunks) { return align_up((size_t)(n_chunks + 1) * sizeof(int64_t), 256); }

}  // namespace pglamd

using namespace pglamd;

extern "C" size_t pglamd_sparse_step_workspace_bytes(int64_t num_entries, int64_t d) {
    if (num_entries <= 0 || d <= 0) return 256;
    const int64_t n_chunks = ceil_div(num_entries, kStepChunk);
    return SplitWs(n_chunks, d, sizeof(float)).bytes() + step_base_bytes(n_chunks) + exclusive_scan64_temp_bytes(n_chunks + 1) + 256;
}

extern "C" int32_t pglamd_sparse_step(float* weight, int64_t num_rows, int64_t d, const float* rows, int64_t num_src_rows, const int64_t* col,
                                      const float* w, int64_t num_entries, const int32_t* row, const int32_t* eid, float scale, int32_t kind,
                                      float lr, float eps, double beta1, double beta2, float corr1, float corr2, float* state0, float* state1,
                                      float* out_rows, int64_t* out_ids, int32_t* out_count, void* workspace, size_t workspace_bytes,
                                      void* stream) {
    if (num_entries == 0) return PGLAMD_OK;
    const bool store = kind == PGLAMD_STEP_STORE;
    if (!rows || !row || !eid || num_entries < 0 || num_rows <= 0 || num_src_rows <= 0 || kind < PGLAMD_STEP_SGD || kind > PGLAMD_STEP_STORE ||
        (w && !col))
        return fail(PGLAMD_E_ARG, "sparse_step: bad argument");
    if (store ? (!out_rows || !out_ids || !out_count) : !weight) return fail(PGLAMD_E_ARG, "sparse_step: the output of this kind is missing");
    if ((kind == PGLAMD_STEP_ADAGRAD || kind == PGLAMD_STEP_ROWWISE_ADAGRAD || kind == PGLAMD_STEP_LAZY_ADAM) && !state0)
        return fail(PGLAMD_E_ARG, "sparse_step: the optimiser's state is missing");
    if (kind == PGLAMD_STEP_LAZY_ADAM && (!state1 || !(corr1 > 0.f) || !(corr2 > 0.f)))
        return fail(PGLAMD_E_ARG, "sparse_step: lazy Adam takes two state tables and positive bias corrections");
    if (!store && rows == weight) return fail(PGLAMD_E_ARG, "sparse_step: rows is the table being updated (store the sums, then apply them)");
    if (!col && num_src_rows < num_entries) return fail(PGLAMD_E_ARG, "sparse_step: the explicit form takes one row per entry");
    if (d < 4 || d % 4 || d > kStepMaxD) return fail(PGLAMD_E_SHAPE, "sparse_step: d = %lld must be a multiple of 4 in 4 .. %d", (long long)d, kStepMaxD);
    const uintptr_t al = reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(out_rows) |
                         reinterpret_cast<uintptr_t>(workspace) | (kind == PGLAMD_STEP_ROWWISE_ADAGRAD ? 0 : reinterpret_cast<uintptr_t>(state0)) |
                         reinterpret_cast<uintptr_t>(state1);
    if (al % 16) return fail(PGLAMD_E_ARG, "sparse_step: the tables, rows, out_rows and the workspace must be 16-byte aligned");
    if (num_entries > kMaxEdges || num_rows >= INT32_MAX || num_src_rows >= INT32_MAX) return fail(PGLAMD_E_RANGE, "sparse_step: sizes beyond int32 engine range");
    if (!workspace || workspace_bytes < pglamd_sparse_step_workspace_bytes(num_entries, d)) return fail(PGLAMD_E_WORKSPACE, "sparse_step: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    StepParams p{};
    p.weight = weight; p.s0 = state0; p.s1 = state1; p.rows = rows; p.col = col; p.w = w; p.row = row; p.eid = eid;
    p.out_rows = out_rows; p.out_ids = out_ids; p.out_count = out_count;
    p.N = num_rows; p.R = num_src_rows; p.cap = std::min(num_entries, num_rows);
    p.M = (int)num_entries; p.n_chunks = (int)ceil_div(num_entries, kStepChunk); p.d = (int)d; p.kind = kind;
    p.scale = scale; p.lr = lr; p.eps = eps; p.b1 = (float)beta1; p.b2 = (float)beta2; p.ob1 = (float)(1.0 - beta1); p.ob2 = (float)(1.0 - beta2); p.c1 = corr1; p.c2 = corr2;
    const SplitWs sw(p.n_chunks, d, sizeof(float));
    sw.carve(p, workspace);
    p.base = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + sw.bytes());
    void* scan_temp = static_cast<char*>(workspace) + sw.bytes() + step_base_bytes(p.n_chunks);
    int G, S;
    step_geometry(d, G, S);
    const bool fixups = p.n_chunks > 1;
    if (fixups) {
        PGLAMD_TRY(reset_split_counters(p, st));
        p.fix_short_blocks = (int)fixup_grid_short(p.n_chunks, kFixGridMergedShort, kFixWaves);
        p.fix_long_blocks = p.n_chunks > kFixShort + 1 ? (int)std::min<int64_t>(kFixGridLong, p.n_chunks / (kFixShort + 1)) : 0;
    }
    if (store) {
        const int64_t nb = std::min<int64_t>(std::max(ceil_div(p.n_chunks + 1, kBlock), ceil_div(p.cap, kBlock)), 65536);
        hipLaunchKernelGGL(step_heads_kernel, dim3((unsigned)nb), dim3(kBlock), 0, st, p);
        PGLAMD_LAUNCH_CHECK();
        PGLAMD_TRY(exclusive_scan64(LoadI64{p.base}, (int64_t)p.n_chunks + 1, p.base, scan_temp, st));
    }
    const dim3 grid((unsigned)ceil_div(p.n_chunks, (int64_t)kWavesPerBlock * (kWave / G)));
    if (store) launch_step_walk<true>(G, S, grid, st, p);
    else launch_step_walk<false>(G, S, grid, st, p);
    PGLAMD_LAUNCH_CHECK();
    if (fixups) {
        const dim3 fgrid((unsigned)(p.fix_short_blocks + p.fix_long_blocks));
        const size_t lds = p.fix_long_blocks ? (size_t)kFixWaves * d * sizeof(float) : 0;
        if (store) hipLaunchKernelGGL(sparse_fixup_kernel<true>, fgrid, dim3(kFixBlock), lds, st, p);
        else hipLaunchKernelGGL(sparse_fixup_kernel<false>, fgrid, dim3(kFixBlock), lds, st, p);
        PGLAMD_LAUNCH_CHECK();
    }
    return PGLAMD_OK;
}
