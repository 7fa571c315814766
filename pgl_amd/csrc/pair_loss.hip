// pair_loss.hip -- the loss at the end of the embedding pipelines (DeepWalk / metapath2vec: examples/deepwalk/model.py:101-127; LightGCN:
// examples/lightgcn/model.py:158-170), forward AND the source-side gradient in one walk, without a [P, d] or [P, K, d] tensor.  With
// emb [Nu, d], ctx [Nv, d], src [P], tgt [P, T] (T = 1 + K: the positive, then K negatives) and z[p,j] = <emb[src[p]], ctx[tgt[p,j]]>:
//     PGLAMD_PAIR_SKIPGRAM   loss = sum_p ( w_pos softplus(-z[p,0]) + w_neg sum_{j>=1} softplus(z[p,j]) )
//     PGLAMD_PAIR_BPR        loss = w_neg sum_p sum_{j>=1} softplus(z[p,j] - z[p,0])
//     g[p,j]   = d loss / d z[p,j]                                  stored [P, T]: the caller's weights of the context-side gradient
//     d emb[u] = sum_{p: src[p] = u} sum_j g[p,j] ctx[tgt[p,j]]     summed in THIS launch, while ctx's row is in registers
// softplus(x) = max(x, 0) + log1p(exp(-|x|)) and sigma(x) = 1 / (1 + t) | t / (1 + t), t = exp(-|x|): one exponential serves both.
//
// THE WALK (pair_loss_kernel).  The pairs arrive sorted by source: row / eid / indptr of pglamd_csr_build over src (eid = the pair's
// own number).  A LANE GROUP of G = the next power of two >= d / 4 lanes holds a row as one float4 per lane (lanes past d / 4 are
// masked: d = 100 runs on 32 lanes, 25 of them live), so a wave walks 64 / G chunks side by side -- four at d = 64, two at d = 128.
// A group takes one chunk of kPairChunk consecutive sorted pairs (cut by chunk_cut: a source with <= kPairChunk pairs is never split)
// and walks it as a FLAT stream of (pair, j) entries, so the rows in flight do not stop at a pair's end (K = 1: two rows a pair):
//     stage C   lanes 0 .. UB-1 of the group fetch one entry each: position -> (source row, pair number) -> tgt[pair, j], range checked
//     stage B   the ids are handed round the group by lane permutes and UB context rows are issued (UB = min(8, G))
//     stage A   the batch before is consumed: dot product (group_sum), coefficient, accumulate g * row into the source's float4
// emb[src] is loaded once per run of equal sources.  BPR keeps z[p,0] and the positive's float4 and folds it in last, with
// g[p,0] = -sum_j g[p,j].  An id outside its table is not a read: its entry has g = 0 and adds no loss; a pair whose source (the
// caller files it under the extra row Nu) or positive is outside has every g = 0.
// SPLIT ROWS.  A source lying inside a chunk is stored once.  One that straddles chunks leaves head / tail partials in the SplitWs
// layout, which the shared fix-up (launch_fixups, aggregate_flat.hpp) adds in chunk order; sources without a pair are cleared by the
// zero-fill blocks of the same launch.  No memset of a gradient, no floating-point atomic.
// LOSS.  The fp32 terms are added in fp64: every chunk writes one partial and pair_loss_sum_kernel, the last launch, adds them in a
// fixed order.
// GRAD = false (evaluation): no g, no accumulator, no partials, no fix-up; the chunks and the order of the loss are the same, so
// the loss has the same bits.
#include "aggregate_flat.hpp"
#include "attention_common.hpp"

namespace pglamd {

constexpr int kPairChunk = 32;          // sorted pairs per lane group (PAIR_CHUNK of pgl_amd/embedding_ops.py)
constexpr int kPairMaxD = 256;

struct PairParams {
    const float* emb; const float* ctx;
    const int64_t* tgt;                         // [E, T]
    const int* row; const int* eid; const int64_t* indptr;
    float* g;                                   // [E, T]
    float* demb;                                // [out_rows, d]
    double* loss_part;                          // [n_chunks]
    float* part_head; float* part_tail;         // [n_chunks, d]
    int* long_count; int* long_list; int* long_list2;
    int64_t out_rows, n_csr_rows, n_ctx;
    int E, T, n_chunks, chunk, n_grid_chunks, d;
    float w_pos, w_neg;
};

// softplus(x) and its derivative sigma(x) from one exponential
__device__ __forceinline__ void softplus_sigma(float x, float& sp, float& sg) {
    const float t = expf(-fabsf(x));
    const float r = 1.f / (1.f + t);
    sp = fmaxf(x, 0.f) + log1pf(t);
    sg = x >= 0.f ? r : t * r;
}

template <int G> __device__ __forceinline__ int group_lane(int v, int i) {
    if constexpr (G == 1) return v;
    else return __shfl(v, i, G);
}

template <int G, int MODE, bool GRAD>
__global__ __launch_bounds__(kBlock) void pair_loss_kernel(PairParams p) {
    constexpr int GPW = kWave / G;              // chunks a wave walks side by side
    constexpr int UB = G < 8 ? G : 8;           // entries per batch: one fetching lane each
    using V = FV<4>;
    const int lane = threadIdx.x & (kWave - 1);
    const int wib = threadIdx.x >> 6;
    const int gl = lane & (G - 1);
    const int j0 = gl * 4;
    const bool act = j0 < p.d;
    if constexpr (GRAD) {
        if ((int)blockIdx.x >= p.n_grid_chunks) {
            zero_fill_role(p, lane, wave_uniform(wib), [&](int64_t r) {
                if (lane * 4 < p.d) *reinterpret_cast<V*>(p.demb + r * p.d + lane * 4) = V{};
            });
            return;
        }
    }
    const int c = ((int)blockIdx.x * kWavesPerBlock + wib) * GPW + lane / G;
    if (c >= p.n_chunks) return;
    const cptr<int> rowp = as_const(p.row);
    const int e0 = chunk_cut(rowp, as_const(p.indptr), c * p.chunk, p.chunk, p.E);
    const int e1 = chunk_cut(rowp, as_const(p.indptr), c * p.chunk + p.chunk, p.chunk, p.E);
    if (e0 >= e1) {
        if (gl == 0) p.loss_part[c] = 0.0;
        return;
    }
    const float* __restrict__ ctx = p.ctx;
    const int T = p.T;
    const int qend = e1 * T;

    struct Ent { int id, pid, r; };             // one entry as its fetching lane holds it: context row (-1: none), pair, source row
    auto fetch = [&](int qb) {
        Ent en{-1, 0, 0};
        const int q = qb + gl;
        if (gl < UB && q < qend) {
            const int pos = q / T, j = q - pos * T;
            en.r = p.row[pos];
            en.pid = p.eid[pos];
            const int64_t t = p.tgt[(int64_t)en.pid * T + j];
            en.id = (t >= 0 && t < p.n_ctx) ? (int)t : -1;
        }
        return en;
    };
    auto load_rows = [&](const Ent& en, V (&x)[UB]) {
#pragma unroll
        for (int i = 0; i < UB; ++i) {
            const int id = group_lane<G>(en.id, i);
            x[i] = V{};
            if (act && id >= 0) x[i] = *reinterpret_cast<const V*>(ctx + (int64_t)id * p.d + j0);
        }
    };

    int cur = rowp[e0];
    bool head_open = e0 > 0 && rowp[e0 - 1] == cur;
    V ev{}, c0{};
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    float z0 = 0.f, g0 = 0.f;
    double loss = 0.0;                          // (a chunk adds up to 2 * kPairChunk * T terms: in fp64 their order stops mattering)
    int j = 0, pid = 0;
    bool pair_ok = false;

    auto open_row = [&](int r) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = 0.f;
        ev = V{};
        if (act && r < p.out_rows) ev = *reinterpret_cast<const V*>(p.emb + (int64_t)r * p.d + j0);
    };
    auto store_acc = [&](float* dst) {
        V o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o.v[k] = acc[k];
        *reinterpret_cast<V*>(dst + j0) = o;
    };
    auto store_partial = [&](bool headp) {
        if (act) store_acc((headp ? p.part_head : p.part_tail) + (int64_t)c * p.d);
        if (!headp && gl == 0) p.long_list[atomicAdd(p.long_count, 1)] = c;
    };
    auto close_row = [&](bool tail_open) {
        if constexpr (GRAD) {
            if (!p.demb) return;                // g alone (the sparse step sums the rows itself); add_row's accumulation is then wasted work
            if (head_open) store_partial(true);
            else if (tail_open) store_partial(false);
            else if (act && cur < p.out_rows) store_acc(p.demb + (int64_t)cur * p.d);
        }
    };
    auto add_row = [&](float g, const V& cv) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fmaf(g, cv.v[k], acc[k]);
    };
    auto consume = [&](int id, int en_pid, int r, const V& cv) {
        if (j == 0) {                           // a new pair (every branch here is uniform over the group)
            if (r != cur) {
                close_row(false);
                head_open = false;
                cur = r;
                open_row(r);
            }
            pid = en_pid;
            pair_ok = r < p.out_rows && id >= 0;
        }
        float z = ev.v[0] * cv.v[0];
#pragma unroll
        for (int k = 1; k < 4; ++k) z = fmaf(ev.v[k], cv.v[k], z);
        z = group_sum(z, G);
        const bool ok = pair_ok && id >= 0;
        float g = 0.f, sp, sg;
        if constexpr (MODE == PGLAMD_PAIR_SKIPGRAM) {
            const float w = j == 0 ? p.w_pos : p.w_neg;
            softplus_sigma(j == 0 ? -z : z, sp, sg);
            if (ok) { loss += (double)(w * sp); g = j == 0 ? -(w * sg) : w * sg; }
            if constexpr (GRAD) {
                add_row(g, cv);
                if (gl == 0) p.g[(int64_t)pid * T + j] = g;
            }
        } else {
            if (j == 0) { z0 = z; c0 = cv; g0 = 0.f; }
            else {
                softplus_sigma(z - z0, sp, sg);
                if (ok) { loss += (double)(p.w_neg * sp); g = p.w_neg * sg; }
                if constexpr (GRAD) {
                    add_row(g, cv);
                    g0 -= g;
                    if (gl == 0) p.g[(int64_t)pid * T + j] = g;
                }
            }
            if constexpr (GRAD) {
                if (j == T - 1) {               // the positive last: its coefficient is minus the sum of the negatives'
                    add_row(g0, c0);
                    if (gl == 0) p.g[(int64_t)pid * T] = g0;
                }
            }
        }
        if (++j == T) j = 0;
    };

    open_row(cur);
    // three stages deep: rows of batch A consumed, rows of batch B in flight, the entries of batch C being fetched
    int qb = e0 * T;
    Ent enA = fetch(qb), enB = fetch(qb + UB);
    V xA[UB];
    load_rows(enA, xA);
    for (; qb < qend; qb += UB) {
        V xB[UB];
        load_rows(enB, xB);
        const Ent enC = fetch(qb + 2 * UB);
#pragma unroll
        for (int i = 0; i < UB; ++i)
            if (qb + i < qend) consume(group_lane<G>(enA.id, i), group_lane<G>(enA.pid, i), group_lane<G>(enA.r, i), xA[i]);
#pragma unroll
        for (int i = 0; i < UB; ++i) xA[i] = xB[i];
        enA = enB;
        enB = enC;
    }
    close_row(e1 < p.E && rowp[e1] == cur);
    if (gl == 0) p.loss_part[c] = loss;
}

// the chunk partials in a fixed order: thread t adds the partials t, t + 256, ... and the 256 sums meet in a halving tree, in fp64
__global__ __launch_bounds__(kBlock) void pair_loss_sum_kernel(const double* __restrict__ part, int n, float* __restrict__ loss) {
    __shared__ double red[kBlock];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += kBlock) s += part[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)red[0];
}

static int pair_group(int64_t d) {
    int g = 1;
    while (g * 4 < d) g <<= 1;
    return g;
}

template <int MODE, bool GRAD>
static void launch_pair_walk(int G, dim3 grid, hipStream_t st, const PairParams& p) {
#define PGLAMD_PAIR_G(g) case g: hipLaunchKernelGGL((pair_loss_kernel<g, MODE, GRAD>), grid, dim3(kBlock), 0, st, p); break
    switch (G) {
        PGLAMD_PAIR_G(1); PGLAMD_PAIR_G(2); PGLAMD_PAIR_G(4); PGLAMD_PAIR_G(8); PGLAMD_PAIR_G(16); PGLAMD_PAIR_G(32);
        default: hipLaunchKernelGGL((pair_loss_kernel<64, MODE, GRAD>), grid, dim3(kBlock), 0, st, p); break;
    }
#undef PGLAMD_PAIR_G
}

static size_t pair_loss_part_bytes(int64_t n_chunks) { return align_up((size_t)n_chunks * sizeof(double), 256); }

}  // namespace pglamd

using namespace pglamd;

extern "C" size_t pglamd_pair_loss_workspace_bytes(int64_t num_pairs, int64_t d) {
    if (num_pairs <= 0 || d <= 0) return 256;
    const int64_t n_chunks = ceil_div(num_pairs, kPairChunk);
    return SplitWs(n_chunks, d, sizeof(float)).bytes() + pair_loss_part_bytes(n_chunks) + 256;
}

extern "C" int32_t pglamd_pair_loss(const float* emb, int64_t num_emb, const float* ctx, int64_t num_ctx, int64_t d, const int64_t* tgt,
                                    int64_t num_pairs, int64_t num_neg, const int32_t* row, const int32_t* eid, const int64_t* indptr,
                                    int32_t mode, float w_pos, float w_neg, float* loss, float* g, float* grad_emb, void* workspace,
                                    size_t workspace_bytes, void* stream) {
    if (!emb || !ctx || !tgt || !row || !eid || !indptr || !loss || (!g && grad_emb) || num_pairs <= 0 || num_neg < 0 ||
        num_emb <= 0 || num_ctx <= 0 || (mode != PGLAMD_PAIR_SKIPGRAM && mode != PGLAMD_PAIR_BPR) || (mode == PGLAMD_PAIR_BPR && num_neg < 1))
        return fail(PGLAMD_E_ARG, "pair_loss: bad argument");
    if (d <= 0 || d % 4 || d > kPairMaxD) return fail(PGLAMD_E_SHAPE, "pair_loss: d = %lld must be a multiple of 4 up to %d", (long long)d, kPairMaxD);
    const uintptr_t al = reinterpret_cast<uintptr_t>(emb) | reinterpret_cast<uintptr_t>(ctx) | reinterpret_cast<uintptr_t>(grad_emb) |
                         reinterpret_cast<uintptr_t>(workspace);
    if (al % 16) return fail(PGLAMD_E_ARG, "pair_loss: emb, ctx, grad_emb and the workspace must be 16-byte aligned");
    if (num_pairs * (num_neg + 1) > kMaxEdges || num_emb >= INT32_MAX - 1 || num_ctx >= INT32_MAX)
        return fail(PGLAMD_E_RANGE, "pair_loss: sizes beyond int32 engine range");
    if (!workspace || workspace_bytes < pglamd_pair_loss_workspace_bytes(num_pairs, d)) return fail(PGLAMD_E_WORKSPACE, "pair_loss: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool grad = g != nullptr;
    PairParams p{};
    p.emb = emb; p.ctx = ctx; p.tgt = tgt; p.row = row; p.eid = eid; p.indptr = indptr; p.g = g; p.demb = grad_emb;
    p.out_rows = num_emb; p.n_csr_rows = num_emb + 1; p.n_ctx = num_ctx;
    p.E = (int)num_pairs; p.T = (int)num_neg + 1; p.chunk = kPairChunk; p.n_chunks = (int)ceil_div(num_pairs, kPairChunk); p.d = (int)d;
    p.w_pos = w_pos; p.w_neg = w_neg;
    const SplitWs sw(p.n_chunks, d, sizeof(float));
    sw.carve(p, workspace);
    p.loss_part = reinterpret_cast<double*>(static_cast<char*>(workspace) + sw.bytes());
    const int G = pair_group(d);
    p.n_grid_chunks = (int)ceil_div(p.n_chunks, (int64_t)kWavesPerBlock * (kWave / G));
    const int64_t zb = grad_emb ? ceil_div(ceil_div(p.out_rows, kWave), kWavesPerBlock) : 0;
    const bool fixups = grad_emb && p.n_chunks > 1;
    if (fixups) PGLAMD_TRY(reset_split_counters(p, st));
    const dim3 grid((unsigned)(p.n_grid_chunks + zb));
    if (mode == PGLAMD_PAIR_SKIPGRAM) {
        if (grad) launch_pair_walk<PGLAMD_PAIR_SKIPGRAM, true>(G, grid, st, p);
        else launch_pair_walk<PGLAMD_PAIR_SKIPGRAM, false>(G, grid, st, p);
    } else {
        if (grad) launch_pair_walk<PGLAMD_PAIR_BPR, true>(G, grid, st, p);
        else launch_pair_walk<PGLAMD_PAIR_BPR, false>(G, grid, st, p);
    }
    PGLAMD_LAUNCH_CHECK();
    if (fixups) {
        // the shared fix-up reads the split-row workspace through the aggregation's parameter block: partial rows of d floats, a lane
        // per float4, the finished row stored to grad_emb (the rows >= num_emb -- the extra row of pairs without a source -- are skipped)
        AggParams a{};
        a.row = row; a.indptr = indptr; a.out = grad_emb; a.ldo = d; a.tile_cols = (int)d; a.out_rows = num_emb; a.n_csr_rows = num_emb + 1;
        a.E = p.E; a.n_chunks = p.n_chunks; a.chunk = p.chunk; a.x_split = INT32_MAX;
        a.part_head = p.part_head; a.part_tail = p.part_tail; a.long_count = p.long_count; a.long_list = p.long_list; a.long_list2 = p.long_list2;
        PGLAMD_TRY((launch_fixups<float, 4, 1, 0>(a, st)));
    }
    hipLaunchKernelGGL(pair_loss_sum_kernel, dim3(1), dim3(kBlock), 0, st, p.loss_part, p.n_chunks, loss);
    PGLAMD_LAUNCH_CHECK();
    return PGLAMD_OK;
}
