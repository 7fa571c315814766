// gat_fused_16.hip -- the fused GAT attention (gat_fused.hpp) on 16-bit rows: feature, out, out_pos, grad_out and grad_feature stored
// as fp16 or bf16, everything that accumulates in fp32.  A translation unit of its own, as aggregate_half.hip / aggregate_bf16.hip are.
#include "gat_fused.hpp"

using namespace pglamd;

extern "C" int32_t pglamd_gat_aggregate_16(int32_t dtype, const void* feature, const float* attn_src, const float* attn_dst,
                                           int64_t heads, int64_t head_dim, float negative_slope, float drop_p, uint32_t seed,
                                           const int32_t* row, const int32_t* col, const int32_t* eid, const int64_t* indptr,
                                           int64_t num_edges, int64_t n_csr_rows, int64_t out_rows, void* out, float* row_max,
                                           float* row_sum, void* out_pos, float* sum_pos, void* workspace, size_t workspace_bytes,
                                           void* stream) {
    auto run = [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        return gat_aggregate_entry<T>(static_cast<const T*>(feature), attn_src, attn_dst, heads, head_dim, negative_slope, drop_p, seed,
                                      row, col, eid, indptr, num_edges, n_csr_rows, out_rows, static_cast<T*>(out), row_max, row_sum,
                                      static_cast<T*>(out_pos), sum_pos, workspace, workspace_bytes, stream);
    };
    if (dtype == PGLAMD_F16) return run(static_cast<__half*>(nullptr));
    if (dtype == PGLAMD_BF16) return run(static_cast<__hip_bfloat16*>(nullptr));
    return fail(PGLAMD_E_ARG, "gat_aggregate_16: dtype %d is neither PGLAMD_F16 nor PGLAMD_BF16", (int)dtype);
}

extern "C" int32_t pglamd_gat_backward_16(int32_t dtype, const void* grad_out, const void* feature, const float* attn_src,
                                          const float* attn_dst, const float* row_max, const float* row_sum, const void* out,
                                          int64_t heads, int64_t head_dim, float negative_slope, float drop_p, uint32_t seed,
                                          const int32_t* dst_row, const int32_t* dst_col, const int32_t* dst_eid,
                                          const int64_t* dst_indptr, const int32_t* src_row, const int32_t* src_col,
                                          const int32_t* src_eid, const int64_t* src_indptr, int64_t num_edges, int64_t num_nodes,
                                          void* grad_feature, float* grad_attn_src, float* grad_attn_dst, float* grad_pre,
                                          const void* out_pos, const float* sum_pos, void* workspace, size_t workspace_bytes,
                                          void* stream) {
    auto run = [&](auto* tag) {
        using T = std::remove_pointer_t<decltype(tag)>;
        return gat_backward_entry<T>(static_cast<const T*>(grad_out), static_cast<const T*>(feature), attn_src, attn_dst, row_max, row_sum,
                                     static_cast<const T*>(out), heads, head_dim, negative_slope, drop_p, seed, dst_row, dst_col, dst_eid,
                                     dst_indptr, src_row, src_col, src_eid, src_indptr, num_edges, num_nodes,
                                     static_cast<T*>(grad_feature), grad_attn_src, grad_attn_dst, grad_pre,
                                     static_cast<const T*>(out_pos), sum_pos, workspace, workspace_bytes, stream);
    };
    if (dtype == PGLAMD_F16) return run(static_cast<__half*>(nullptr));
    if (dtype == PGLAMD_BF16) return run(static_cast<__hip_bfloat16*>(nullptr));
    return fail(PGLAMD_E_ARG, "gat_backward_16: dtype %d is neither PGLAMD_F16 nor PGLAMD_BF16", (int)dtype);
}
