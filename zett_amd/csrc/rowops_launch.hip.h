// rowops_launch.hip.h — the launch rule of every row kernel of the forward (rowops.hip.h): which kernel, how many lanes per row, what
// grid, which flags.  One function per kernel family, called by the forward (zett_hip.hip) and by the direct entry points
// (rowops_entry.hip), so that a test of one launch runs the launch the forward runs.  Each function takes the stream, the width H and
// the handle's ln_rows8 / attention_fast / attention_pack options as plain arguments, enqueues exactly one kernel and returns an
// identifier of what it launched; the caller asks hipGetLastError.  Nothing here allocates or validates.
#pragma once

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "rowops.hip.h"

namespace zett {

// One LayerNorm launch of the instantiation (EMBED, READOUT, BT) over `rows` rows of H columns -> zett_ln_kernel.
// (r6) 16-bit modes, narrow rows: layernorm_rows8_kernel, eight columns per lane, 32 lanes per row up to H = 1024 (two rows per
// wave), 64 up to 2048.  Otherwise layernorm_rows_kernel: H <= 2048 a wave per row, four rows per workgroup; wider, a workgroup per row.
template <typename T, bool EMBED, bool READOUT, typename BT>
inline int launch_layernorm(hipStream_t st, int H, int ln_rows8, const float* in, int ld_in, int rows, const float* gamma, const float* beta, float eps,
                            float* of, T* ol, float* stats, float* sum, const LnEmbed& embed, int t0, const LnReadout& readout) {
    auto go = [&](auto kernel, dim3 grid) {
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, in, ld_in, rows, H, gamma, beta, eps, of, ol, stats, sum, embed, t0, readout);
    };
    if constexpr (sizeof(T) == 2) {
        if (const int tpr8 = ln_rows8 ? ln_rows8_tpr(H) : 0) {
            const dim3 grid8((rows + 256 / tpr8 - 1) / (256 / tpr8));
            if (tpr8 == 32) { go(layernorm_rows8_kernel<T, EMBED, 32, READOUT, BT>, grid8); return ZETT_LN_ROWS8_32; }
            go(layernorm_rows8_kernel<T, EMBED, 64, READOUT, BT>, grid8);
            return ZETT_LN_ROWS8_64;
        }
    }
    if (H <= 2048) { go(layernorm_rows_kernel<T, EMBED, 64, READOUT, BT>, dim3((rows + 3) / 4)); return ZETT_LN_WAVE; }
    go(layernorm_rows_kernel<T, EMBED, 256, READOUT, BT>, dim3(rows));
    return ZETT_LN_WORKGROUP;
}

// attention_rows_kernel over `rows` vocabulary rows -> the flags word it ran with (bit 0 cls_only, bit 1 fast path, bit 2 pack,
// bit 3 single rows copy their value row: with cls_slot, the forward's lever 5)
template <typename T>
inline int launch_attention(hipStream_t st, int H, int attention_fast, int attention_pack, const T* q, size_t ldq, const T* k, const T* v, size_t ldkv,
                            int head_dim, const int32_t* row_offset, const uint8_t* row_uniform, const uint8_t* tok_key, int64_t row0, int rows, int tok0,
                            float scaling, int cls_only, const int32_t* tok_pair, T* ctx, const int32_t* cls_slot = nullptr, int skip_single = 0) {
    const int64_t waves = attention_waves(rows, H, attention_pack != 0).total;
    const int flags = (cls_only ? 1 : 0) | (attention_fast ? 2 : 0) | (attention_pack ? 4 : 0) | (skip_single ? 8 : 0);
    hipLaunchKernelGGL((attention_rows_kernel<T>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, q, ldq, k, v, ldkv, H, head_dim, row_offset,
                       row_uniform, tok_key, row0, rows, tok0, scaling, flags, tok_pair, ctx, cls_slot);
    return flags;
}

// LayerNorm fold: (mean, rstd) per row from the H / 128 partials per row the producer GEMM wrote -> the number of partials
inline int launch_ln_stats(hipStream_t st, int H, const float2* parts, int ld_part, int rows, float eps, float* stats) {
    hipLaunchKernelGGL(ln_stats_kernel, dim3((rows + 63) / 64), dim3(64), 0, st, parts, H / 128, ld_part, rows, H, eps, stats);
    return H / 128;
}

// A2 + A3 for table slots [slot0, slot0 + n_slots) -> SRC_DTYPE
template <typename T, int SRC_DTYPE>
inline int launch_gather_src(hipStream_t st, const int32_t* id_list, int slot0, int n_slots, const void* src, int e_in, int v0, const float* fallback,
                             const float* sc_w, const float* sc_b, T* out, int32_t* range_flag) {
    hipLaunchKernelGGL((gather_src_kernel<T, SRC_DTYPE>), dim3(n_slots), dim3(256), 0, st, id_list, slot0, n_slots, src, e_in, v0, fallback, sc_w, sc_b, out,
                       range_flag);
    return SRC_DTYPE;
}

// The gamma-folded copy of a weight [N, K] with its column sums and folded bias -> the grid (one workgroup per output row)
template <typename T>
inline int launch_fold_weight(hipStream_t st, const float* w, int N, int K, const float* gamma, const float* beta, const float* bias, T* w_fold, float* c_out,
                              float* b_out, int32_t* range_flag) {
    hipLaunchKernelGGL(fold_weight_kernel<T>, dim3((unsigned)N), dim3(256), 0, st, w, K, gamma, beta, bias, w_fold, c_out, b_out, range_flag);
    return N;
}

// Lever 6, one-off: C [n_pos, N], cW [N], bq [N] of a weight [N, K] (pos_qkv_kernel; K floats of LDS) -> the grid
inline int launch_pos_qkv(hipStream_t st, const float* w, int N, int K, const float* gamma, const float* beta, const float* bias, const float* type0,
                          const float* pos_emb, int n_pos, float* c_pos, float* c_w, float* b_q) {
    hipLaunchKernelGGL(pos_qkv_kernel, dim3((unsigned)N), dim3(256), (size_t)K * sizeof(float), st, w, K, gamma, beta, bias, type0, pos_emb, n_pos, N, c_pos, c_w,
                       b_q);
    return N;
}

// Lever 6 on a caller's table: its rows of the call's n distinct ids into the handle's own table (table_gather_kernel) -> n
template <typename T>
inline int launch_table_gather(hipStream_t st, const T* table, const float* stats, const int32_t* id_slot, const int32_t* id_list, int n, int H, T* out,
                               float* out_stats) {
    hipLaunchKernelGGL(table_gather_kernel<T>, dim3((unsigned)n), dim3(256), 0, st, table, stats, id_slot, id_list, n, H, out, out_stats);
    return n;
}

// Lever 6: n rows of [q | k | v] (N = 3H columns) from U (pair_qkv_kernel).  Column blocks of PQ_COLS in x; in y as many row walkers as
// give the chip about 2 048 workgroups (each reads its C rows once: the first min(n_pos, PQ_LDS_POS) positions in LDS) -> the y extent
template <typename T>
inline int launch_pair_qkv(hipStream_t st, const T* U, const PairQkvRows& rw, int n, const float* stats, const float* c_pos, int n_pos, const float* c_w,
                           const float* b_q, int N, T* out, size_t ld_out, int32_t* range_flag) {
    const int bx = (N + PQ_COLS - 1) / PQ_COLS;
    const int by = grid_for((n + PQ_UNROLL - 1) / PQ_UNROLL, std::max(1, 2048 / bx));
    const int n_lds = std::min(n_pos, PQ_LDS_POS);
    hipLaunchKernelGGL(pair_qkv_kernel<T>, dim3(bx, by), dim3(256), (size_t)n_lds * 2 * 256 * sizeof(float4), st, U, rw, n, stats, c_pos, n_lds, c_w, b_q, N, out,
                       ld_out, range_flag);
    return by;
}

}  // namespace zett
