// rowops_entry.hip — C ABI of the forward's row kernels on their own (include/zett_hip.h, "the forward's row kernels, one launch at a
// time"): what tests/test_rowops_direct_gpu.py calls to check one launch of rowops.hip.h element by element.  Every entry point
// validates all of its arguments, allocates nothing and then goes through the launcher of rowops_launch.hip.h that the forward
// itself calls, so the kernel, lanes per row, grid and flags are the forward's for the same (H, options).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "gemm.hip.h"
#include "rowops.hip.h"
#include "rowops_launch.hip.h"

using namespace zett;

namespace {

bool is_prec(int32_t p) { return p == ZETT_PREC_F32 || p == ZETT_PREC_BF16 || p == ZETT_PREC_F16; }
bool is_pow2(int32_t v) { return v > 0 && (v & (v - 1)) == 0; }

// what every LayerNorm entry point refuses: -> 0 or ZETT_E_INVALID with the text set
int ln_common(const char* who, int32_t prec, int32_t h, const float* gamma, const float* beta, const void* a, const void* b, const void* c, const void* d) {
    if (!is_prec(prec)) return fail(ZETT_E_INVALID, "%s: unknown precision %d", who, prec);
    if (h < 8 || h % 8) return fail(ZETT_E_INVALID, "%s: the width must be a positive multiple of 8, got %d", who, h);
    if (!gamma || !beta) return fail(ZETT_E_INVALID, "%s: gamma and beta are required (null argument)", who);
    if (!aligned(gamma, 16) || !aligned(beta, 16) || !aligned(a, 16) || !aligned(b, 16) || !aligned(c, 16) || !aligned(d, 16))
        return fail(ZETT_E_INVALID, "%s needs 16-byte aligned base pointers", who);
    return 0;
}

}  // namespace

extern "C" {

int zett_op_fwd_layernorm(int32_t prec, const float* in, const void* in_lo, int32_t ld_in, int32_t rows, int32_t h, const float* gamma, const float* beta,
                          float eps, int32_t ln_rows8, float* out_f32, void* out_lo, float* stats, const float* bias_w, const float* bias_b, void* out_bias,
                          const int64_t* bias_rows, int32_t bias_dtype, int32_t* range_flag, int32_t* kernel_id, void* stream) {
    if (int rc = ln_common("zett_op_fwd_layernorm", prec, h, gamma, beta, in, in_lo, out_f32, out_lo)) return rc;
    if (!in && !in_lo) return fail(ZETT_E_INVALID, "zett_op_fwd_layernorm: no input rows (null argument)");
    if (in_lo && prec == ZETT_PREC_F32) return fail(ZETT_E_INVALID, "zett_op_fwd_layernorm: in_lo is a 16-bit feature, not available with ZETT_PREC_F32");
    if (in_lo && !out_bias) return fail(ZETT_E_INVALID, "zett_op_fwd_layernorm: in_lo is read by the readout instantiations only (out_bias is null)");
    if (ld_in < h || ld_in % 8) return fail(ZETT_E_INVALID, "zett_op_fwd_layernorm: ld_in must be a multiple of 8 and at least the width, got %d for %d", ld_in, h);
    if (bias_dtype != -1 && !is_dtype(bias_dtype)) return fail(ZETT_E_INVALID, "zett_op_fwd_layernorm: unknown bias dtype %d", bias_dtype);
    if (!out_bias && (bias_w || bias_rows || bias_dtype != -1)) return fail(ZETT_E_INVALID, "zett_op_fwd_layernorm: a bias head without out_bias (null argument)");
    if (bias_w && !bias_b) return fail(ZETT_E_INVALID, "zett_op_fwd_layernorm: bias_w without bias_b (null argument)");
    if (bias_rows && bias_dtype == -1) return fail(ZETT_E_INVALID, "zett_op_fwd_layernorm: bias_rows needs a destination dtype (bias_dtype -1 is the fp32 store without a map)");
    if (!aligned(bias_w, 16) || !aligned(out_bias, 4) || !aligned(stats, 8)) return fail(ZETT_E_INVALID, "zett_op_fwd_layernorm needs 16-byte aligned base pointers (bias_w), 8-byte aligned stats");
    if (rows < 0) return fail(ZETT_E_INVALID, "zett_op_fwd_layernorm: negative row count");
    if (kernel_id) *kernel_id = -1;
    if (rows == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    LnReadout ro{};
    ro.bias_w = bias_w; ro.bias_b = bias_b; ro.out_bias = (float*)out_bias; ro.in_lo = in_lo; ro.bias_rows = bias_rows; ro.range_flag = range_flag;
    const int id = with_precision(prec, [&](auto a) -> int {
        using T = typename decltype(a)::type;
        if (!out_bias) return launch_layernorm<T, false, false, void>(st, h, ln_rows8, in, ld_in, rows, gamma, beta, eps, out_f32, (T*)out_lo, stats, nullptr, LnEmbed{}, 0, ro);
        if (bias_dtype < 0) return launch_layernorm<T, false, true, void>(st, h, ln_rows8, in, ld_in, rows, gamma, beta, eps, out_f32, (T*)out_lo, stats, nullptr, LnEmbed{}, 0, ro);
        int k = -1;
        with_dtype(bias_dtype, [&](auto dt) {
            k = launch_layernorm<T, false, true, elem_t<decltype(dt)::value>>(st, h, ln_rows8, in, ld_in, rows, gamma, beta, eps, out_f32, (T*)out_lo, stats, nullptr,
                                                                              LnEmbed{}, 0, ro);
        });
        return k;
    });
    HIP_TRY(hipGetLastError());
    if (kernel_id) *kernel_id = id;
    return 0;
}

int zett_op_fwd_embed_layernorm(int32_t prec, const float* table, const void* table_lo, const float* table_stats, const float* table_gamma, const float* table_beta,
                                const int32_t* tok_slot, const int32_t* tok_pos, const float* type0, const float* pos_emb, const float* lang, int32_t lang_pos,
                                const int32_t* tok_row, const int32_t* row_offset, int64_t row0, int32_t rows, int32_t tok0, int32_t m, int32_t h, const float* gamma,
                                const float* beta, float eps, int32_t ln_rows8, void* out_lo, float* stats, float* sum, int32_t* kernel_id, void* stream) {
    if (int rc = ln_common("zett_op_fwd_embed_layernorm", prec, h, gamma, beta, table, table_lo, out_lo, sum)) return rc;
    if (!table && !table_lo) return fail(ZETT_E_INVALID, "zett_op_fwd_embed_layernorm: no table (null argument)");
    if (table_lo && prec == ZETT_PREC_F32) return fail(ZETT_E_INVALID, "zett_op_fwd_embed_layernorm: table_lo is a 16-bit feature, not available with ZETT_PREC_F32");
    if (table_lo && (!table_stats || !table_gamma || !table_beta))
        return fail(ZETT_E_INVALID, "zett_op_fwd_embed_layernorm: table_lo needs table_stats, table_gamma and table_beta (null argument)");
    if (!tok_slot || !tok_pos || !type0 || !pos_emb) return fail(ZETT_E_INVALID, "zett_op_fwd_embed_layernorm: tok_slot, tok_pos, type0 and pos_emb are required (null argument)");
    if (tok_row && !row_offset) return fail(ZETT_E_INVALID, "zett_op_fwd_embed_layernorm: tok_row without row_offset (null argument)");
    if (!aligned(type0, 16) || !aligned(pos_emb, 16) || !aligned(lang, 16) || !aligned(table_gamma, 16) || !aligned(table_beta, 16) || !aligned(table_stats, 8) ||
        !aligned(stats, 8))
        return fail(ZETT_E_INVALID, "zett_op_fwd_embed_layernorm needs 16-byte aligned base pointers, 8-byte aligned statistics");
    if (m < 0 || rows < 0 || tok0 < 0 || row0 < 0 || lang_pos < 0 || (tok_row && rows > m))
        return fail(ZETT_E_INVALID, "zett_op_fwd_embed_layernorm: negative count or offset, or more vocabulary rows than positions");
    if (kernel_id) *kernel_id = -1;
    if (m == 0) return 0;
    LnEmbed e{};
    e.table = table; e.tok_slot = tok_slot; e.tok_pos = tok_pos; e.type0 = type0; e.pos_emb = pos_emb; e.lang = lang; e.lang_pos = lang_pos;
    e.tok_row = tok_row; e.row_offset = row_offset; e.row0 = row0; e.rows = rows;
    e.table_lo = table_lo; e.table_stats = table_stats; e.table_gamma = table_gamma; e.table_beta = table_beta;
    const int id = with_precision(prec, [&](auto a) -> int {
        using T = typename decltype(a)::type;
        return launch_layernorm<T, true, false, void>((hipStream_t)stream, h, ln_rows8, nullptr, h, m, gamma, beta, eps, nullptr, (T*)out_lo, stats, sum, e, tok0, LnReadout{});
    });
    HIP_TRY(hipGetLastError());
    if (kernel_id) *kernel_id = id;
    return 0;
}

int zett_op_fwd_attention(int32_t prec, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, int32_t h, int32_t head_dim,
                          const int32_t* row_offset, const uint8_t* row_uniform, const uint8_t* tok_key, int64_t row0, int32_t rows, int32_t tok0, float scaling,
                          int32_t flags, const int32_t* tok_pair, void* ctx, void* stream) {
    if (!is_prec(prec)) return fail(ZETT_E_INVALID, "zett_op_fwd_attention: unknown precision %d", prec);
    if (!q || !k || !v || !ctx || !row_offset || !row_uniform || !tok_key) return fail(ZETT_E_INVALID, "zett_op_fwd_attention: null argument");
    if (h < 8 || h % 8) return fail(ZETT_E_INVALID, "zett_op_fwd_attention: the width must be a positive multiple of 8, got %d", h);
    if (!is_pow2(head_dim) || head_dim < 8 || head_dim > 512 || h % head_dim)
        return fail(ZETT_E_INVALID, "zett_op_fwd_attention: head_dim must be a power of two in [8, 512] that divides the width, got %d for %d", head_dim, h);
    if (!aligned(q, 16) || !aligned(k, 16) || !aligned(v, 16) || !aligned(ctx, 16)) return fail(ZETT_E_INVALID, "zett_op_fwd_attention needs 16-byte aligned base pointers");
    if (ldq < h || ldq % 8 || ldkv < h || ldkv % 8)
        return fail(ZETT_E_INVALID, "zett_op_fwd_attention: ldq and ldkv must be multiples of 8 and at least the width, got %lld and %lld for %d", (long long)ldq,
                    (long long)ldkv, h);
    if (flags < 0 || flags > 7) return fail(ZETT_E_INVALID, "zett_op_fwd_attention: flags has bits 0..2, got %d", flags);
    if (rows < 0 || row0 < 0 || tok0 < 0) return fail(ZETT_E_INVALID, "zett_op_fwd_attention: negative count or offset");
    if (rows == 0) return 0;
    with_precision(prec, [&](auto a) -> int {
        using T = typename decltype(a)::type;
        return launch_attention<T>((hipStream_t)stream, h, flags & 2, flags & 4, (const T*)q, (size_t)ldq, (const T*)k, (const T*)v, (size_t)ldkv, head_dim, row_offset,
                                   row_uniform, tok_key, row0, rows, tok0, scaling, flags & 1, tok_pair, (T*)ctx);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_fwd_gather_src(int32_t prec, const int32_t* id_list, int32_t slot0, int32_t n_slots, const void* src, int32_t src_dtype, int32_t e_in, int32_t v0,
                           const float* fallback, const float* sc_w, const float* sc_b, void* out, int32_t* range_flag, void* stream) {
    if (!is_prec(prec)) return fail(ZETT_E_INVALID, "zett_op_fwd_gather_src: unknown precision %d", prec);
    if (!is_dtype(src_dtype)) return fail(ZETT_E_INVALID, "zett_op_fwd_gather_src: unknown source dtype %d", src_dtype);
    if (!id_list || !src || !fallback || !out) return fail(ZETT_E_INVALID, "zett_op_fwd_gather_src: null argument");
    if ((sc_w != nullptr) != (sc_b != nullptr)) return fail(ZETT_E_INVALID, "zett_op_fwd_gather_src: the rescaler is sc_w and sc_b together (null argument)");
    if (e_in < 8 || e_in % 8) return fail(ZETT_E_INVALID, "zett_op_fwd_gather_src: the width must be a positive multiple of 8, got %d", e_in);
    if (!aligned(src, 16) || !aligned(fallback, 16) || !aligned(sc_w, 16) || !aligned(sc_b, 16) || !aligned(out, 16))
        return fail(ZETT_E_INVALID, "zett_op_fwd_gather_src needs 16-byte aligned base pointers");
    if (slot0 < 0 || n_slots < 0 || v0 < 0) return fail(ZETT_E_INVALID, "zett_op_fwd_gather_src: negative count or offset");
    if (n_slots == 0) return 0;
    with_precision(prec, [&](auto a) -> int {
        using T = typename decltype(a)::type;
        with_dtype(src_dtype, [&](auto sd) {
            launch_gather_src<T, decltype(sd)::value>((hipStream_t)stream, id_list, slot0, n_slots, src, e_in, v0, fallback, sc_w, sc_b, (T*)out, range_flag);
        });
        return 0;
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_fwd_ln_stats(int32_t prec, const float* parts, int32_t ld_part, int32_t rows, int32_t h, float eps, float* stats, void* stream) {
    if (!is_prec(prec)) return fail(ZETT_E_INVALID, "zett_op_fwd_ln_stats: unknown precision %d", prec);
    if (!parts || !stats) return fail(ZETT_E_INVALID, "zett_op_fwd_ln_stats: null argument");
    if (h < 128 || h % 128) return fail(ZETT_E_INVALID, "zett_op_fwd_ln_stats: one partial per 128 columns: the width must be a positive multiple of 128, got %d", h);
    if (!aligned(parts, 16) || !aligned(stats, 16)) return fail(ZETT_E_INVALID, "zett_op_fwd_ln_stats needs 16-byte aligned base pointers");
    if (rows < 0 || ld_part < rows) return fail(ZETT_E_INVALID, "zett_op_fwd_ln_stats: ld_part must be at least the row count, got %d for %d", ld_part, rows);
    if (rows == 0) return 0;
    launch_ln_stats((hipStream_t)stream, h, (const float2*)parts, ld_part, rows, eps, stats);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_fwd_fold_weight(int32_t prec, const float* w, int32_t n, int32_t k, const float* gamma, const float* beta, const float* bias, void* w_fold,
                            float* c_out, float* b_out, int32_t* range_flag, void* stream) {
    if (!is_prec(prec)) return fail(ZETT_E_INVALID, "zett_op_fwd_fold_weight: unknown precision %d", prec);
    if (prec == ZETT_PREC_F32) return fail(ZETT_E_INVALID, "zett_op_fwd_fold_weight: the LayerNorm fold is a 16-bit feature, not available with ZETT_PREC_F32");
    if (!w || !gamma || !beta || !bias || !w_fold || !c_out || !b_out) return fail(ZETT_E_INVALID, "zett_op_fwd_fold_weight: null argument");
    if (k < 8 || k % 8) return fail(ZETT_E_INVALID, "zett_op_fwd_fold_weight: the width must be a positive multiple of 8, got %d", k);
    if (!aligned(w, 16) || !aligned(w_fold, 16) || !aligned(gamma, 16) || !aligned(beta, 16)) return fail(ZETT_E_INVALID, "zett_op_fwd_fold_weight needs 16-byte aligned base pointers");
    if (n < 0) return fail(ZETT_E_INVALID, "zett_op_fwd_fold_weight: negative row count");
    if (n == 0) return 0;
    with_precision(prec, [&](auto a) -> int {
        using T = typename decltype(a)::type;
        if constexpr (sizeof(T) == 2) launch_fold_weight<T>((hipStream_t)stream, w, n, k, gamma, beta, bias, (T*)w_fold, c_out, b_out, range_flag);
        return 0;
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_fwd_pair_qkv(int32_t prec, const void* u, const int32_t* slot, const int32_t* pos, int32_t t0, int32_t n, const int32_t* tok_row,
                         const int32_t* row_offset, int64_t row0, int32_t rows, const int32_t* cls_slot, const float* stats, const float* c_pos, int32_t n_pos,
                         const float* c_w, const float* b_q, int32_t n_cols, void* out, int64_t ld_out, int32_t* range_flag, void* stream) {
    if (!is_prec(prec)) return fail(ZETT_E_INVALID, "zett_op_fwd_pair_qkv: unknown precision %d", prec);
    if (prec == ZETT_PREC_F32) return fail(ZETT_E_INVALID, "zett_op_fwd_pair_qkv: the id-level Q/K/V is a 16-bit feature, not available with ZETT_PREC_F32");
    if (!u || !slot || !pos || !stats || !c_pos || !c_w || !b_q || !out) return fail(ZETT_E_INVALID, "zett_op_fwd_pair_qkv: null argument");
    if (tok_row && !row_offset) return fail(ZETT_E_INVALID, "zett_op_fwd_pair_qkv: tok_row without row_offset (null argument)");
    if (cls_slot && !tok_row) return fail(ZETT_E_INVALID, "zett_op_fwd_pair_qkv: cls_slot orders buffer rows: it needs tok_row (null argument)");
    if (n_cols < 8 || n_cols % 8) return fail(ZETT_E_INVALID, "zett_op_fwd_pair_qkv: the width must be a positive multiple of 8, got %d", n_cols);
    if (ld_out < n_cols || ld_out % 8) return fail(ZETT_E_INVALID, "zett_op_fwd_pair_qkv: ld_out must be a multiple of 8 and at least the width, got %lld for %d", (long long)ld_out, n_cols);
    if (!aligned(u, 16) || !aligned(out, 16) || !aligned(c_pos, 16) || !aligned(c_w, 16) || !aligned(b_q, 16) || !aligned(stats, 8))
        return fail(ZETT_E_INVALID, "zett_op_fwd_pair_qkv needs 16-byte aligned base pointers, 8-byte aligned statistics");
    if (n < 0 || t0 < 0 || row0 < 0 || rows < 0 || n_pos < 1 || (tok_row && rows > n))
        return fail(ZETT_E_INVALID, "zett_op_fwd_pair_qkv: negative count or offset, no position, or more vocabulary rows than positions");
    if (n == 0) return 0;
    const PairQkvRows rw{slot, pos, t0, tok_row, row_offset, row0, rows, cls_slot};
    with_precision(prec, [&](auto a) -> int {
        using T = typename decltype(a)::type;
        if constexpr (sizeof(T) == 2)
            launch_pair_qkv<T>((hipStream_t)stream, (const T*)u, rw, n, stats, c_pos, n_pos, c_w, b_q, n_cols, (T*)out, (size_t)ld_out, range_flag);
        return 0;
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
