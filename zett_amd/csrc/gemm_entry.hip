// gemm_entry.hip — C ABI of ONE GEMM launch of the forward (include/zett_hip.h, "one GEMM launch of the forward"): what
// tests/test_gemm_fwd_direct_gpu.py calls to check a launch with any epilogue element by element.  The entry point validates all of its
// arguments, allocates nothing and then takes the forward's own path: gemm_variant_for / gemm_row0_for (gemm_launch.hip.h) choose the
// tile and the tail cut exactly as Runner::gemm of zett_hip.hip does, launch_gemm_variant launches it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "gemm.hip.h"
#include "gemm_launch.hip.h"

using namespace zett;

namespace {

const char* const WHO = "zett_op_fwd_gemm";

template <typename T>
int run(const zett_fwd_gemm_desc& d, int32_t* variant_out, int32_t* mode_out, hipStream_t st) {
    constexpr int es = (int)sizeof(T);
    if ((int64_t)d.k * es < 128 || ((int64_t)d.k * es) % 128)
        return fail(ZETT_E_INVALID, "%s: k must be a positive multiple of %d (128 bytes of K), got %d", WHO, 128 / es, d.k);
    if (d.lda < d.k || d.ldw < d.k || ((int64_t)d.lda * es) % 16 || ((int64_t)d.ldw * es) % 16)
        return fail(ZETT_E_INVALID, "%s: lda and ldw must be at least k and multiples of %d (16-byte rows), got %d and %d for k = %d", WHO, 16 / es, d.lda, d.ldw, d.k);
    const bool split = d.split_col > 0 && d.split_col < d.n;
    const int width = split ? d.split_col : d.n;          // columns of out_f32 / out_lo
    if (d.out_f32 && d.ld_f32 < width) return fail(ZETT_E_INVALID, "%s: ld_f32 %d is smaller than the %d columns of out_f32", WHO, d.ld_f32, width);
    if (d.out_f32_b && d.ld_f32 < d.n - d.split_col) return fail(ZETT_E_INVALID, "%s: ld_f32 %d is smaller than the %d columns of out_f32_b", WHO, d.ld_f32, d.n - d.split_col);
    if (d.out_lo && d.ld_lo < width) return fail(ZETT_E_INVALID, "%s: ld_lo %d is smaller than the %d columns of out_lo", WHO, d.ld_lo, width);
    if (d.residual && d.ld_res < d.n) return fail(ZETT_E_INVALID, "%s: ld_res %d is smaller than n = %d", WHO, d.ld_res, d.n);
    if (d.residual_lo && d.ld_res_lo < d.n) return fail(ZETT_E_INVALID, "%s: ld_res_lo %d is smaller than n = %d", WHO, d.ld_res_lo, d.n);
    if (d.stats_part && d.ld_part < d.m) return fail(ZETT_E_INVALID, "%s: ld_part %d is smaller than m = %d", WHO, d.ld_part, d.m);
    if (d.dst && d.ld_dst < d.n) return fail(ZETT_E_INVALID, "%s: ld_dst %lld is smaller than n = %d", WHO, (long long)d.ld_dst, d.n);

    GemmEpilogue<T> e{};
    e.bias = d.bias; e.act = d.act;
    e.residual = d.residual; e.ld_res = d.ld_res;
    e.res_stats = d.res_stats; e.res_gamma = d.res_gamma; e.res_beta = d.res_beta; e.res_index = d.res_index;
    e.stats_part = (float2*)d.stats_part; e.ld_part = d.ld_part;
    e.fold_stats = d.fold_stats; e.fold_c = d.fold_c;
    e.scale = d.scale; e.shift = d.shift;
    e.out_f32 = d.out_f32; e.ld_f32 = d.ld_f32;
    e.out_lo = (T*)d.out_lo; e.ld_lo = d.ld_lo;
    e.split_col = split ? d.split_col : 0x7fffffff;
    e.out_f32_b = d.out_f32_b;
    e.range_flag = d.range_flag; e.range_final = d.range_final;
    e.residual_lo = (const T*)d.residual_lo; e.ld_res_lo = d.ld_res_lo;
    e.dst = d.dst; e.dst_rows = d.dst_rows; e.ld_dst = d.ld_dst; e.dst_dtype = d.dst_dtype;

    GemmOptions o;
    o.gemm_variant = d.gemm_variant; o.gemm4d_min_k = d.gemm4d_min_k; o.gemm_tail_split = d.gemm_tail_split;
    o.gemm_tile_order = d.gemm_tile_order; o.gemm_group = d.gemm_group;
    const GemmArgs<T> g = gemm_args_for(o, (const T*)d.a, d.lda, (const T*)d.w, d.ldw, d.m, d.n, d.k, e);
    const int variant = gemm_variant_for<T>(o, (long)d.a_rows_readable, d.m, d.n, d.k, e);
    int mode = -1;
    if (variant == 7 || variant == 8) {
        mode = gemm_4d_launch_mode(g, variant == 8);
        if (mode < 0)
            return fail(ZETT_E_INVALID, d.dst ? "%s: no gemm4d instantiation stores this launch into dst (the forward stages such rows in fp32): F32_SCALE / F32_SCALE_FOLD "
                                                "epilogues with ld_dst %% 4 == 0 and a base aligned for four values only"
                                              : "%s: no gemm4d instantiation carries this stats_part / fold_stats epilogue (gemm4d_epi_mode)", WHO);
    }
    if (d.dst && variant != 7) return fail(ZETT_E_INVALID, "%s: dst is stored by tile variant 7 only; this launch takes variant %d (the forward stages such rows in fp32)", WHO, variant);
    if (d.m == 0 || d.n == 0) return 0;          // (an empty launch passes every check above and launches nothing)
    if (variant_out) *variant_out = variant;
    if (mode_out) *mode_out = mode;
    HIP_TRY(launch_gemm_variant(variant, g, st));
    return 0;
}

}  // namespace

extern "C" {

int zett_op_fwd_gemm(int32_t prec, const zett_fwd_gemm_desc* desc, int32_t* variant_out, int32_t* mode_out, void* stream) {
    if (!desc) return fail(ZETT_E_INVALID, "%s: null descriptor", WHO);
    if (desc->size != (int64_t)sizeof(zett_fwd_gemm_desc))
        return fail(ZETT_E_INVALID, "%s: descriptor size %lld, this library knows %lld", WHO, (long long)desc->size, (long long)sizeof(zett_fwd_gemm_desc));
    const zett_fwd_gemm_desc& d = *desc;
    if (prec != ZETT_PREC_F32 && prec != ZETT_PREC_BF16 && prec != ZETT_PREC_F16) return fail(ZETT_E_INVALID, "%s: unknown precision %d", WHO, prec);
    if (prec == ZETT_PREC_F32 && (d.stats_part || d.fold_stats || d.fold_c || d.residual_lo || d.dst))
        return fail(ZETT_E_INVALID, "%s: stats_part, fold_stats, residual_lo and dst are 16-bit features, not available with ZETT_PREC_F32", WHO);
    if (d.act != ACT_NONE && d.act != ACT_GELU_TANH && d.act != ACT_GELU_ERF) return fail(ZETT_E_INVALID, "%s: unknown act %d", WHO, d.act);
    if (d.dst && !is_dtype(d.dst_dtype)) return fail(ZETT_E_INVALID, "%s: unknown dst dtype %d", WHO, d.dst_dtype);
    if (d.reserved != 0) return fail(ZETT_E_INVALID, "%s: the reserved field must be 0", WHO);
    if (d.gemm_variant != 0 && d.gemm_variant != 1 && d.gemm_variant != 2 && d.gemm_variant != 3 && d.gemm_variant != 7 && d.gemm_variant != 8)
        return fail(ZETT_E_INVALID, "%s: gemm_variant must be 0 (auto), 1, 2, 3, 7 or 8, got %d", WHO, d.gemm_variant);
    if (d.gemm4d_min_k < 64) return fail(ZETT_E_INVALID, "%s: gemm4d_min_k must be >= 64", WHO);
    if (d.gemm_tail_split < 0 || d.gemm_tail_split > 3) return fail(ZETT_E_INVALID, "%s: gemm_tail_split must be 0 .. 3", WHO);
    if (d.gemm_tile_order < 0 || d.gemm_tile_order > 1) return fail(ZETT_E_INVALID, "%s: gemm_tile_order must be 0 or 1", WHO);
    if (d.gemm_group < 0 || d.gemm_group > 64) return fail(ZETT_E_INVALID, "%s: gemm_group must be 0 .. 64", WHO);
    if (d.m < 0 || d.n < 0) return fail(ZETT_E_INVALID, "%s: negative m or n", WHO);
    if (!d.a || !d.w) return fail(ZETT_E_INVALID, "%s: a and w are required (null argument)", WHO);
    if (!aligned(d.a, 16) || !aligned(d.w, 16) || !aligned(d.bias, 16) || !aligned(d.residual, 16) || !aligned(d.residual_lo, 16) || !aligned(d.res_gamma, 16) ||
        !aligned(d.res_beta, 16) || !aligned(d.fold_c, 16) || !aligned(d.scale, 16) || !aligned(d.shift, 16) || !aligned(d.out_f32, 16) || !aligned(d.out_lo, 16) ||
        !aligned(d.out_f32_b, 16))
        return fail(ZETT_E_INVALID, "%s needs 16-byte aligned base pointers", WHO);
    if (!aligned(d.res_stats, 8) || !aligned(d.fold_stats, 8) || !aligned(d.stats_part, 8) || !aligned(d.dst_rows, 8) || !aligned(d.res_index, 4) || !aligned(d.range_flag, 4) ||
        !aligned(d.dst, d.dst_dtype == ZETT_F32 ? 4 : 2))
        return fail(ZETT_E_INVALID, "%s needs 8-byte aligned statistics, partials and dst_rows, 4-byte aligned res_index and range_flag, dst aligned to its element", WHO);
    if (!d.out_f32 && !d.out_lo && !d.out_f32_b && !d.dst) return fail(ZETT_E_INVALID, "%s: no output at all (out_f32, out_lo, out_f32_b and dst are null)", WHO);
    if (d.dst && (d.out_f32 || d.out_lo || d.out_f32_b)) return fail(ZETT_E_INVALID, "%s: dst replaces out_f32: it cannot be combined with out_f32, out_lo or out_f32_b", WHO);
    if (d.dst_rows && !d.dst) return fail(ZETT_E_INVALID, "%s: dst_rows without dst (null argument)", WHO);
    const bool split = d.split_col > 0 && d.split_col < d.n;
    if (split != (d.out_f32_b != nullptr)) return fail(ZETT_E_INVALID, "%s: out_f32_b and a split_col inside (0, n) come together, got split_col %d for n = %d", WHO, d.split_col, d.n);
    if (d.residual && d.residual_lo) return fail(ZETT_E_INVALID, "%s: residual together with residual_lo", WHO);
    if (d.residual_lo && !d.stats_part) return fail(ZETT_E_INVALID, "%s: residual_lo is read by the LayerNorm producer only (stats_part is null)", WHO);
    if (d.res_stats && (!d.res_gamma || !d.res_beta)) return fail(ZETT_E_INVALID, "%s: res_stats without res_gamma and res_beta (null argument)", WHO);
    if ((d.res_stats || d.res_index) && !d.residual && !d.residual_lo) return fail(ZETT_E_INVALID, "%s: res_stats / res_index without a residual (null argument)", WHO);
    if ((d.scale != nullptr) != (d.shift != nullptr)) return fail(ZETT_E_INVALID, "%s: the Rescaler is scale and shift together (null argument)", WHO);
    if ((d.fold_stats != nullptr) != (d.fold_c != nullptr)) return fail(ZETT_E_INVALID, "%s: the LayerNorm fold is fold_stats and fold_c together (null argument)", WHO);
    if (d.a_rows_readable < d.m) return fail(ZETT_E_INVALID, "%s: a_rows_readable %lld is smaller than m = %d", WHO, (long long)d.a_rows_readable, d.m);
    if (variant_out) *variant_out = -1;
    if (mode_out) *mode_out = -1;
    return with_precision(prec, [&](auto a) -> int {
        using T = typename decltype(a)::type;
        return run<T>(d, variant_out, mode_out, (hipStream_t)stream);
    });
}

}  // extern "C"
