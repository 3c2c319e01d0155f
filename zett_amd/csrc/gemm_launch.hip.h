// gemm_launch.hip.h — the GEMM launchers as the host translation unit sees them.
//
// The tile kernels are instantiated in their own translation units (gemm_x_<type>.hip: 128x128, gemm8r, gemm384;
// gemm4d_<type>.hip: the four-wave direct-to-LDS tile with its epilogue instantiations) so that hipcc compiles them in parallel (zett_amd/build.py) and an edit to one kernel
// does not rebuild the others.  zett_hip.hip sees only these non-template entry points.
//
//   variant: 1 = 128x128, 2 = 256x256 register-staged eight-wave (gemm8r), 3 = 384x256 LDS-DMA (gemm384),
//            7 = 256x256 four-wave direct-to-LDS (gemm4d), 8 = 7 with the generic epilogue drain
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "common.hip.h"      // GemmOptions
#include "gemm.hip.h"

namespace zett {

hipError_t launch_gemm_variant(int variant, const GemmArgs<f16_t>& g, hipStream_t stream);
hipError_t launch_gemm_variant(int variant, const GemmArgs<bf16_t>& g, hipStream_t stream);
hipError_t launch_gemm_variant(int variant, const GemmArgs<float>& g, hipStream_t stream);

// per-type pieces (defined in the translation units named above)
hipError_t launch_gemm_x(int variant, const GemmArgs<f16_t>& g, hipStream_t stream);
hipError_t launch_gemm_x(int variant, const GemmArgs<bf16_t>& g, hipStream_t stream);
hipError_t launch_gemm_x(int variant, const GemmArgs<float>& g, hipStream_t stream);
hipError_t launch_gemm_4d(const GemmArgs<f16_t>& g, hipStream_t stream, bool generic_epilogue);
hipError_t launch_gemm_4d(const GemmArgs<bf16_t>& g, hipStream_t stream, bool generic_epilogue);
// (zett_forward_into) >= 0 when a gemm4d launch (variant 7) of these arguments stores into g.epi.dst itself: the output heads'
// F32_SCALE / F32_SCALE_FOLD epilogues with an aligned destination; -1 = the caller stages fp32 rows and converts them
int gemm_4d_dst_mode(const GemmArgs<f16_t>& g);
int gemm_4d_dst_mode(const GemmArgs<bf16_t>& g);
inline int gemm_4d_dst_mode(const GemmArgs<float>&) { return -1; }
// the epilogue a gemm4d launch (variant 7; generic_epilogue: 8) of these arguments gets: gemm4d_dst_mode with a destination, else
// gemm4d_epi_mode (a G4D_EPI_* of gemm4d.hip.h); -1 = no instantiation carries it, the launch would be refused
int gemm_4d_launch_mode(const GemmArgs<f16_t>& g, bool generic_epilogue);
int gemm_4d_launch_mode(const GemmArgs<bf16_t>& g, bool generic_epilogue);
inline int gemm_4d_launch_mode(const GemmArgs<float>&, bool) { return -1; }

// The tile variant a launch of the forward takes (Runner::gemm of zett_hip.hip and zett_op_fwd_gemm of gemm_entry.hip: the one rule).
// a_rows_readable: rows the A operand buffer can be read for (the 384-row tile does not clamp rows).
template <typename T>
inline int gemm_variant_for(const GemmOptions& o, long a_rows_readable, int M, int N, int K, const GemmEpilogue<T>& e) {
    // Tile choice.  Small problems: 128x128.  Otherwise the 256x256 register-staged eight-wave kernel (gemm8r), unless the 384x256
    // LDS-DMA tile needs fewer rounds over the 256 CUs (it runs ~1.7x as long per tile): wave quantisation decides, e.g. M = 5 111
    // at N = 4096.  The 384-row kernel has no registers to spare for a residual or scale/shift epilogue (168 per wave: it would
    // spill to scratch, and no kernel with scratch is ever launched) and does not clamp rows, so A must have `a_rows_readable` >=
    // tiles*384 rows (every A operand of the forward is a workspace buffer with that slack) and N must be a multiple of 256.  (The
    // kernels that led to gemm8r and gemm4d -- four-wave register-staged, eight-wave LDS-DMA, gemm8r on 16x16x32 MFMAs -- live in
    // tools/experiments/ with tools/gemm_bench on the `experiments` branch.)
    constexpr bool is_f32 = std::is_same<T, float>::value;
    int variant = o.gemm_variant;
    if (variant == 0) {
        variant = (M > 128 && N > 128) ? 2 : 1;
        if (variant != 1 && N % 256 == 0 && !e.scale && !e.residual) {
            const long t256 = (long)((M + 255) / 256) * (N / 256), t384 = (long)((M + 383) / 384) * (N / 256);
            const double c256 = (double)((t256 + 255) / 256), c384 = 1.7 * (double)((t384 + 255) / 256);
            if (c384 < c256) variant = 3;
        }
    }
    if (variant == 3 && (N % 256 != 0 || (long)((M + 383) / 384) * 384 > a_rows_readable || e.scale || e.shift || e.residual || e.range_final)) variant = 2;
    // 16-bit operands, K >= 2048: the four-wave direct-to-LDS tile on 16x16x32 MFMAs (4-8 % ahead of the
    // register-staged eight-wave kernels on the launches of the benchmark step; identical bits).
    if (o.gemm_variant == 0 && variant == 2 && !is_f32 && K >= o.gemm4d_min_k) variant = 7;
    if ((variant == 7 || variant == 8) && is_f32) variant = 2;
    // the large tiles drain eight columns per lane with 16-byte accesses
    const bool wide_ok = N % 8 == 0 && (!e.out_lo || e.ld_lo % 8 == 0) && e.ld_f32 % 4 == 0 && (!e.residual || e.ld_res % 4 == 0) &&
                         (e.split_col >= N || e.split_col % 8 == 0);
    if (variant != 1 && !wide_ok) variant = 1;
    if (e.residual && (e.scale || e.shift)) variant = 1;      // the large tiles compile their residual epilogues without the Rescaler
    if (e.stats_part || e.fold_stats) variant = 7;       // LayerNorm-fold launches exist in gemm4d only (any M)
    return variant;
}

// GemmArgs::row0 as the launcher of gemm4d reads it (gemm4d.hip.h launch_gemm4d), from the gemm_tail_split option
inline int gemm_row0_for(int gemm_tail_split, int M) {
    return gemm_tail_split == 1 ? -1 : gemm_tail_split == 2 ? ((M / 2 + 255) / 256) * 256 : gemm_tail_split == 3 ? -2 : 0;
}

// The arguments of one launch under the options `o`: what the launchers read of them besides the variant (Runner::gemm and zett_op_fwd_gemm)
template <typename T>
inline GemmArgs<T> gemm_args_for(const GemmOptions& o, const T* A, int lda, const T* W, int ldw, int M, int N, int K, const GemmEpilogue<T>& e) {
    GemmArgs<T> g{A, lda, W, ldw, M, N, K, e};
    g.tile_order = o.gemm_tile_order;
    g.group = o.gemm_group;
    g.row0 = gemm_row0_for(o.gemm_tail_split, M);
    return g;
}

}  // namespace zett
