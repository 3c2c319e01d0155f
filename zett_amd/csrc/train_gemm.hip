// train_gemm.hip — the dense contractions of the training step (include/zett_hip.h, "training use": zett_op_gemm_f32,
// zett_op_gemm_lo).  Forward, dgrad and wgrad are one contraction with swapped / transposed operands, so the library's TN GEMM
// family (gemm_launch.hip.h) serves all three:
//     forward   y[M,N]  = x[M,K]  · W[N,K]ᵀ                     (A = x,    W-operand = W)
//     dgrad     dx[M,K] = dy[M,N] · (Wᵀ)[K,N]ᵀ                  (A = dy,   W-operand = Wᵀ: train_operands.hip's transposes)
//     wgrad     dW[N,K] = (dyᵀ)[N,M] · (xᵀ)[K,M]ᵀ               (A = dyᵀ,  W-operand = xᵀ; M zero-padded to the K step)
// No kernel of its own: the pointer contract, the tile rule and the launch.  The one training unit that sees the GEMM launchers.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "gemm_launch.hip.h"
#include "train_common.hip.h"

using namespace zett;

// Pointer contract of zett_op_gemm_f32 / zett_op_gemm_lo (include/zett_hip.h).  Every tile fetches its operands as 16-byte
// pieces of a row (global_load_dwordx4 in the 128x128 tile, buffer_load_dwordx4 in gemm8r, 16-byte LDS-DMA requests in gemm4d):
// `a` and `w` are 16-byte aligned for all three or the call is refused.  bias, residual and out are fp32: 4-byte aligned or
// refused.  The 128x128 tile reads and writes them one float at a time and takes any such pointer; both 256x256 tiles (gemm8r's
// and gemm4d's drains, generic and streamlined) move them as float4, so they additionally need 16-byte aligned bases there.
static int gemm_pointers_ok(const void* a, const void* w, const float* bias, const float* residual, const float* out) {
    if (!aligned(a, 16) || !aligned(w, 16)) return fail(ZETT_E_INVALID, "operand pointers a and w must be 16-byte aligned");
    if (!aligned(bias, 4) || !aligned(residual, 4) || !aligned(out, 4)) return fail(ZETT_E_INVALID, "bias, residual and out must be 4-byte aligned");
    return 0;
}
// what the float4 drains of the 256x256 tiles need beyond the 128x128 tile: eight columns per lane, 16-byte rows and bases
static inline bool gemm_wide_ok(int n, const float* bias, const float* residual, int ld_res, const float* out, int ld_out) {
    return n % 8 == 0 && ld_out % 4 == 0 && (!residual || ld_res % 4 == 0) && aligned(out, 16) && aligned(residual, 16) && aligned(bias, 16);
}
// The tile: a 256x256 one where it pays and its 16-byte drains apply — for 16-bit operands the choice of the inference path, gemm4d
// (7) from K = 512 and gemm8r (2) below; fp32 has gemm8r only —, the 128x128 tile (1) otherwise.  Identical bits either way.
// (tests/test_gemm_direct_gpu.py expected_tile mirrors this rule and gemm4d_epi_mode's choice of drain)
static int gemm_tile_for(int64_t m, int n, int k, bool wide_ok, bool is_16bit) {
    if (!(m > 128 && n > 128 && wide_ok)) return 1;
    return is_16bit && k >= 512 ? 7 : 2;
}

// fp32 or 16-bit MFMA operands (checked by the entry points), fp32 accumulate and output
template <typename T>
static int gemm_go(const T* a, int lda, const T* w, int ldw, int64_t m, int n, int k, const float* bias, int act, const float* residual, int ld_res, float* out,
                   int ld_out, hipStream_t st) {
    GemmEpilogue<T> e{};
    e.split_col = 0x7fffffff;
    e.bias = bias; e.act = act; e.residual = residual; e.ld_res = ld_res; e.out_f32 = out; e.ld_f32 = ld_out;
    GemmOptions o;
    o.gemm_tail_split = 0;      // 256x256 tiles only: a training launch does not cut its last round (the forward's default does)
    const GemmArgs<T> g = gemm_args_for(o, a, lda, w, ldw, (int)m, n, k, e);
    const int variant = gemm_tile_for(m, n, k, gemm_wide_ok(n, bias, residual, ld_res, out, ld_out), !std::is_same<T, float>::value);
    const hipError_t err = launch_gemm_variant(variant, g, st);
    if (err != hipSuccess) return fail(ZETT_E_HIP, "gemm launch failed: %s", hipGetErrorString(err));
    return 0;
}

extern "C" {

int zett_op_gemm_f32(const float* a, int32_t lda, const float* w, int32_t ldw, int64_t m, int32_t n, int32_t k, const float* bias, int32_t act,
                     const float* residual, int32_t ld_res, float* out, int32_t ld_out, void* stream) {
    if (!a || !w || !out) return fail(ZETT_E_INVALID, "null argument");
    if (m <= 0 || n <= 0) return 0;
    if (k <= 0 || k % 32) return fail(ZETT_E_INVALID, "contraction width %d is not a positive multiple of 32", k);
    if (lda % 4 || ldw % 4) return fail(ZETT_E_INVALID, "operand leading dimensions must be multiples of 4 floats");
    if (m >= (int64_t)0x7fffffff) return fail(ZETT_E_INVALID, "too many rows");
    if (const int rc = gemm_pointers_ok(a, w, bias, residual, out)) return rc;
    return gemm_go<float>(a, lda, w, ldw, m, n, k, bias, act, residual, ld_res, out, ld_out, (hipStream_t)stream);
}

int zett_op_gemm_lo(int32_t prec, const void* a, int32_t lda, const void* w, int32_t ldw, int64_t m, int32_t n, int32_t k, const float* bias, int32_t act,
                    const float* residual, int32_t ld_res, float* out, int32_t ld_out, void* stream) {
    if (!a || !w || !out) return fail(ZETT_E_INVALID, "null argument");
    if (const int rc = lo_prec_ok(prec, "zett_op_gemm_lo takes")) return rc;
    if (m <= 0 || n <= 0) return 0;
    if (k <= 0 || k % 64) return fail(ZETT_E_INVALID, "contraction width %d is not a positive multiple of 64", k);
    if (lda % 8 || ldw % 8) return fail(ZETT_E_INVALID, "operand leading dimensions must be multiples of 8 elements");
    if (m >= (int64_t)0x7fffffff) return fail(ZETT_E_INVALID, "too many rows");
    if (const int rc = gemm_pointers_ok(a, w, bias, residual, out)) return rc;
    return with_lo(prec, [&](auto ar) {
        using T = typename decltype(ar)::type;
        return gemm_go<T>((const T*)a, lda, (const T*)w, ldw, m, n, k, bias, act, residual, ld_res, out, ld_out, (hipStream_t)stream);
    });
}

}  // extern "C"
