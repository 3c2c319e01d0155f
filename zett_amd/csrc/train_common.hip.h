// train_common.hip.h — the small device / host layer the training units (train_gemm.hip, train_operands.hip, train_layernorm.hip, train_attention.hip, train_gather.hip, train_dist.hip, train_step.hip,
// train_adafactor.hip, train_loss.hip, train_embed.hip, train_batch.hip, train_init.hip) share: element accessors over gemm.hip.h's conversions (to_lo, lo_to_f32, pack2_lo, unpack2_lo: widen on load —
// bf16 by the 16-bit left shift —, round to nearest even on store), the reductions, the id read and the splitmix64 finalizer.  (The zett_dtype ->
// storage-type map and the dtype dispatch of the launches — elem_t, is_dtype, with_dtype — are common.hip.h's: the forward uses
// them too.)  The device helpers here hold only conversions and additions, so a caller's `#pragma clang fp contract(off)` keeps
// its meaning.  Training only (zett_amd/build.py TRAINING_ONLY): no forward source includes it.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "gemm.hip.h"

namespace zett {

// ---- element accessors (fp32 / f16 / bf16 storage: elem_t, common.hip.h) -----------------------------------------------------------
template <typename T> __device__ __forceinline__ float load1(const T* p) { return lo_to_f32<T>(*p); }
template <typename T> __device__ __forceinline__ void store1(T* p, float v) { *p = to_lo<T>(v); }

// four consecutive elements, p aligned to four elements: one 16-byte (fp32) or 8-byte (16-bit) access
template <typename T> __device__ __forceinline__ float4 load4(const T* p) {
    if constexpr (std::is_same<T, float>::value) {
        return *(const float4*)p;
    } else {
        const uint2 u = *(const uint2*)p;
        float4 v;
        unpack2_lo<T>(u.x, v.x, v.y);
        unpack2_lo<T>(u.y, v.z, v.w);
        return v;
    }
}
template <typename T> __device__ __forceinline__ void store4(T* p, float4 v) {
    if constexpr (std::is_same<T, float>::value) *(float4*)p = v;
    else *(uint2*)p = make_uint2(pack2_lo<T>(v.x, v.y), pack2_lo<T>(v.z, v.w));
}

// W elements moved by one access (train_embed.hip: 1, 4 or 8), and their conversion.  Equal types copy the bits and never go through
// float: a bf16 -> bf16 or f16 -> f16 lookup keeps NaN payloads and signalling bits.
template <typename T, int W> struct alignas(sizeof(T) * W) Pack { T v[W]; };
template <typename TO, typename TI> struct Convert { static __device__ __forceinline__ TO go(TI x) { return to_lo<TO>(lo_to_f32<TI>(x)); } };
template <typename T> struct Convert<T, T> { static __device__ __forceinline__ T go(T x) { return x; } };

__device__ __forceinline__ int64_t load_id(const void* ids, int ids64, int64_t i) {
    return ids64 ? ((const int64_t*)ids)[i] : (int64_t)((const int32_t*)ids)[i];
}

// the finalizer of splitmix64, for the host (the keys of a call) and the device (a draw per position): zett_op_label_batch.  (The
// tokenizer sampler keeps its own device copy in tokenizer_sample.hip: that unit is not a training unit and does not include this header.)
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// ---- reductions -----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
// The two sums of a 256-thread workgroup differ in how the four wave results are added, and the bits of their callers depend on it:
// they are not interchangeable.
// left to right, ((r0 + r1) + r2) + r3: train_layernorm.hip (the forward's statistics), train_operands.hip (rowdot)
__device__ __forceinline__ float block_sum_ltr(float v, float* red /* [4] */) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}
// pairwise, (r0 + r1) + (r2 + r3): train_optim.hip.h (the sums of squares behind the gradient norm), train_adafactor.hip
__device__ __forceinline__ float block_sum_pairwise(float v, float* red /* [4] */) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
// 256 threads, a binary tree over LDS
__device__ __forceinline__ double block_sum_f64(double v, double* red /* [256] */) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const double s = red[0];
    __syncthreads();
    return s;
}

// ---- host side ------------------------------------------------------------------------------------------------------------------
// Declared here, DEFINED in train_loss.hip, which holds the one column-sum kernel and the one converting-copy kernel of the training
// units: out[c] (+)= sum_r in[r, c], and out[r, c] = convert(in[r, c]) with columns [cols, cols_padded) zero.  train_operands.hip
// (zett_op_colsum_f32, the general path of zett_op_convert_lo) links against them; they are internal to the library (hidden).
// Arguments are the callers' to check.
__attribute__((visibility("hidden"))) void launch_colsum(int32_t dtype, const void* in, int64_t ld, int64_t rows, int cols, float* out, int accumulate, hipStream_t st);
__attribute__((visibility("hidden"))) void launch_cast(int32_t in_dtype, int32_t out_dtype, const void* in, int64_t ld_in, void* out, int64_t ld_out, int64_t rows, int cols,
                                                       int cols_padded, hipStream_t st);

// The 16-bit operand type of a training primitive.  lo_prec_ok refuses anything but the two; `who_takes` opens the sentence
// ("zett_op_gemm_lo takes", "the 16-bit transposes take").  with_lo(prec, f) is f(Arith<f16_t | bf16_t>{}) for a prec that passed it
// (with_precision, common.hip.h, without the fp32 arm: no training kernel has one); returns what f returns.
inline int lo_prec_ok(int32_t prec, const char* who_takes) {
    if (prec != ZETT_PREC_BF16 && prec != ZETT_PREC_F16) return fail(ZETT_E_INVALID, "%s ZETT_PREC_BF16 or ZETT_PREC_F16", who_takes);
    return 0;
}
template <typename F> inline auto with_lo(int32_t prec, F&& f) {
    if (prec == ZETT_PREC_F16) return f(Arith<f16_t>{});
    return f(Arith<bf16_t>{});
}

}  // namespace zett
