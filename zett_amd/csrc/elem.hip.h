// elem.hip.h — the element types of the library and what is done to ONE element: conversions between fp32 and the 16-bit operand
// types, LayerNorm's affine step and the range guard.  Shared by the GEMM (gemm.hip.h), the row kernels (rowops.hip.h) and the
// host units, which need the types but no tile kernel (common.hip.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace zett {

typedef uint16_t bf16_t;   // storage type of bf16 activations / weights
typedef _Float16 f16_t;    // IEEE half: the third operand type (ZETT_PREC_F16)

__device__ __forceinline__ float bf16_to_f32(bf16_t v) { return __uint_as_float(((uint32_t)v) << 16); }
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {   // round to nearest even: v_cvt_pk_bf16_f32 on gfx950
    return __builtin_bit_cast(bf16_t, (__bf16)f);
}

// fp32 -> operand type of a GEMM (round to nearest even)
template <typename T> __device__ __forceinline__ T to_lo(float v);
template <> __device__ __forceinline__ float to_lo<float>(float v) { return v; }
template <> __device__ __forceinline__ bf16_t to_lo<bf16_t>(float v) { return f32_to_bf16(v); }
template <> __device__ __forceinline__ f16_t to_lo<f16_t>(float v) { return (f16_t)v; }
template <typename T> __device__ __forceinline__ float lo_to_f32(T v);
template <> __device__ __forceinline__ float lo_to_f32<float>(float v) { return v; }
template <> __device__ __forceinline__ float lo_to_f32<bf16_t>(bf16_t v) { return bf16_to_f32(v); }
template <> __device__ __forceinline__ float lo_to_f32<f16_t>(f16_t v) { return (float)v; }
template <typename T> __device__ __forceinline__ uint32_t pack2_lo(float a, float b);      // two 16-bit operands in a dword
template <> __device__ __forceinline__ uint32_t pack2_lo<bf16_t>(float a, float b) {
    typedef __attribute__((ext_vector_type(2))) float f32x2_t;
    typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
    const f32x2_t v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));      // one v_cvt_pk_bf16_f32
}
template <> __device__ __forceinline__ uint32_t pack2_lo<f16_t>(float a, float b) {
    typedef __attribute__((ext_vector_type(2))) _Float16 h2;
    const h2 v = {(f16_t)a, (f16_t)b};
    return __builtin_bit_cast(uint32_t, v);
}
template <typename T> __device__ __forceinline__ void unpack2_lo(uint32_t u, float& a, float& b);
template <> __device__ __forceinline__ void unpack2_lo<bf16_t>(uint32_t u, float& a, float& b) { a = __uint_as_float(u << 16); b = __uint_as_float(u & 0xffff0000u); }
template <> __device__ __forceinline__ void unpack2_lo<f16_t>(uint32_t u, float& a, float& b) {
    typedef __attribute__((ext_vector_type(2))) _Float16 h2;
    const h2 v = __builtin_bit_cast(h2, u);
    a = (float)v[0]; b = (float)v[1];
}

// LayerNorm's affine step, the ONE definition shared by the LayerNorm kernel (which writes the 16-bit operand of the
// next GEMM and two statistics per row) and by every consumer that needs the fp32 LayerNorm output again — the
// residual epilogues of gemm.hip.h and the position-0 readout: they recompute it from the pre-LayerNorm sum they read
// anyway, so the fp32 LayerNorm output is never stored (4 of the 10 bytes per element the LayerNorm kernel moved).
__device__ __forceinline__ float ln_affine(float x, float mean, float rstd, float g, float b) {
#pragma clang fp contract(off)
    return __builtin_fmaf((x - mean) * rstd, g, b);
}

// Largest finite value of the operand type: what a value written as a 16-bit operand is checked against.  bf16 and fp32
// share fp32's exponent range: only the half type can overflow where the fp32 value was finite.
template <typename T> struct LoRange { static constexpr bool checked = false; static constexpr float limit = 0.f; };
template <> struct LoRange<f16_t> { static constexpr bool checked = true; static constexpr float limit = 65504.0f; };
// true where v would not survive: beyond the limit, or NaN (the comparison is false for NaN)
__device__ __forceinline__ bool out_of_range(float v, float limit) { return !(__builtin_fabsf(v) <= limit); }
constexpr float ZETT_F32_MAX = 3.402823466e38f;
constexpr int ZETT_RANGE_BIT_SOURCE = 1, ZETT_RANGE_BIT_ACTIVATION = 2, ZETT_RANGE_BIT_OUTPUT = 4, ZETT_RANGE_BIT_WEIGHT = 8, ZETT_RANGE_BIT_DEST = 16;
// Destination store (zett_forward_into): true where a FINITE fp32 value became inf in the destination type.  Only half can: a value
// rounds to inf from 65520 up (65504 + half an ulp); bf16 and fp32 share fp32's exponent range.
template <typename OT> __device__ __forceinline__ bool dest_overflow(float v) {
    if constexpr (std::is_same<OT, f16_t>::value) { const float a = __builtin_fabsf(v); return a >= 65520.0f && a <= 3.402823466e38f; }
    else return false;
}
__device__ __forceinline__ void range_report(int32_t* flag, bool bad, int bit) {
    if (bad && flag) atomicOr(flag, bit);      // (never taken on a healthy checkpoint)
}

}  // namespace zett
