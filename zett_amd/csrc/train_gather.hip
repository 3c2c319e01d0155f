// train_gather.hip — the indexed-row primitives of the training step (include/zett_hip.h, "training use"): gather / scatter-add
// of rows by an index, and the source-embedding gather with its in_scaler / fallback select and its two backward forms.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "train_common.hip.h"

using namespace zett;

namespace {

// ---- indexed rows: out[r] = (a ? a[r] : 0) + src[idx[r]];  dst[idx[r]] += src[r] -------------------------------------------
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ a, const float* __restrict__ src, int ld_src, const int32_t* __restrict__ idx,
                                                          float* __restrict__ out, int cols) {
    const size_t r = blockIdx.x;
    const float* s = src + (size_t)idx[r] * ld_src;
    for (int c = threadIdx.x; c < cols; c += 256) out[r * cols + c] = (a ? a[r * cols + c] : 0.f) + s[c];
}
__global__ __launch_bounds__(256) void scatter_add_rows_kernel(float* __restrict__ dst, int ld_dst, const int32_t* __restrict__ idx, const float* __restrict__ src,
                                                               int cols) {
    const size_t r = blockIdx.x;
    float* d = dst + (size_t)idx[r] * ld_dst;
    for (int c = threadIdx.x; c < cols; c += 256) atomicAdd(d + c, src[r * cols + c]);
}

// ---- source-embedding gather (A2 + A3) and its backward -----------------------------------------------------------------
// x[t] = id < V0 ? sw * src[id] + sb : fallback[id - V0]
template <typename TS>
__global__ __launch_bounds__(256) void gather_fwd_kernel(const int32_t* __restrict__ ids, int64_t T, const TS* __restrict__ src, int e_in, int v0,
                                                         const float* __restrict__ fallback, const float* __restrict__ sw, const float* __restrict__ sb,
                                                         float* __restrict__ x) {
    const int64_t t = blockIdx.x;
    if (t >= T) return;
    const int id = ids[t];
    for (int c = threadIdx.x; c < e_in; c += 256) {
        float v;
        if (id >= v0) v = fallback[(size_t)(id - v0) * e_in + c];
        else { v = load1(src + (size_t)id * e_in + c); if (sw) v = sw[c] * v + sb[c]; }
        x[(size_t)t * e_in + c] = v;
    }
}
// dfallback[id - V0] += dx[t] (atomics: few rows); prod[t] = dx[t] * src[id] and keep[t] = dx[t] for source rows, 0 for fallback
// rows — their column sums are d in_scaler.w and d in_scaler.b.  FB = false: prod and keep only, by the same expressions, no atomic;
// d fallback is then the fixed-order sum of dx over the plan of ids - v0 (zett_op_embed_lookup_plan_base, zett_op_embed_lookup_bwd)
template <typename TS, bool FB>
__global__ __launch_bounds__(256) void gather_bwd_kernel(const int32_t* __restrict__ ids, int64_t T, const TS* __restrict__ src, int e_in, int v0,
                                                         const float* __restrict__ dx, float* __restrict__ dfallback, float* __restrict__ prod,
                                                         float* __restrict__ keep) {
    const int64_t t = blockIdx.x;
    if (t >= T) return;
    const int id = ids[t];
    for (int c = threadIdx.x; c < e_in; c += 256) {
        const float g = dx[(size_t)t * e_in + c];
        if (id >= v0) {
            if constexpr (FB) atomicAdd(dfallback + (size_t)(id - v0) * e_in + c, g);
            prod[(size_t)t * e_in + c] = 0.f; keep[(size_t)t * e_in + c] = 0.f;
        } else {
            prod[(size_t)t * e_in + c] = g * load1(src + (size_t)id * e_in + c);
            keep[(size_t)t * e_in + c] = g;
        }
    }
}

}  // namespace

extern "C" {

int zett_op_gather_rows_f32(const float* a, const float* src, int32_t ld_src, const int32_t* idx, float* out, int64_t rows, int32_t cols, void* stream) {
    if (!src || !idx || !out) return fail(ZETT_E_INVALID, "null argument");
    if (rows <= 0 || cols <= 0) return 0;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, a, src, ld_src, idx, out, cols);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_scatter_add_rows_f32(float* dst, int32_t ld_dst, const int32_t* idx, const float* src, int64_t rows, int32_t cols, void* stream) {
    if (!dst || !idx || !src) return fail(ZETT_E_INVALID, "null argument");
    if (rows <= 0 || cols <= 0) return 0;
    hipLaunchKernelGGL(scatter_add_rows_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, dst, ld_dst, idx, src, cols);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_gather_fwd_f32(const int32_t* ids, int64_t n_tokens, const void* src, int32_t src_dtype, int32_t e_in, int32_t v0, const float* fallback,
                           const float* sw, const float* sb, float* x, void* stream) {
    if (!ids || !src || !fallback || !x || !is_dtype(src_dtype)) return fail(ZETT_E_INVALID, "bad gather arguments");
    if (n_tokens <= 0) return 0;
    const dim3 grid((unsigned)n_tokens), block(256);
    hipStream_t st = (hipStream_t)stream;
    with_dtype(src_dtype, [&](auto dt) {
        using TS = elem_t<decltype(dt)::value>;
        hipLaunchKernelGGL(gather_fwd_kernel<TS>, grid, block, 0, st, ids, n_tokens, (const TS*)src, e_in, v0, fallback, sw, sb, x);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_gather_bwd_f32(const int32_t* ids, int64_t n_tokens, const void* src, int32_t src_dtype, int32_t e_in, int32_t v0, const float* dx,
                           float* dfallback, float* prod, float* keep, void* stream) {
    if (!ids || !src || !dx || !dfallback || !prod || !keep || !is_dtype(src_dtype)) return fail(ZETT_E_INVALID, "bad gather arguments");
    if (n_tokens <= 0) return 0;
    const dim3 grid((unsigned)n_tokens), block(256);
    hipStream_t st = (hipStream_t)stream;
    with_dtype(src_dtype, [&](auto dt) {
        using TS = elem_t<decltype(dt)::value>;
        hipLaunchKernelGGL((gather_bwd_kernel<TS, true>), grid, block, 0, st, ids, n_tokens, (const TS*)src, e_in, v0, dx, dfallback, prod, keep);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_gather_bwd_rows_f32(const int32_t* ids, int64_t n_tokens, const void* src, int32_t src_dtype, int32_t e_in, int32_t v0, const float* dx, float* prod,
                                float* keep, void* stream) {
    if (!ids || !src || !dx || !prod || !keep) return fail(ZETT_E_INVALID, "null argument");
    if (!is_dtype(src_dtype)) return fail(ZETT_E_INVALID, "unknown source dtype %d", (int)src_dtype);
    if (n_tokens < 0 || n_tokens > 0x7fffffffLL || e_in <= 0 || v0 < 0)
        return fail(ZETT_E_INVALID, "the gather needs 0 <= n_tokens < 2^31 (a workgroup each), e_in > 0 and v0 >= 0 (n_tokens = %lld, e_in = %d, v0 = %d)", (long long)n_tokens,
                    (int)e_in, (int)v0);
    if (n_tokens == 0) return 0;
    const dim3 grid((unsigned)n_tokens), block(256);
    hipStream_t st = (hipStream_t)stream;
    with_dtype(src_dtype, [&](auto dt) {
        using TS = elem_t<decltype(dt)::value>;
        hipLaunchKernelGGL((gather_bwd_kernel<TS, false>), grid, block, 0, st, ids, n_tokens, (const TS*)src, e_in, v0, dx, (float*)nullptr, prod, keep);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
