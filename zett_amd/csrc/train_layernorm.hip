// train_layernorm.hip — LayerNorm forward and backward of the training step (include/zett_hip.h, "training use"): row kernels
// that read a row once, into registers.  The forward can leave the next contraction's 16-bit operand beside its fp32 rows; the
// backward takes the residual branch's gradient as a second addend and carries the parameter gradients as per-workgroup partials.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "train_common.hip.h"

using namespace zett;

namespace {

// ---- LayerNorm ------------------------------------------------------------------------------------------------------
// y = (x - mean) * rstd * gamma + beta; stats[r] = (mean, rstd)   (two-pass variance, as torch.nn.LayerNorm).  A row is read
// once, into registers: a thread owns columns 4 (tid + 256 j) ... + 3, j < J (H <= 1024 J, H % 4 == 0).  y_lo (nullable): the
// same values as a 16-bit operand of the next contraction, written while they are in registers.
template <int J, typename T>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, int ld, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     float eps, float* __restrict__ y, float* __restrict__ stats, int R, int H, T* __restrict__ y_lo) {
    __shared__ float red[4];
    const int tid = threadIdx.x;
    for (int r = blockIdx.x; r < R; r += gridDim.x) {
        float4 v[J];
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = 4 * (tid + 256 * j);
            v[j] = c < H ? *(const float4*)(x + (size_t)r * ld + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            s += (v[j].x + v[j].y) + (v[j].z + v[j].w);
        }
        const float mean = block_sum_ltr(s, red) / (float)H;
        float q = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            if (4 * (tid + 256 * j) < H) {
                const float a = v[j].x - mean, b = v[j].y - mean, c = v[j].z - mean, d = v[j].w - mean;
                q += (a * a + b * b) + (c * c + d * d);
            }
        }
        const float rstd = 1.0f / sqrtf(block_sum_ltr(q, red) / (float)H + eps);
        if (tid == 0) { stats[2 * (size_t)r] = mean; stats[2 * (size_t)r + 1] = rstd; }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = 4 * (tid + 256 * j);
            if (c < H) {
                const float4 g = *(const float4*)(gamma + c), b = *(const float4*)(beta + c);
                const float4 o = make_float4(ln_affine(v[j].x, mean, rstd, g.x, b.x), ln_affine(v[j].y, mean, rstd, g.y, b.y),
                                             ln_affine(v[j].z, mean, rstd, g.z, b.z), ln_affine(v[j].w, mean, rstd, g.w, b.w));
                *(float4*)(y + (size_t)r * H + c) = o;
                if (y_lo) store4(y_lo + (size_t)r * H + c, o);      // the next contraction's operand
            }
        }
    }
}

// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma,  xhat = (x - mean) * rstd, dy = dy1 (+ dy2: the gradient
// arriving over the residual branch, added here instead of in a pass of its own).  The parameter gradients ride along:
// workgroup b walks rows b, b + gridDim.x, ... and keeps, per thread, the running sums of dy * xhat (-> dgamma) and dy (-> dbeta)
// of its columns; they leave as partials[b] = (dgamma part [H], dbeta part [H]) and one small column sum over the gridDim.x
// partials finishes them — the same result for the same grid, no atomics, and no [R, H] product written or read.
// A thread owns columns 4 (tid + 256 j) ... + 3, j < J (H <= 1024 J, H % 4 == 0); a row is read once, into registers.
template <int J>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const float* __restrict__ dy1, const float* __restrict__ dy2, const float* __restrict__ x, int ld,
                                                     const float* __restrict__ stats, const float* __restrict__ gamma, float* __restrict__ dx,
                                                     float* __restrict__ partials, int R, int H) {
    __shared__ float red[2][2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float4 gam[J], ag[J], ab[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = 4 * (tid + 256 * j);
        gam[j] = c < H ? *(const float4*)(gamma + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        ag[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        ab[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    int par = 0;
    for (int r = blockIdx.x; r < R; r += gridDim.x, par ^= 1) {
        const float mean = stats[2 * (size_t)r], rstd = stats[2 * (size_t)r + 1];
        float4 xh[J], d[J];
        float sg = 0.f, sgx = 0.f;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = 4 * (tid + 256 * j);
            xh[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            d[j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < H) {
                const float4 xv = *(const float4*)(x + (size_t)r * ld + c);
                d[j] = *(const float4*)(dy1 + (size_t)r * H + c);
                if (dy2) {
                    const float4 e = *(const float4*)(dy2 + (size_t)r * H + c);
                    d[j].x += e.x; d[j].y += e.y; d[j].z += e.z; d[j].w += e.w;
                }
                xh[j] = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd, (xv.w - mean) * rstd);
                const float4 g = make_float4(d[j].x * gam[j].x, d[j].y * gam[j].y, d[j].z * gam[j].z, d[j].w * gam[j].w);
                sg += (g.x + g.y) + (g.z + g.w);
                sgx += (g.x * xh[j].x + g.y * xh[j].y) + (g.z * xh[j].z + g.w * xh[j].w);
            }
        }
        sg = wave_sum(sg);
        sgx = wave_sum(sgx);
        if (lane == 0) { red[par][0][wave] = sg; red[par][1][wave] = sgx; }
        __syncthreads();                               // (the other parity's slots are rewritten only after the next barrier)
        const float mg = ((red[par][0][0] + red[par][0][1]) + (red[par][0][2] + red[par][0][3])) / (float)H;
        const float mgx = ((red[par][1][0] + red[par][1][1]) + (red[par][1][2] + red[par][1][3])) / (float)H;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int c = 4 * (tid + 256 * j);
            if (c < H) {
                float4 o;
                o.x = rstd * (d[j].x * gam[j].x - mg - xh[j].x * mgx);
                o.y = rstd * (d[j].y * gam[j].y - mg - xh[j].y * mgx);
                o.z = rstd * (d[j].z * gam[j].z - mg - xh[j].z * mgx);
                o.w = rstd * (d[j].w * gam[j].w - mg - xh[j].w * mgx);
                *(float4*)(dx + (size_t)r * H + c) = o;
                ag[j].x += d[j].x * xh[j].x; ag[j].y += d[j].y * xh[j].y; ag[j].z += d[j].z * xh[j].z; ag[j].w += d[j].w * xh[j].w;
                ab[j].x += d[j].x; ab[j].y += d[j].y; ab[j].z += d[j].z; ab[j].w += d[j].w;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = 4 * (tid + 256 * j);
        if (c < H) {
            *(float4*)(partials + ((size_t)blockIdx.x * 2) * H + c) = ag[j];
            *(float4*)(partials + ((size_t)blockIdx.x * 2 + 1) * H + c) = ab[j];
        }
    }
}

// f(std::integral_constant<int, J>{}): the groups of four columns a thread owns, J = 1 / 2 / 4 / 8 for h <= 1024 J (h <= 8192: the callers' check)
template <typename F> void with_ln_width(int h, F&& f) {
    const int j = (h + 1023) / 1024;
    if (j <= 1) f(std::integral_constant<int, 1>{});
    else if (j <= 2) f(std::integral_constant<int, 2>{});
    else if (j <= 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}

}  // namespace

extern "C" {

int zett_op_layernorm_fwd_f32(const float* x, int32_t ld, const float* gamma, const float* beta, float eps, float* y, float* stats,
                              int64_t rows, int32_t h, void* y_lo, int32_t prec, void* stream) {
    if (!x || !gamma || !beta || !y || !stats) return fail(ZETT_E_INVALID, "null argument");
    if (h < 4 || h % 4 || h > 8192 || ld % 4) return fail(ZETT_E_INVALID, "LayerNorm: 4 <= h <= 8192, h and ld multiples of 4");
    if ((((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)y) & 15) != 0 || ((uintptr_t)y_lo & 7) != 0)
        return fail(ZETT_E_INVALID, "LayerNorm needs 16-byte aligned rows");
    if (const int rc = y_lo ? lo_prec_ok(prec, "the 16-bit copy takes") : 0) return rc;
    if (rows <= 0) return 0;
    const dim3 grid((unsigned)std::min<int64_t>(rows, 16384));
    with_ln_width(h, [&](auto j) {
        with_lo(prec, [&](auto ar) {       // (no y_lo: the type is not used, any prec launches the bf16 instantiation)
            using T = typename decltype(ar)::type;
            hipLaunchKernelGGL((ln_fwd_kernel<decltype(j)::value, T>), grid, dim3(256), 0, (hipStream_t)stream, x, ld, gamma, beta, eps, y, stats, (int)rows, h, (T*)y_lo);
        });
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_layernorm_bwd_f32(const float* dy, const float* dy2, const float* x, int32_t ld, const float* stats, const float* gamma, float* dx,
                              float* partials, int32_t n_part, int64_t rows, int32_t h, void* stream) {
    if (!dy || !x || !stats || !gamma || !dx || !partials) return fail(ZETT_E_INVALID, "null argument");
    if (n_part < 1 || h < 4 || h % 4 || h > 8192 || ld % 4) return fail(ZETT_E_INVALID, "LayerNorm backward: 4 <= h <= 8192, h and ld multiples of 4, n_part >= 1");
    if ((((uintptr_t)dy | (uintptr_t)dy2 | (uintptr_t)x | (uintptr_t)gamma | (uintptr_t)dx | (uintptr_t)partials) & 15) != 0)
        return fail(ZETT_E_INVALID, "LayerNorm backward needs 16-byte aligned rows");
    if (rows < 0) rows = 0;                            // (no rows: the partials are still written, as zeros)
    with_ln_width(h, [&](auto j) {
        hipLaunchKernelGGL(ln_bwd_kernel<decltype(j)::value>, dim3(n_part), dim3(256), 0, (hipStream_t)stream, dy, dy2, x, ld, stats, gamma, dx, partials, (int)rows, h);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
