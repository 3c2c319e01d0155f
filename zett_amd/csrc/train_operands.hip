// train_operands.hip — what the training step prepares and combines around its contractions (include/zett_hip.h, "training
// use"): the 16-bit operands of the GEMMs (conversion, transposition, and one pass that makes everything a Linear's backward
// needs of a gradient), the fp32 transpose, column sums, the row dot product, three element-wise forms and the two GELUs with
// their derivatives.  The GELUs live here because transpose_lo_kernel applies gelu_grad1 to the gradient it transposes.
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

// ---- transposes / reductions / element-wise ----------------------------------------------------------------------
// out[c, r] = in[r, c] for r < R; out[c, r] = 0 for R <= r < Rpad   (ld_out >= Rpad)
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ in, int ld_in, float* __restrict__ out, int ld_out,
                                                        int R, int C, int Rpad) {
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;     // 32 x 8
    for (int k = ty; k < 32; k += 8) {
        const int r = r0 + k, c = c0 + tx;
        tile[k][tx] = (r < R && c < C) ? in[(size_t)r * ld_in + c] : 0.f;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) {
        const int c = c0 + k, r = r0 + tx;
        if (c < C && r < Rpad) out[(size_t)c * ld_out + r] = tile[tx][k];
    }
}

// 16-bit operands of the training GEMMs: out[r, c] = lo(in[r, c]) (columns zero-padded to cols_padded: launch_cast), and the
// transposed form out[c, r] = lo(in[r, c]) (rows zero-padded to rows_padded): conversion fused with the layout change.
// convert_lo4_kernel is the common case of the first (no column padding, widths multiples of 4): 16-byte loads, 8-byte stores, one
// row per workgroup pass
template <typename T>
__global__ __launch_bounds__(256) void convert_lo4_kernel(const float* __restrict__ in, int ld_in, T* __restrict__ out, int ld_out, int64_t rows, int cols) {
    const int c4 = cols >> 2;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        for (int c = threadIdx.x; c < c4; c += 256) store4(out + r * ld_out + 4 * c, load4(in + r * ld_in + 4 * c));
    }
}
__device__ __forceinline__ float gelu_fwd1(float x, int kind) { return kind == 1 ? gelu_tanh_f(x) : gelu_erf_f(x); }
__device__ __forceinline__ float gelu_grad1(float x, int kind) {
    if (kind == 1) {       // d/dx [0.5 x (1 + tanh u)], u = sqrt(2/pi) (x + 0.044715 x^3)
        const float u = 0.7978845608028654f * (x + 0.044715f * x * x * x);
        const float t = tanhf(u);
        return 0.5f * (1.0f + t) + 0.5f * x * (1.0f - t * t) * 0.7978845608028654f * (1.0f + 3.0f * 0.044715f * x * x);
    }
    return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);       // Phi(x) + x phi(x)
}

// four consecutive values of a row as floats: one access where all four exist and the row allows it, element-wise tail at the edges
template <typename T>
__device__ __forceinline__ float4 load4_edge(const T* __restrict__ row, int c, int C, bool vec_ok) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (c + 3 < C && vec_ok) return load4(row + c);
    if (c < C) v.x = load1(row + c);
    if (c + 1 < C) v.y = load1(row + c + 1);
    if (c + 2 < C) v.z = load1(row + c + 2);
    if (c + 3 < C) v.w = load1(row + c + 3);
    return v;
}

// 64 x 64 tiles through LDS: wide loads along the input rows (fp32 or, TIn = T, an operand that is already 16-bit), 8-byte stores
// (four converted values) along the output rows.
// One read of a gradient serves everything a Linear's backward needs from it: `plain` (nullable) gets the un-transposed 16-bit
// copy (dgrad's A operand), `colpart` (nullable, [ceil(R / 64), C]) the column sums of each 64-row band (their sum is the bias
// gradient: a deterministic two-level reduction, no atomics).  With `act_z` (nullable: the pre-activation of a GELU whose OUTPUT
// gradient `in` is) the value used everywhere is in * gelu'(act_z): the activation's backward costs no pass of its own and its
// fp32 result is never written.
template <typename T, typename TIn>
__global__ __launch_bounds__(256) void transpose_lo_kernel(const TIn* __restrict__ in, int ld_in, T* __restrict__ out, int ld_out, int R, int C, int Rpad,
                                                           T* __restrict__ plain, int ld_plain, float* __restrict__ colpart,
                                                           const float* __restrict__ act_z, int ld_z, int act_kind) {
    __shared__ float tile[64][65];
    const int c0 = blockIdx.x * 64, r0 = blockIdx.y * 64;
    const int t = threadIdx.x;
    const bool in_vec = (ld_in & 3) == 0, z_vec = (ld_z & 3) == 0;
    for (int k = t; k < 64 * 16; k += 256) {           // 64 rows x 16 groups of four columns
        const int rr = k >> 4, cc = (k & 15) << 2;
        const int r = r0 + rr, c = c0 + cc;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r < R) {
            v = load4_edge(in + (size_t)r * ld_in, c, C, in_vec);
            if (act_z) {
                const float4 z = load4_edge(act_z + (size_t)r * ld_z, c, C, z_vec);
                v.x *= gelu_grad1(z.x, act_kind); v.y *= gelu_grad1(z.y, act_kind); v.z *= gelu_grad1(z.z, act_kind); v.w *= gelu_grad1(z.w, act_kind);
            }
            if (plain) {
                if (c + 3 < C && ((ld_plain & 3) == 0)) store4(plain + (size_t)r * ld_plain + c, v);
                else {
                    if (c < C) plain[(size_t)r * ld_plain + c] = to_lo<T>(v.x);
                    if (c + 1 < C) plain[(size_t)r * ld_plain + c + 1] = to_lo<T>(v.y);
                    if (c + 2 < C) plain[(size_t)r * ld_plain + c + 2] = to_lo<T>(v.z);
                    if (c + 3 < C) plain[(size_t)r * ld_plain + c + 3] = to_lo<T>(v.w);
                }
            }
        }
        tile[rr][cc] = v.x; tile[rr][cc + 1] = v.y; tile[rr][cc + 2] = v.z; tile[rr][cc + 3] = v.w;
    }
    __syncthreads();
    if (colpart && r0 < R && t < 64 && c0 + t < C) {   // (bands past R exist only as zero padding of the transposed output)
        float s = 0.f;
#pragma unroll 8
        for (int rr = 0; rr < 64; ++rr) s += tile[rr][t];
        colpart[(size_t)blockIdx.y * C + c0 + t] = s;
    }
    for (int k = t; k < 64 * 16; k += 256) {           // 64 output rows (= input columns) x 16 groups of four input rows
        const int cc = k >> 4, rr = (k & 15) << 2;
        const int c = c0 + cc, r = r0 + rr;
        if (c >= C || r >= Rpad) continue;
        if (r + 3 < Rpad && ((ld_out & 3) == 0))
            store4(out + (size_t)c * ld_out + r, make_float4(tile[rr][cc], tile[rr + 1][cc], tile[rr + 2][cc], tile[rr + 3][cc]));
        else
            for (int j = 0; j < 4 && r + j < Rpad; ++j) out[(size_t)c * ld_out + r + j] = to_lo<T>(tile[rr + j][cc]);
    }
}

// op 0: out = a + b;  1: out = a * b;  2: out = a * vec[col] + vec2[col] (vec null: 1, vec2 null: 0);  3: out = a + s[row] * vec[col];
// 4: out = a * s[row] (a may be null: out = s[row] * vec[col]).  One thread per four consecutive elements of a row (cols % 4 == 0:
// 16-byte accesses, one division per four values) or per element (V = 1).
template <int V>
__global__ __launch_bounds__(256) void elementwise_kernel(int op, const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ vec,
                                                          const float* __restrict__ vec2, const float* __restrict__ s, float* __restrict__ out, int64_t n, int cols) {
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * V;
    for (; i < n; i += stride) {
        float av[V], bv[V], ov[V];
        if (V == 4) {
            if (a) *(float4*)av = *(const float4*)(a + i);
            if (b) *(float4*)bv = *(const float4*)(b + i);
        } else {
            if (a) av[0] = a[i];
            if (b) bv[0] = b[i];
        }
        int col = 0;
        int64_t row = 0;
        if (op >= 2) { row = i / cols; col = (int)(i - row * cols); }
        const float sr = (op >= 3) ? s[row] : 0.f;
#pragma unroll
        for (int e = 0; e < V; ++e) {
            switch (op) {
                case 0: ov[e] = av[e] + bv[e]; break;
                case 1: ov[e] = av[e] * bv[e]; break;
                case 2: ov[e] = (vec ? av[e] * vec[col + e] : av[e]) + (vec2 ? vec2[col + e] : 0.f); break;
                case 3: ov[e] = av[e] + sr * vec[col + e]; break;
                default: ov[e] = a ? av[e] * sr : sr * vec[col + e]; break;
            }
        }
        if (V == 4) *(float4*)(out + i) = *(float4*)ov;
        else out[i] = ov[0];
    }
}

// out[r] = sum_c a[r, c] * w[c] + (b ? b[0] : 0)
__global__ __launch_bounds__(256) void rowdot_kernel(const float* __restrict__ a, int ld, const float* __restrict__ w, const float* __restrict__ b,
                                                     float* __restrict__ out, int R, int C) {
    __shared__ float red[4];
    const int r = blockIdx.x;
    if (r >= R) return;
    float s = 0.f;
    for (int c = threadIdx.x; c < C; c += 256) s += a[(size_t)r * ld + c] * w[c];
    const float t = block_sum_ltr(s, red);
    if (threadIdx.x == 0) out[r] = t + (b ? b[0] : 0.f);
}

// ---- GELU -----------------------------------------------------------------------------------------------------------
// kind 1: F.gelu(approximate="tanh") (ProjectorBlock), 2: erf form (RobertaIntermediate) — the forward functions of gemm.hip.h
// V = 4: 16-byte accesses (n % 4 == 0, aligned), V = 1 otherwise
template <int V>
__global__ __launch_bounds__(256) void gelu_fwd_kernel(const float* __restrict__ z, float* __restrict__ h, int64_t n, int kind) {
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * V;
    for (; i < n; i += stride) {
        if (V == 4) {
            const float4 v = *(const float4*)(z + i);
            *(float4*)(h + i) = make_float4(gelu_fwd1(v.x, kind), gelu_fwd1(v.y, kind), gelu_fwd1(v.z, kind), gelu_fwd1(v.w, kind));
        } else {
            h[i] = gelu_fwd1(z[i], kind);
        }
    }
}
template <int V>
__global__ __launch_bounds__(256) void gelu_bwd_kernel(const float* __restrict__ z, const float* __restrict__ dh, float* __restrict__ dz, int64_t n, int kind) {
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * V;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * V;
    for (; i < n; i += stride) {
        if (V == 4) {
            const float4 v = *(const float4*)(z + i), g = *(const float4*)(dh + i);
            *(float4*)(dz + i) = make_float4(g.x * gelu_grad1(v.x, kind), g.y * gelu_grad1(v.y, kind), g.z * gelu_grad1(v.z, kind), g.w * gelu_grad1(v.w, kind));
        } else {
            dz[i] = dh[i] * gelu_grad1(z[i], kind);
        }
    }
}

// the 16-bit form of the forward: the activation as the next contraction's operand (its fp32 value is never stored)
template <typename T>
__global__ __launch_bounds__(256) void gelu_fwd_lo_kernel(const float* __restrict__ z, T* __restrict__ h, int64_t n, int kind) {
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * 4;
    for (; i < n; i += stride) {
        if (i + 3 < n) {
            const float4 v = *(const float4*)(z + i);
            store4(h + i, make_float4(gelu_fwd1(v.x, kind), gelu_fwd1(v.y, kind), gelu_fwd1(v.z, kind), gelu_fwd1(v.w, kind)));
        } else {
            for (int64_t j = i; j < n; ++j) h[j] = to_lo<T>(gelu_fwd1(z[j], kind));
        }
    }
}

// The width of the flat kernels (elementwise, gelu_fwd, gelu_bwd): f(std::integral_constant<int, V>{}, grid) with V = 4 where
// n % 4 == 0, `rows_ok` holds and every pointer given is 16-byte aligned (a null one is), V = 1 otherwise
template <typename F, typename... P>
void with_vec_width(int64_t n, bool rows_ok, F&& f, const P*... ptrs) {
    if (rows_ok && n % 4 == 0 && (aligned(ptrs, 16) && ...)) f(std::integral_constant<int, 4>{}, dim3(grid256(n / 4, 65535)));
    else f(std::integral_constant<int, 1>{}, dim3(grid256(n, 65535)));
}

// in_lo: the input is already a 16-bit operand of type `prec` (plain transposition), otherwise fp32
int transpose_lo_launch(int32_t prec, bool in_lo, const void* in, int32_t ld_in, void* out, int32_t ld_out, int64_t rows, int32_t cols, int64_t rows_padded,
                        void* plain, int32_t ld_plain, float* colpart, const float* act_z, int32_t ld_z, int32_t act_kind, void* stream) {
    if (!in || !out || rows_padded < rows || ld_out < rows_padded) return fail(ZETT_E_INVALID, "bad transpose arguments");
    if (const int rc = lo_prec_ok(prec, "the 16-bit transposes take")) return rc;
    if (rows <= 0 || cols <= 0) return 0;
    if (plain && ld_plain < cols) return fail(ZETT_E_INVALID, "bad leading dimension of the plain copy");
    if (act_z && (act_kind != 1 && act_kind != 2)) return fail(ZETT_E_INVALID, "activation kind must be 1 (tanh-GELU) or 2 (erf-GELU)");
    if (act_z && ld_z < cols) return fail(ZETT_E_INVALID, "bad leading dimension of the pre-activation");
    if (((uintptr_t)in & (in_lo ? 7 : 15)) != 0 || ((uintptr_t)out & 7) != 0 || ((uintptr_t)plain & 7) != 0 || ((uintptr_t)act_z & 15) != 0)
        return fail(ZETT_E_INVALID, "the 16-bit transposes need 16-byte aligned fp32 inputs and 8-byte aligned 16-bit buffers");
    const dim3 grid((cols + 63) / 64, (unsigned)((rows_padded + 63) / 64));
    with_lo(prec, [&](auto ar) {
        using T = typename decltype(ar)::type;
        auto go = [&](auto in_type) {
            using TIn = typename decltype(in_type)::type;
            hipLaunchKernelGGL((transpose_lo_kernel<T, TIn>), grid, dim3(256), 0, (hipStream_t)stream, (const TIn*)in, ld_in, (T*)out, ld_out, (int)rows, cols,
                               (int)rows_padded, (T*)plain, ld_plain, colpart, act_z, ld_z, act_kind);
        };
        if (in_lo) go(Arith<T>{});
        else go(Arith<float>{});
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int zett_op_convert_lo(int32_t prec, const float* in, int32_t ld_in, void* out, int32_t ld_out, int64_t rows, int32_t cols, int32_t cols_padded, void* stream) {
    if (!in || !out || cols_padded < cols || ld_out < cols_padded) return fail(ZETT_E_INVALID, "bad conversion arguments");
    if (const int rc = lo_prec_ok(prec, "zett_op_convert_lo takes")) return rc;
    if (rows <= 0 || cols <= 0) return 0;
    if (cols_padded == cols && cols % 4 == 0 && ld_in % 4 == 0 && ld_out % 4 == 0 && ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & 7) == 0) {
        const int grid = (int)std::min<int64_t>(rows, 65535);
        with_lo(prec, [&](auto ar) {
            using T = typename decltype(ar)::type;
            hipLaunchKernelGGL(convert_lo4_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, in, ld_in, (T*)out, ld_out, rows, cols);
        });
    } else {
        launch_cast(ZETT_F32, prec == ZETT_PREC_F16 ? ZETT_F16 : ZETT_BF16, in, ld_in, out, ld_out, rows, cols, cols_padded, (hipStream_t)stream);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_transpose_lo(int32_t prec, const float* in, int32_t ld_in, void* out, int32_t ld_out, int64_t rows, int32_t cols, int64_t rows_padded, void* stream) {
    return transpose_lo_launch(prec, false, in, ld_in, out, ld_out, rows, cols, rows_padded, nullptr, 0, nullptr, nullptr, 0, 0, stream);
}

int zett_op_transpose_lo16(int32_t prec, const void* in, int32_t ld_in, void* out, int32_t ld_out, int64_t rows, int32_t cols, int64_t rows_padded, void* stream) {
    return transpose_lo_launch(prec, true, in, ld_in, out, ld_out, rows, cols, rows_padded, nullptr, 0, nullptr, nullptr, 0, 0, stream);
}

int zett_op_grad_operands_lo(int32_t prec, const float* dy, int32_t ld, const float* act_z, int32_t ld_z, int32_t act_kind, int64_t rows, int32_t cols,
                             int64_t rows_padded, void* dy_lo, int32_t ld_lo, void* dy_t, int32_t ld_t, float* colsum_part, void* stream) {
    if (!dy_lo || !colsum_part) return fail(ZETT_E_INVALID, "null argument");
    return transpose_lo_launch(prec, false, dy, ld, dy_t, ld_t, rows, cols, rows_padded, dy_lo, ld_lo, colsum_part, act_z, ld_z, act_kind, stream);
}

int zett_op_transpose_f32(const float* in, int32_t ld_in, float* out, int32_t ld_out, int64_t rows, int32_t cols, int64_t rows_padded, void* stream) {
    if (!in || !out || rows_padded < rows || ld_out < rows_padded) return fail(ZETT_E_INVALID, "bad transpose arguments");
    if (rows <= 0 || cols <= 0) return 0;
    hipLaunchKernelGGL(transpose_kernel, dim3((cols + 31) / 32, (unsigned)((rows_padded + 31) / 32)), dim3(256), 0, (hipStream_t)stream,
                       in, ld_in, out, ld_out, (int)rows, cols, (int)rows_padded);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_colsum_f32(const float* in, int32_t ld, int64_t rows, int32_t cols, float* out, int32_t accumulate, void* stream) {
    if (!in || !out) return fail(ZETT_E_INVALID, "null argument");
    if (cols <= 0) return 0;
    launch_colsum(ZETT_F32, in, ld, rows, cols, out, accumulate, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_elementwise_f32(int32_t op, const float* a, const float* b, const float* vec, const float* vec2, const float* s, float* out,
                            int64_t n, int32_t cols, void* stream) {
    if (!out || op < 0 || op > 4 || cols <= 0) return fail(ZETT_E_INVALID, "bad elementwise arguments");
    if (n <= 0) return 0;
    with_vec_width(n, cols % 4 == 0, [&](auto v, dim3 grid) {       // (V = 4 also wants whole groups of four within a row)
        hipLaunchKernelGGL(elementwise_kernel<decltype(v)::value>, grid, dim3(256), 0, (hipStream_t)stream, op, a, b, vec, vec2, s, out, n, cols);
    }, a, b, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_rowdot_f32(const float* a, int32_t ld, const float* w, const float* b, float* out, int64_t rows, int32_t cols, void* stream) {
    if (!a || !w || !out) return fail(ZETT_E_INVALID, "null argument");
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(rowdot_kernel, dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, a, ld, w, b, out, (int)rows, cols);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_gelu_fwd_f32(const float* z, float* h, int64_t n, int32_t kind, void* stream) {
    if (!z || !h || (kind != 1 && kind != 2)) return fail(ZETT_E_INVALID, "bad gelu arguments");
    if (n <= 0) return 0;
    with_vec_width(n, true, [&](auto v, dim3 grid) {
        hipLaunchKernelGGL(gelu_fwd_kernel<decltype(v)::value>, grid, dim3(256), 0, (hipStream_t)stream, z, h, n, kind);
    }, z, h);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_gelu_fwd_lo(int32_t prec, const float* z, void* h_lo, int64_t n, int32_t kind, void* stream) {
    if (!z || !h_lo || (kind != 1 && kind != 2)) return fail(ZETT_E_INVALID, "bad gelu arguments");
    if (const int rc = lo_prec_ok(prec, "zett_op_gelu_fwd_lo takes")) return rc;
    if ((((uintptr_t)z) & 15) != 0 || (((uintptr_t)h_lo) & 7) != 0) return fail(ZETT_E_INVALID, "zett_op_gelu_fwd_lo needs a 16-byte aligned input and an 8-byte aligned output");
    if (n <= 0) return 0;
    const int grid = grid256((n + 3) / 4, 65535);
    with_lo(prec, [&](auto ar) {
        using T = typename decltype(ar)::type;
        hipLaunchKernelGGL(gelu_fwd_lo_kernel<T>, dim3(grid), dim3(256), 0, (hipStream_t)stream, z, (T*)h_lo, n, kind);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_gelu_bwd_f32(const float* z, const float* dh, float* dz, int64_t n, int32_t kind, void* stream) {
    if (!z || !dh || !dz || (kind != 1 && kind != 2)) return fail(ZETT_E_INVALID, "bad gelu arguments");
    if (n <= 0) return 0;
    with_vec_width(n, true, [&](auto v, dim3 grid) {
        hipLaunchKernelGGL(gelu_bwd_kernel<decltype(v)::value>, grid, dim3(256), 0, (hipStream_t)stream, z, dh, dz, n, kind);
    }, z, dh, dz);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
