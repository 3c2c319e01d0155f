// train_dist.hip — the embedding-distance losses of the reference's trainer (identity warm-up, train.py:941-960; lexical loss,
// train.py:1086-1141) with their gradient, and the single-token mask the lexical loss takes (include/zett_hip.h, "training use").
//
// Memory-bound: 16-byte accesses per lane on fp32 data where the pointers allow it (a scalar path where they do not; a 16-bit target row
// is read 8 bytes per lane, four elements beside the float4 of the prediction), grids capped at 2048 workgroups with a grid stride.  The
// loss is per-row values plus a fixed-order second stage in float64 — no float atomics — so the bits are the same on every run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "train_common.hip.h"

using namespace zett;

namespace {

constexpr int kMaxGrid = 2048;                // 256 CUs x 8 workgroups
constexpr float kHuberDelta = 1e-3f, kHuberCorrection = 30.f;      // train.py:1107-1108

__device__ __forceinline__ int64_t target_row(const void* ids, int ids64, int64_t ids_stride, int64_t r, int64_t src_rows) {
    const int64_t id = load_id(ids, ids64, r * ids_stride);
    return id < 0 ? 0 : (id >= src_rows ? src_rows - 1 : id);          // (JAX's gather rule: out-of-range indices are clamped)
}

// per-element distance term and its derivative in e = pred - target (kind: 0 mse, 1 rmse, 2 huber)
template <int KIND> __device__ __forceinline__ float dist_term(float e) {
    if (KIND == ZETT_DIST_HUBER) {                  // zett/utils.py huber_loss: 0.5 q^2 + delta (|e| - q), q = min(|e|, delta)
        const float a = fabsf(e), q = fminf(a, kHuberDelta);
        return 0.5f * q * q + kHuberDelta * (a - q);
    }
    return e * e;
}
template <int KIND> __device__ __forceinline__ float dist_grad(float e) {
    if (KIND == ZETT_DIST_HUBER) return fminf(fmaxf(e, -kHuberDelta), kHuberDelta);      // (/ delta / 30 is in the row factor)
    if (KIND == ZETT_DIST_RMSE) return e;                                                // (/ ||e|| is in the row factor)
    return 2.f * e;
}

// One wave per row, four rows per workgroup.  row_dist[r] = distance(pred[r], target[r]) * mask[r], row_tnorm[r] = ||target[r]||.
template <int SD, int KIND>
__global__ __launch_bounds__(256) void dist_rows_kernel(const float* __restrict__ pred, int64_t ld_pred, const void* __restrict__ src, int64_t ld_src,
                                                        int64_t src_rows, int col0, const void* __restrict__ ids, int ids64, int64_t ids_stride,
                                                        const float* __restrict__ mask, int64_t n, int e, int vec_ok, float* __restrict__ row_dist,
                                                        float* __restrict__ row_tnorm) {
    using T = elem_t<SD>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
        const float* x = pred + r * ld_pred;
        const T* y = (const T*)src + target_row(ids, ids64, ids_stride, r, src_rows) * ld_src + col0;
        float d = 0.f, t = 0.f;
        int tail = 0;
        if (vec_ok) {
            tail = e & ~3;
            for (int c = lane * 4; c < tail; c += 256) {
                const float4 a = *(const float4*)(x + c), b = load4(y + c);
                d += (dist_term<KIND>(a.x - b.x) + dist_term<KIND>(a.y - b.y)) + (dist_term<KIND>(a.z - b.z) + dist_term<KIND>(a.w - b.w));
                t += (b.x * b.x + b.y * b.y) + (b.z * b.z + b.w * b.w);
            }
        }
        for (int c = tail + lane; c < e; c += 64) {
            const float b = load1(y + c);
            d += dist_term<KIND>(x[c] - b);
            t += b * b;
        }
        d = wave_sum(d);
        t = wave_sum(t);
        if (lane == 0) {
            if (KIND == ZETT_DIST_RMSE) d = sqrtf(d);
            if (KIND == ZETT_DIST_HUBER) d = d / kHuberDelta / kHuberCorrection;
            row_dist[r] = mask ? d * mask[r] : d;
            row_tnorm[r] = sqrtf(t);
        }
    }
}

// record = { loss, gradient scale, masked-row fraction, 0 }: one workgroup, double sums in a fixed order
__global__ __launch_bounds__(256) void dist_finalize_kernel(const float* __restrict__ row_dist, const float* __restrict__ row_tnorm, const float* __restrict__ mask,
                                                            int64_t n, int mode, float* __restrict__ record) {
    __shared__ double red[256];
    double sd = 0.0, st = 0.0, sm = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        sd += (double)row_dist[i];
        st += (double)row_tnorm[i];
        sm += mask ? (double)mask[i] : 1.0;
    }
    sd = block_sum_f64(sd, red);
    st = block_sum_f64(st, red);
    sm = block_sum_f64(sm, red);
    if (threadIdx.x == 0) {
        // mean: sum / n (train.py:942-946).  lexical: sum / (sum(mask) + EPSILON) / mean ||target|| over ALL rows (train.py:1121-1125)
        const double denom = mode == ZETT_LOSS_LEXICAL ? (sm + 1e-8) * (st / (double)n) : (double)n;
        record[0] = (float)(sd / denom);
        record[1] = (float)(1.0 / denom);
        record[2] = (float)(sm / (double)n);
        record[3] = 0.f;
    }
}

// dpred[r, :] (+)= upstream * scale * mask[r] * d distance / d pred[r, :]
template <int SD, int KIND>
__global__ __launch_bounds__(256) void dist_grad_kernel(const float* __restrict__ pred, int64_t ld_pred, const void* __restrict__ src, int64_t ld_src,
                                                        int64_t src_rows, int col0, const void* __restrict__ ids, int ids64, int64_t ids_stride,
                                                        const float* __restrict__ mask, const float* __restrict__ row_dist, int64_t n, int e, int vec_ok,
                                                        const float* __restrict__ record, const float* __restrict__ upstream, float* __restrict__ dpred,
                                                        int64_t ld_dpred, int accumulate) {
    using T = elem_t<SD>;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float base = upstream[0] * record[1];
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < n; r += (int64_t)gridDim.x * 4) {
        const float* x = pred + r * ld_pred;
        const T* y = (const T*)src + target_row(ids, ids64, ids_stride, r, src_rows) * ld_src + col0;
        float* o = dpred + r * ld_dpred;
        const float m = mask ? mask[r] : 1.f;
        float f = base * m;
        if (KIND == ZETT_DIST_HUBER) f = f / kHuberDelta / kHuberCorrection;
        if (KIND == ZETT_DIST_RMSE) {                   // d ||e|| / de = e / ||e||; 0 at e = 0 (the reference: NaN)
            const float dist = row_dist[r];             // = ||e|| * m
            f = (m != 0.f && dist != 0.f) ? f * (m / dist) : 0.f;
        }
        int tail = 0;
        if (vec_ok) {
            tail = e & ~3;
            for (int c = lane * 4; c < tail; c += 256) {
                const float4 a = *(const float4*)(x + c), b = load4(y + c);
                float4 g = make_float4(f * dist_grad<KIND>(a.x - b.x), f * dist_grad<KIND>(a.y - b.y), f * dist_grad<KIND>(a.z - b.z), f * dist_grad<KIND>(a.w - b.w));
                if (accumulate) {
#pragma clang fp contract(off)                          // old + g with g rounded first: accumulating adds exactly what a plain call writes
                    const float4 old = *(const float4*)(o + c);
                    g = make_float4(old.x + g.x, old.y + g.y, old.z + g.z, old.w + g.w);
                }
                *(float4*)(o + c) = g;
            }
        }
        for (int c = tail + lane; c < e; c += 64) {
            float g = f * dist_grad<KIND>(x[c] - load1(y + c));
            if (accumulate) {
#pragma clang fp contract(off)
                g = o[c] + g;
            }
            o[c] = g;
        }
    }
}

// mask[r] = every position after the first is pad (train.py:1092-1094)
__global__ __launch_bounds__(256) void single_token_mask_kernel(const void* __restrict__ ids, int ids64, int64_t n, int width, int64_t ld, int64_t pad,
                                                                float* __restrict__ mask) {
    for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
        bool single = true;
        for (int j = 1; j < width; ++j) {
            single = single && load_id(ids, ids64, r * ld + j) == pad;
        }
        mask[r] = single ? 1.f : 0.f;
    }
}
// what both passes check: shapes, the dtype, and whether every row start allows the 4-element accesses
int dist_args(const float* pred, int64_t ld_pred, const void* src, int32_t src_dtype, int64_t ld_src, int64_t src_rows, int32_t col0, const void* ids, int32_t ids_bytes,
              int64_t n, int32_t e, int32_t kind, int* vec_ok) {
    if (!pred || !src || !ids) return fail(ZETT_E_INVALID, "null argument");
    if (n <= 0 || e <= 0) return fail(ZETT_E_INVALID, "the loss needs at least one row and one column (n = %lld, e = %d)", (long long)n, (int)e);
    if (!is_dtype(src_dtype)) return fail(ZETT_E_INVALID, "unknown source dtype %d", (int)src_dtype);
    if (ids_bytes != 4 && ids_bytes != 8) return fail(ZETT_E_INVALID, "ids must be int32 or int64");
    if (kind != ZETT_DIST_MSE && kind != ZETT_DIST_RMSE && kind != ZETT_DIST_HUBER) return fail(ZETT_E_INVALID, "unknown distance kind %d", (int)kind);
    if (src_rows <= 0 || col0 < 0 || (int64_t)col0 + e > ld_src || ld_pred < e) return fail(ZETT_E_INVALID, "columns [%d, %d) do not fit the leading dimensions", (int)col0, (int)(col0 + e));
    const int es = src_dtype == ZETT_F32 ? 4 : 2;
    *vec_ok = ((uintptr_t)pred & 15) == 0 && ld_pred % 4 == 0 && ((uintptr_t)src & (uintptr_t)(4 * es - 1)) == 0 && ld_src % 4 == 0 && col0 % 4 == 0;
    return 0;
}

}  // namespace

extern "C" {

int zett_op_single_token_mask(const void* ids, int32_t ids_bytes, int64_t n, int32_t width, int64_t ld, int64_t pad_token_id, float* mask, void* stream) {
    if (!ids || !mask) return fail(ZETT_E_INVALID, "null argument");
    if (ids_bytes != 4 && ids_bytes != 8) return fail(ZETT_E_INVALID, "ids must be int32 or int64");
    if (n <= 0) return 0;
    if (width < 1 || ld < width) return fail(ZETT_E_INVALID, "bad surface-form width");
    const int grid = (int)std::min<int64_t>((n + 255) / 256, kMaxGrid);
    hipLaunchKernelGGL(single_token_mask_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, ids, ids_bytes == 8, n, width, ld, pad_token_id, mask);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_embed_dist_rows(const float* pred, int64_t ld_pred, const void* src, int32_t src_dtype, int64_t ld_src, int64_t src_rows, int32_t col0, const void* ids,
                            int32_t ids_bytes, int64_t ids_stride, const float* mask, int64_t n, int32_t e, int32_t kind, float* row_dist, float* row_tnorm,
                            void* stream) {
    int vec_ok = 0;
    if (int rc = dist_args(pred, ld_pred, src, src_dtype, ld_src, src_rows, col0, ids, ids_bytes, n, e, kind, &vec_ok)) return rc;
    if (!row_dist || !row_tnorm) return fail(ZETT_E_INVALID, "null argument");
    const int grid = (int)std::min<int64_t>((n + 3) / 4, kMaxGrid);
    hipStream_t st = (hipStream_t)stream;
    with_dtype(src_dtype, [&](auto dt) {
        constexpr int SD = decltype(dt)::value;
        const auto kernel = kind == ZETT_DIST_MSE ? dist_rows_kernel<SD, ZETT_DIST_MSE> : kind == ZETT_DIST_RMSE ? dist_rows_kernel<SD, ZETT_DIST_RMSE> : dist_rows_kernel<SD, ZETT_DIST_HUBER>;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, pred, ld_pred, src, ld_src, src_rows, col0, ids, ids_bytes == 8, ids_stride, mask, n, e, vec_ok, row_dist, row_tnorm);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_embed_dist_finalize(const float* row_dist, const float* row_tnorm, const float* mask, int64_t n, int32_t mode, float* record, void* stream) {
    if (!row_dist || !row_tnorm || !record) return fail(ZETT_E_INVALID, "null argument");
    if (n <= 0) return fail(ZETT_E_INVALID, "the loss needs at least one row");
    if (mode != ZETT_LOSS_MEAN && mode != ZETT_LOSS_LEXICAL) return fail(ZETT_E_INVALID, "unknown loss mode %d", (int)mode);
    hipLaunchKernelGGL(dist_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_dist, row_tnorm, mask, n, mode, record);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_embed_dist_grad(const float* pred, int64_t ld_pred, const void* src, int32_t src_dtype, int64_t ld_src, int64_t src_rows, int32_t col0, const void* ids,
                            int32_t ids_bytes, int64_t ids_stride, const float* mask, const float* row_dist, int64_t n, int32_t e, int32_t kind, const float* record,
                            const float* upstream, float* dpred, int64_t ld_dpred, int32_t accumulate, void* stream) {
    int vec_ok = 0;
    if (int rc = dist_args(pred, ld_pred, src, src_dtype, ld_src, src_rows, col0, ids, ids_bytes, n, e, kind, &vec_ok)) return rc;
    if (!row_dist || !record || !upstream || !dpred) return fail(ZETT_E_INVALID, "null argument");
    if (ld_dpred < e) return fail(ZETT_E_INVALID, "ld_dpred %lld < %d columns", (long long)ld_dpred, (int)e);
    vec_ok = vec_ok && ((uintptr_t)dpred & 15) == 0 && ld_dpred % 4 == 0;
    const int grid = (int)std::min<int64_t>((n + 3) / 4, kMaxGrid);
    hipStream_t st = (hipStream_t)stream;
    with_dtype(src_dtype, [&](auto dt) {
        constexpr int SD = decltype(dt)::value;
        const auto kernel = kind == ZETT_DIST_MSE ? dist_grad_kernel<SD, ZETT_DIST_MSE> : kind == ZETT_DIST_RMSE ? dist_grad_kernel<SD, ZETT_DIST_RMSE> : dist_grad_kernel<SD, ZETT_DIST_HUBER>;
        hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, pred, ld_pred, src, ld_src, src_rows, col0, ids, ids_bytes == 8, ids_stride, mask, row_dist, n, e, vec_ok, record, upstream,
                           dpred, ld_dpred, accumulate);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
