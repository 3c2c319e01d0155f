// train_step.hip — what a training step needs around the differentiable forward (include/zett_hip.h, "training use"): the
// embedding-distance losses of the reference's trainer (identity warm-up, train.py:941-960; lexical loss, train.py:1086-1141)
// with their gradient, and the parameter update of optax.chain(clip_by_global_norm, multi_transform({train: adamw,
// freeze: set_to_zero})) (train.py:591-656) as two multi-tensor kernels.
//
// Everything here is memory-bound: 16-byte accesses per lane on fp32 data where the pointers allow it (a scalar path where they do
// not; a 16-bit target row is read 8 bytes per lane, four elements beside the float4 of the prediction),
// grids capped at 2048 workgroups with a grid stride, no LDS beyond the four words of a block sum.  Every reduction is
// per-workgroup partials plus a fixed-order second stage — no float atomics — so the results are the same bits on every run,
// whatever the grid.
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
constexpr int64_t kChunk = ZETT_MT_CHUNK;     // elements of one (tensor, chunk) work item of the multi-tensor kernels
constexpr int kGroup = 64;                    // tensors per launch: the lists travel as kernel arguments (< 4 KB)
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

// ---- multi-tensor kernels: the tensor list travels in the kernel arguments ------------------------------------------------
// Work item = (tensor, chunk of kChunk elements); chunk_start[t] = first work item of tensor t in this launch.
struct NormList {
    const float* g[kGroup];
    int64_t n[kGroup];
    int32_t chunk_start[kGroup + 1];
    int32_t n_tensors;
    int64_t partial_base;          // work items of the launches before this one
};
struct AdamList {
    float* p[kGroup];
    float* g[kGroup];
    float* m[kGroup];
    float* v[kGroup];
    int64_t n[kGroup];
    int32_t chunk_start[kGroup + 1];
    int32_t n_tensors;
    uint8_t flags[kGroup];         // ZETT_ADAMW_DECAY | ZETT_ADAMW_FROZEN
};
struct AdamHyper {
    float lr, b1, b2, one_minus_b1, one_minus_b2, eps, wd;
    int32_t zero_grad;
};
static_assert(sizeof(NormList) < 4096 && sizeof(AdamList) + sizeof(AdamHyper) + 8 < 4096, "tensor lists must fit the kernel-argument limit");

template <typename L> __device__ __forceinline__ int tensor_of(const L& a, int item) {
    int t = 0;
    while (t + 1 < a.n_tensors && a.chunk_start[t + 1] <= item) ++t;
    return t;
}

// partials[partial_base + item] = sum of squares of the item's elements (fp32, fixed order)
__global__ __launch_bounds__(256) void sumsq_kernel(const NormList a, float* __restrict__ partials) {
    __shared__ float red[4];
    const int total = a.chunk_start[a.n_tensors];
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int t = tensor_of(a, item);
        const int64_t off = (int64_t)(item - a.chunk_start[t]) * kChunk;
        const int len = (int)std::min<int64_t>(kChunk, a.n[t] - off);
        const float* g = a.g[t] + off;
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int tail = 0;
        if (((uintptr_t)g & 15) == 0) {
            tail = len & ~3;
            for (int i = threadIdx.x * 4; i < tail; i += 1024) {
                const float4 x = *(const float4*)(g + i);
                s0 += x.x * x.x; s1 += x.y * x.y; s2 += x.z * x.z; s3 += x.w * x.w;
            }
        }
        for (int i = tail + threadIdx.x; i < len; i += 256) s0 += g[i] * g[i];       // the ragged end, or a pointer that is only 4-byte aligned
        const float s = block_sum_pairwise((s0 + s1) + (s2 + s3), red);
        if (threadIdx.x == 0) partials[a.partial_base + item] = s;
    }
}

// record = { norm, coef, skip (int32), step (int32), 1 - b1^step, 1 - b2^step, 0, 0 }.  coef: optax.clip_by_global_norm — 1 below
// max_norm, max_norm / norm otherwise.  A norm that is not finite sets skip and leaves the step count alone.
__global__ __launch_bounds__(256) void norm_finalize_kernel(const float* __restrict__ partials, int64_t total, double max_norm, double b1, double b2,
                                                            float* __restrict__ record) {
    __shared__ double red[256];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < total; i += 256) s += (double)partials[i];
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) {
        const double norm = sqrt(s);
        const bool finite = isfinite(norm);
        int32_t* ri = (int32_t*)record;
        const int32_t step = ri[3] + (finite ? 1 : 0);
        record[0] = (float)norm;
        record[1] = !finite ? 0.f : (norm < max_norm ? 1.f : (float)(max_norm / norm));
        ri[2] = finite ? 0 : 1;
        ri[3] = step;
        record[4] = (float)(1.0 - pow(b1, (double)step));
        record[5] = (float)(1.0 - pow(b2, (double)step));
        record[6] = 0.f;
        record[7] = 0.f;
    }
}

__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const AdamHyper& h, float coef, float inv_c1, float inv_c2, float wd) {
    g *= coef;
    m = h.b1 * m + h.one_minus_b1 * g;
    v = h.b2 * v + h.one_minus_b2 * (g * g);
    p -= h.lr * ((m * inv_c1) / (sqrtf(v * inv_c2) + h.eps) + wd * p);
}

// g[0 .. len) = 0 by the whole workgroup: 16-byte stores where the pointer allows it
__device__ __forceinline__ void zero_chunk(float* __restrict__ g, int len) {
    int tail = 0;
    if (((uintptr_t)g & 15) == 0) {
        tail = len & ~3;
        for (int i = threadIdx.x * 4; i < tail; i += 1024) *(float4*)(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    for (int i = tail + threadIdx.x; i < len; i += 256) g[i] = 0.f;
}

__global__ __launch_bounds__(256) void adamw_kernel(const AdamList a, const AdamHyper h, const float* __restrict__ record) {
    // A non-finite gradient norm: no parameter and no moment is written.  The gradients the caller asked to clear are cleared all the
    // same — left in place, the inf / NaN would be what the next backward accumulates into, and every later step would be skipped too.
    const bool skip = ((const int32_t*)record)[2] != 0;
    if (skip && !h.zero_grad) return;
    const float coef = record[1], inv_c1 = 1.f / record[4], inv_c2 = 1.f / record[5];
    const int total = a.chunk_start[a.n_tensors];
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int t = tensor_of(a, item);
        const int64_t off = (int64_t)(item - a.chunk_start[t]) * kChunk;
        const int len = (int)std::min<int64_t>(kChunk, a.n[t] - off);
        float* g = a.g[t] + off;
        const int flags = a.flags[t];
        if (skip || (flags & ZETT_ADAMW_FROZEN)) {        // frozen = optax.set_to_zero: no update, no moments; the gradient is still cleared
            if (h.zero_grad) zero_chunk(g, len);
            continue;
        }
        float* p = a.p[t] + off;
        float* m = a.m[t] + off;
        float* v = a.v[t] + off;
        const float wd = (flags & ZETT_ADAMW_DECAY) ? h.wd : 0.f;
        int tail = 0;
        if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) {
            tail = len & ~3;
            for (int i = threadIdx.x * 4; i < tail; i += 1024) {
                float4 pp = *(const float4*)(p + i), mm = *(const float4*)(m + i), vv = *(const float4*)(v + i);
                const float4 gg = *(const float4*)(g + i);
                adamw1(pp.x, gg.x, mm.x, vv.x, h, coef, inv_c1, inv_c2, wd);
                adamw1(pp.y, gg.y, mm.y, vv.y, h, coef, inv_c1, inv_c2, wd);
                adamw1(pp.z, gg.z, mm.z, vv.z, h, coef, inv_c1, inv_c2, wd);
                adamw1(pp.w, gg.w, mm.w, vv.w, h, coef, inv_c1, inv_c2, wd);
                *(float4*)(p + i) = pp;
                *(float4*)(m + i) = mm;
                *(float4*)(v + i) = vv;
                if (h.zero_grad) *(float4*)(g + i) = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        for (int i = tail + threadIdx.x; i < len; i += 256) {      // the ragged end, or a pointer that is only 4-byte aligned
            float pp = p[i], mm = m[i], vv = v[i];
            adamw1(pp, g[i], mm, vv, h, coef, inv_c1, inv_c2, wd);
            p[i] = pp; m[i] = mm; v[i] = vv;
            if (h.zero_grad) g[i] = 0.f;
        }
    }
}

int64_t items_of(int64_t n) { return (n + kChunk - 1) / kChunk; }

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

int zett_op_grad_norm(const void* const* grads, const int64_t* numel, int32_t n_tensors, double max_norm, double b1, double b2, float* partials,
                      int64_t partials_capacity, float* record, void* stream) {
    if (n_tensors < 0 || (n_tensors && (!grads || !numel)) || !record) return fail(ZETT_E_INVALID, "null argument");
    int64_t total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] < 0 || (numel[i] && !grads[i])) return fail(ZETT_E_INVALID, "tensor %d: bad pointer or element count", i);
        total += items_of(numel[i]);
    }
    if (total > partials_capacity || (total && !partials)) return fail(ZETT_E_INVALID, "partials holds %lld floats, %lld are needed (one per %lld elements of each tensor)",
                                                                      (long long)partials_capacity, (long long)total, (long long)kChunk);
    if (total >= 0x7fffffff) return fail(ZETT_E_INVALID, "too many elements");
    hipStream_t st = (hipStream_t)stream;
    int64_t base = 0;
    for (int first = 0; first < n_tensors;) {
        NormList a{};
        int k = 0, items = 0;
        for (; first < n_tensors && k < kGroup; ++first) {
            if (!numel[first]) continue;
            a.g[k] = (const float*)grads[first];
            a.n[k] = numel[first];
            a.chunk_start[k] = items;
            items += (int)items_of(numel[first]);
            ++k;
        }
        if (!k) break;
        a.chunk_start[k] = items;
        a.n_tensors = k;
        a.partial_base = base;
        hipLaunchKernelGGL(sumsq_kernel, dim3(std::min(items, kMaxGrid)), dim3(256), 0, st, a, partials);
        base += items;
    }
    hipLaunchKernelGGL(norm_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)partials, total, max_norm, b1, b2, record);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_adamw(void* const* params, void* const* grads, void* const* exp_avg, void* const* exp_avg_sq, const int64_t* numel, const uint8_t* flags, int32_t n_tensors,
                  double lr, double b1, double b2, double eps, double weight_decay, int32_t zero_grad, const float* record, void* stream) {
    if (n_tensors < 0 || (n_tensors && (!params || !grads || !exp_avg || !exp_avg_sq || !numel || !flags)) || !record) return fail(ZETT_E_INVALID, "null argument");
    int64_t total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        const bool frozen = flags[i] & ZETT_ADAMW_FROZEN;
        if (numel[i] < 0 || (numel[i] && (!grads[i] || (!frozen && (!params[i] || !exp_avg[i] || !exp_avg_sq[i])))))
            return fail(ZETT_E_INVALID, "tensor %d: bad pointer or element count", i);
        total += items_of(numel[i]);
    }
    if (total >= 0x7fffffff) return fail(ZETT_E_INVALID, "too many elements");
    AdamHyper h{};
    h.lr = (float)lr; h.b1 = (float)b1; h.b2 = (float)b2; h.one_minus_b1 = (float)(1.0 - b1); h.one_minus_b2 = (float)(1.0 - b2);
    h.eps = (float)eps; h.wd = (float)weight_decay; h.zero_grad = zero_grad;
    hipStream_t st = (hipStream_t)stream;
    for (int first = 0; first < n_tensors;) {
        AdamList a{};
        int k = 0, items = 0;
        for (; first < n_tensors && k < kGroup; ++first) {
            if (!numel[first]) continue;
            a.p[k] = (float*)params[first]; a.g[k] = (float*)grads[first]; a.m[k] = (float*)exp_avg[first]; a.v[k] = (float*)exp_avg_sq[first];
            a.n[k] = numel[first];
            a.flags[k] = flags[first];
            a.chunk_start[k] = items;
            items += (int)items_of(numel[first]);
            ++k;
        }
        if (!k) break;
        a.chunk_start[k] = items;
        a.n_tensors = k;
        hipLaunchKernelGGL(adamw_kernel, dim3(std::min(items, kMaxGrid)), dim3(256), 0, st, a, h, record);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
