// train_step.hip — the parameter update of optax.chain(clip_by_global_norm, multi_transform({train: adamw, freeze: set_to_zero}))
// (train.py:591-656) as two multi-tensor kernels behind zett_op_grad_norm and zett_op_adamw (include/zett_hip.h, "training use").  The
// work items, the order of the sums and the first four words of the step record are train_optim.hip.h's, shared with train_adafactor.hip.
//
// Memory-bound: 16-byte accesses per lane where the pointers allow it (a scalar path where they do not), grids capped at 2048 workgroups
// with a grid stride.  The norm is per-workgroup partials plus a fixed-order second stage — no float atomics — so the results are the
// same bits on every run, whatever the grid.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/zett_hip.h"
#include "train_optim.hip.h"      // (and through it train_common.hip.h, common.hip.h)

using namespace zett;

namespace {

constexpr int kGroup = 64;                    // tensors per launch: the lists travel as kernel arguments (< 4 KB)

// The tensor list travels in the kernel arguments.  Work item = (tensor, chunk of kChunk elements); chunk_start: tensor_of's start.
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

// partials[partial_base + item] = sum of squares of the item's elements (fp32, chunk_sum's order)
__global__ __launch_bounds__(256) void sumsq_kernel(const NormList a, float* __restrict__ partials) {
    __shared__ float red[4];
    const int total = a.chunk_start[a.n_tensors];
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int t = tensor_of(a.chunk_start, a.n_tensors, item);
        const int64_t off = (int64_t)(item - a.chunk_start[t]) * kChunk;
        const int len = (int)std::min<int64_t>(kChunk, a.n[t] - off);
        const float s = chunk_sumsq(a.g[t] + off, len, red);
        if (threadIdx.x == 0) partials[a.partial_base + item] = s;
    }
}

// record = { norm, coef, skip (int32), step (int32), 1 - b1^step, 1 - b2^step, 0, 0 }: norm_words, then the new count's bias corrections
__global__ __launch_bounds__(256) void norm_finalize_kernel(const float* __restrict__ partials, int64_t total, double max_norm, double b1, double b2,
                                                            float* __restrict__ record) {
    __shared__ double red[256];
    const double s = strided_sum_f64(partials, total, red);
    if (threadIdx.x == 0) {
        const int32_t step = norm_words(s, max_norm, record).after;
        record[4] = (float)(1.0 - pow(b1, (double)step));
        record[5] = (float)(1.0 - pow(b2, (double)step));
        record[6] = record[7] = 0.f;
    }
}

__device__ __forceinline__ void adamw1(float& p, float g, float& m, float& v, const AdamHyper& h, float coef, float inv_c1, float inv_c2, float wd) {
    g *= coef;
    m = h.b1 * m + h.one_minus_b1 * g;
    v = h.b2 * v + h.one_minus_b2 * (g * g);
    p -= h.lr * ((m * inv_c1) / (sqrtf(v * inv_c2) + h.eps) + wd * p);
}

__global__ __launch_bounds__(256) void adamw_kernel(const AdamList a, const AdamHyper h, const float* __restrict__ record) {
    // A non-finite gradient norm: no parameter and no moment is written.  The gradients the caller asked to clear are cleared all the
    // same — left in place, the inf / NaN would be what the next backward accumulates into, and every later step would be skipped too.
    const bool skip = ((const int32_t*)record)[2] != 0;
    if (skip && !h.zero_grad) return;
    const float coef = record[1], inv_c1 = 1.f / record[4], inv_c2 = 1.f / record[5];
    const int total = a.chunk_start[a.n_tensors];
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int t = tensor_of(a.chunk_start, a.n_tensors, item);
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

}  // namespace

extern "C" {

int zett_op_grad_norm(const void* const* grads, const int64_t* numel, int32_t n_tensors, double max_norm, double b1, double b2, float* partials,
                      int64_t partials_capacity, float* record, void* stream) {
    if (n_tensors < 0 || (n_tensors && (!grads || !numel)) || !record) return fail(ZETT_E_INVALID, "null argument");
    int64_t total = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] < 0 || (numel[i] && !grads[i])) return fail(ZETT_E_INVALID, "tensor %d: bad pointer or element count", i);
        total += chunk_items(numel[i]);
    }
    if (total > partials_capacity || (total && !partials)) return fail(ZETT_E_INVALID, "partials holds %lld floats, %lld are needed (one per %lld elements of each tensor)",
                                                                      (long long)partials_capacity, (long long)total, (long long)kChunk);
    if (total >= 0x7fffffff) return fail(ZETT_E_INVALID, "too many elements");
    hipStream_t st = (hipStream_t)stream;
    NormList a{};
    for_each_group(n_tensors, kGroup, a.chunk_start,
                   [&](int k, int i) {
                       a.g[k] = (const float*)grads[i];
                       a.n[k] = numel[i];
                       return (int)chunk_items(numel[i]);
                   },
                   [&](int k, int items) {
                       a.n_tensors = k;
                       hipLaunchKernelGGL(sumsq_kernel, dim3(std::min(items, kMaxGrid)), dim3(256), 0, st, a, partials);
                       a.partial_base += items;
                   });
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
        total += chunk_items(numel[i]);
    }
    if (total >= 0x7fffffff) return fail(ZETT_E_INVALID, "too many elements");
    AdamHyper h{};
    h.lr = (float)lr; h.b1 = (float)b1; h.b2 = (float)b2; h.one_minus_b1 = (float)(1.0 - b1); h.one_minus_b2 = (float)(1.0 - b2);
    h.eps = (float)eps; h.wd = (float)weight_decay; h.zero_grad = zero_grad;
    hipStream_t st = (hipStream_t)stream;
    AdamList a{};
    for_each_group(n_tensors, kGroup, a.chunk_start,
                   [&](int k, int i) {
                       a.p[k] = (float*)params[i]; a.g[k] = (float*)grads[i]; a.m[k] = (float*)exp_avg[i]; a.v[k] = (float*)exp_avg_sq[i];
                       a.n[k] = numel[i];
                       a.flags[k] = flags[i];
                       return (int)chunk_items(numel[i]);
                   },
                   [&](int k, int items) {
                       a.n_tensors = k;
                       hipLaunchKernelGGL(adamw_kernel, dim3(std::min(items, kMaxGrid)), dim3(256), 0, st, a, h, record);
                   });
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
