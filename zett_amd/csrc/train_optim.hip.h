// train_optim.hip.h — what the two optimizer units (train_step.hip: gradient norm + AdamW; train_adafactor.hip) share, each once: the
// chunked work items of a multi-tensor launch and the search from an item to its tensor, the order in which a chunk is summed and
// cleared, the first four words of the step record (norm, clip coefficient, skipped step, step count) and the host loop that packs a
// caller's list into launch groups.  The orders and the skip rule are part of both optimizers' results.  Training only (build.py).
#pragma once

#include "train_common.hip.h"

namespace zett {

constexpr int kMaxGrid = 2048;                // 256 CUs x 8 workgroups
constexpr int64_t kChunk = ZETT_MT_CHUNK;     // elements of one (tensor, chunk) work item of a flat tensor

inline int64_t chunk_items(int64_t n) { return (n + kChunk - 1) / kChunk; }

// The tensor lists travel in the kernel arguments; start[t] = first work item of tensor t in this launch, start[n_tensors] = their
// number.  -> the tensor of `item`.
__device__ __forceinline__ int tensor_of(const int32_t* start, int n_tensors, int item) {
    int t = 0;
    while (t + 1 < n_tensors && start[t + 1] <= item) ++t;
    return t;
}

// The sum of a chunk's f(i) over the workgroup (fp32, fixed order): four sums per thread over 16-byte accesses where `vec` (four(i) ->
// f of elements i .. i + 3), one sum otherwise and over the ragged end (one(i)), (s0 + s1) + (s2 + s3), block_sum_pairwise.  Depth 74
// for a full 16-byte aligned chunk, 266 for one that is only 4-byte aligned.
template <typename F4, typename F1> __device__ __forceinline__ float chunk_sum(int len, bool vec, float* red /* [4] */, F4 four, F1 one) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int tail = 0;
    if (vec) {
        tail = len & ~3;
        for (int i = threadIdx.x * 4; i < tail; i += 1024) {
            const float4 x = four(i);
            s0 += x.x; s1 += x.y; s2 += x.z; s3 += x.w;
        }
    }
    for (int i = tail + threadIdx.x; i < len; i += 256) s0 += one(i);
    return block_sum_pairwise((s0 + s1) + (s2 + s3), red);
}
// ... of the squares of x[0 .. len)
__device__ __forceinline__ float chunk_sumsq(const float* __restrict__ x, int len, float* red /* [4] */) {
    return chunk_sum(len, ((uintptr_t)x & 15) == 0, red,
                     [&](int i) { const float4 v = *(const float4*)(x + i); return make_float4(v.x * v.x, v.y * v.y, v.z * v.z, v.w * v.w); },
                     [&](int i) { return x[i] * x[i]; });
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

// The sum of x[0 .. n) by one workgroup in float64: a thread's strided terms in index order (eight loads in flight), then the tree.
__device__ __forceinline__ double strided_sum_f64(const float* __restrict__ x, int64_t n, double* red /* [256] */) {
    double s = 0.0;
#pragma unroll 8
    for (int64_t i = threadIdx.x; i < n; i += 256) s += (double)x[i];
    return block_sum_f64(s, red);
}

// Words 0 - 3 of the step record from the sum of squares of every gradient, by one thread: record = { norm, coef, skip (int32), count
// (int32), ... }.  coef: optax.clip_by_global_norm — 1 below max_norm, max_norm / norm otherwise.  A norm that is not finite sets skip,
// makes coef 0 and leaves the count of applied updates alone.  -> the count before and after this step.
struct StepCount { int32_t before, after; };
__device__ __forceinline__ StepCount norm_words(double sumsq, double max_norm, float* __restrict__ record) {
    const double norm = sqrt(sumsq);
    const bool finite = isfinite(norm);
    int32_t* ri = (int32_t*)record;
    const StepCount count{ri[3], ri[3] + (finite ? 1 : 0)};
    record[0] = (float)norm;
    record[1] = !finite ? 0.f : (norm < max_norm ? 1.f : (float)(max_norm / norm));
    ri[2] = finite ? 0 : 1;
    ri[3] = count.after;
    return count;
}

// Host.  Packs the caller's entries 0 .. n into launch groups of at most `capacity` tensors.  add(k, i) writes entry i into slot k of the list
// being filled and returns its work items; an entry that returns 0 (no elements) takes no slot: the next one overwrites it.  start[0 .. k]
// (the list's own array) gets the first work item of every slot and their number; launch(k, items) gets every group that holds a tensor.
template <typename Add, typename Launch> void for_each_group(int n, int capacity, int32_t* start, Add add, Launch launch) {
    for (int i = 0; i < n;) {
        int k = 0, items = 0;
        for (; i < n && k < capacity; ++i) {
            const int m = add(k, i);
            if (!m) continue;
            start[k++] = items;
            items += m;
        }
        if (!k) break;
        start[k] = items;
        launch(k, items);
    }
}

}  // namespace zett
