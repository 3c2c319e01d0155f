// scan.hip.h — the integer prefix sums of the device code, once: a wave's inclusive scan, a workgroup's exclusive scan, the
// exclusive scan of an array (one workgroup, or chunked over many: the forward's plan, the retokenizer's block totals), and the
// compaction of byte flags into an ascending index list built from them.  Integers only (addition is associative: however a sum
// is bracketed, the bits are the same); the float reductions, whose order is part of their callers' results, live in
// train_common.hip.h.  The kernels and their launcher have internal linkage: a translation unit that includes the header gets its
// own copy (of the three small compaction kernels too, whether it launches them or not).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "common.hip.h"

namespace zett {

// the wave of a thread within its workgroup, in a scalar register
__device__ __forceinline__ int wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
// how many lanes below the calling one have their bit set in a ballot
__device__ __forceinline__ int lanes_below(uint64_t mask) { return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0)); }

// the sum of v over the lanes up to and including the calling one (every lane of the wave calls)
template <typename T> __device__ __forceinline__ T wave_inclusive_scan(T v) {
    static_assert(std::is_same<T, int>::value || std::is_same<T, long long>::value, "int or long long");
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T below = __shfl_up(v, o, 64);
        if (lane >= o) v += below;
    }
    return v;
}

// The sum of v over the threads below the calling one in a workgroup of N threads (every thread calls); *total: the sum over all N.
// A wave scan, the waves' sums through LDS, two barriers.  The first barrier lets a kernel call again with the same `lds`.
template <int N, typename T> __device__ __forceinline__ T block_exclusive_scan(T v, T* lds /* [N / 64] */, T* total = nullptr) {
    static_assert(N == 256 || N == 1024, "256 or 1024 threads");
    const int wave = wave_index();
    const T inc = wave_inclusive_scan(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 63) lds[wave] = inc;
    __syncthreads();
    T below = 0, all = 0;
#pragma unroll
    for (int w = 0; w < N / 64; ++w) {
        const T sum = lds[w];
        if (w < wave) below += sum;
        all += sum;
    }
    if (total) *total = all;
    return below + inc - v;
}

// ---- the exclusive scan of an int32 array in global memory ------------------------------------------------------------------
// Single-workgroup exclusive scan (n <= a few million): out[i] = sum(in[0..i)), out[n] = total.
static __global__ __launch_bounds__(1024) void exclusive_scan_kernel(const int32_t* __restrict__ in,
                                                              int32_t* __restrict__ out, int64_t n) {
    __shared__ int32_t s_waves[16];
    const int t = threadIdx.x;
    const int64_t per = (n + 1023) / 1024;
    const int64_t b = (int64_t)t * per, e = (b + per < n) ? b + per : n;
    int32_t s = 0;
    for (int64_t i = b; i < e; ++i) s += in[i];
    int32_t total;
    int32_t run = block_exclusive_scan<1024>(s, s_waves, &total);
    for (int64_t i = b; i < e; ++i) { const int32_t v = in[i]; out[i] = run; run += v; }
    if (t == 1023) out[n] = total;
}

// Multi-block exclusive scan for the plan arrays (V can be 250 k source ids, N 262 k rows: the single
// workgroup above takes 75-400 us on those).  Chunks of SCAN_CHUNK elements:
//   (1) scan_chunk_sums_kernel: sums[c] = sum of chunk c;
//   (2) exclusive_scan_kernel on sums (a few hundred entries) -> offs[c], offs[chunks] = total;
//   (3) scan_apply_kernel: out[i] = offs[c] + exclusive scan inside the chunk; out[n] = total.
constexpr int SCAN_CHUNK = 4096;          // 256 threads x 16 elements

static __global__ __launch_bounds__(256) void scan_chunk_sums_kernel(const int32_t* __restrict__ in, int64_t n, int32_t* __restrict__ sums) {
    __shared__ int32_t s_waves[4];
    const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK + threadIdx.x * 16;
    int32_t s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int64_t i = base + k; if (i < n) s += in[i]; }
    int32_t total;
    block_exclusive_scan<256>(s, s_waves, &total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

static __global__ __launch_bounds__(256) void scan_apply_kernel(const int32_t* __restrict__ in, int64_t n, const int32_t* __restrict__ offs,
                                                         int32_t* __restrict__ out) {
    __shared__ int32_t s_waves[4];
    const int64_t base = (int64_t)blockIdx.x * SCAN_CHUNK + threadIdx.x * 16;
    int32_t v[16];
    int32_t s = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int64_t i = base + k; v[k] = i < n ? in[i] : 0; s += v[k]; }
    int32_t run = offs[blockIdx.x] + block_exclusive_scan<256>(s, s_waves);
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int64_t i = base + k; if (i < n) out[i] = run; run += v[k]; }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[n] = offs[gridDim.x];
}

// out[0..n] = exclusive scan of in[0..n) (out[n] = total); scratch: 2*chunks + 1 ints
inline void launch_exclusive_scan(const int32_t* in, int32_t* out, int64_t n, int32_t* scratch, hipStream_t st) {
    if (n <= SCAN_CHUNK * 4) {        // small: one workgroup does it in one launch
        hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, st, in, out, n);
        return;
    }
    const int chunks = (int)((n + SCAN_CHUNK - 1) / SCAN_CHUNK);
    int32_t* sums = scratch;
    int32_t* offs = scratch + chunks;
    hipLaunchKernelGGL(scan_chunk_sums_kernel, dim3(chunks), dim3(256), 0, st, in, n, sums);
    hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, st, (const int32_t*)sums, offs, (int64_t)chunks);
    hipLaunchKernelGGL(scan_apply_kernel, dim3(chunks), dim3(256), 0, st, in, n, (const int32_t*)offs, out);
}

namespace {

// ---- byte flags -> the ascending list of the flagged items' indices ---------------------------------------------------------
// Three launches: count per segment of kSeg items (a wave owns a segment, so no launch waits for another workgroup), one
// workgroup scans the segment counts, place.
constexpr int kSeg = 1024;                  // items of one wave's segment: 16 per lane

// the flags of a lane's 16 items of segment seg, as a bit mask
__device__ __forceinline__ uint32_t lane_flags(const uint8_t* __restrict__ flags, int64_t np, int64_t seg, int lane) {
    const int64_t base = seg * kSeg + lane * 16;
    uint32_t bits = 0;
    if (base + 16 <= np) {
        const uint4 v = *(const uint4*)(flags + base);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 16; ++j) bits |= (uint32_t)(((w[j >> 2] >> ((j & 3) * 8)) & 0xff) != 0) << j;
    } else {
#pragma unroll
        for (int j = 0; j < 16; ++j) bits |= (uint32_t)(base + j < np && flags[base + j] != 0) << j;
    }
    return bits;
}

__global__ __launch_bounds__(256) void compact_count_kernel(const uint8_t* __restrict__ flags, int64_t np, int64_t nseg, int* __restrict__ segcnt) {
    const int lane = threadIdx.x & 63;
    for (int64_t seg = (int64_t)blockIdx.x * 4 + wave_index(); seg < nseg; seg += (int64_t)gridDim.x * 4) {
        int a = __popc(lane_flags(flags, np, seg, lane));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
        if (lane == 0) segcnt[seg] = a;
    }
}

// exclusive scan of the segment counts: one workgroup, 1024 segments (2^20 items) per round, the carry in registers
__global__ __launch_bounds__(1024) void compact_scan_kernel(const int* __restrict__ segcnt, int64_t nseg, int* __restrict__ segoff, int* __restrict__ totals,
                                                            int* __restrict__ index, int64_t np) {
    __shared__ int s_waves[16];
    const int tid = threadIdx.x;
    int carry = 0;
    for (int64_t base = 0; base < nseg; base += 1024) {
        const int64_t i = base + tid;
        const int a = i < nseg ? segcnt[i] : 0;
        int round;
        const int before = block_exclusive_scan<1024>(a, s_waves, &round);
        if (i < nseg) segoff[i] = carry + before;
        carry += round;
    }
    if (tid == 0) {
        totals[0] = carry;                 // the number of flagged items
        index[carry] = (int)np;            // one entry behind the list: the end of the last item
    }
}

__global__ __launch_bounds__(256) void compact_place_kernel(const uint8_t* __restrict__ flags, int64_t np, int64_t nseg, const int* __restrict__ segoff,
                                                            int* __restrict__ index) {
    const int lane = threadIdx.x & 63;
    for (int64_t seg = (int64_t)blockIdx.x * 4 + wave_index(); seg < nseg; seg += (int64_t)gridDim.x * 4) {
        const uint32_t bits = lane_flags(flags, np, seg, lane);
        const int n = __popc(bits);
        int at = segoff[seg] + wave_inclusive_scan(n) - n;
        const int64_t base = seg * kSeg + lane * 16;
#pragma unroll
        for (int j = 0; j < 16; ++j)
            if ((bits >> j) & 1) index[at++] = (int)(base + j);
    }
}

// segments of n items: the length of segcnt[] and of segoff[]
inline int64_t compact_segments(int64_t n) { return (n + kSeg - 1) / kSeg; }

// index[0 .. k) = the items i of [0, n) with flags[i] != 0, ascending; index[k] = n; totals[0] = k.  flags is 16-byte aligned;
// index holds n + 1 entries, segcnt and segoff compact_segments(n) each.
inline void launch_compact(const uint8_t* flags, int64_t n, int32_t* index, int32_t* segcnt, int32_t* segoff, int32_t* totals, hipStream_t st) {
    const int64_t nseg = compact_segments(n);
    const int grid = grid_for((nseg + 3) / 4, 1 << 16);
    hipLaunchKernelGGL(compact_count_kernel, dim3(grid), dim3(256), 0, st, flags, n, nseg, segcnt);
    hipLaunchKernelGGL(compact_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)segcnt, nseg, segoff, totals, index, n);
    hipLaunchKernelGGL(compact_place_kernel, dim3(grid), dim3(256), 0, st, flags, n, nseg, (const int*)segoff, index);
}

}  // namespace

}  // namespace zett
