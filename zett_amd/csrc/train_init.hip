// train_init.hip — fitting a fresh hypernetwork's Rescalers (include/zett_hip.h, "fitting a fresh hypernetwork's Rescalers"):
// per-column count / mean / M2 of a [rows, cols] fp32 / f16 / bf16 matrix in ONE read, and the (w, b) of Rescaler.scale_to from two
// such states (zett/utils.py:165-175, called by Hypernet.init_rescaler, zett/model/__init__.py:348-385).
//
// The pass streams: a work item is (chunk of kChunk rows, vector of W columns), one lane each, consecutive lanes on consecutive
// column vectors, so a wave reads 1 KiB of a row at a time; a lane walks its chunk's rows in ascending order, four rows requested
// before the first is used, with one Welford recurrence per column in registers — in fp64: a running mean stored in fp32 would put
// its rounding, an ulp of the MEAN, into every deviation, which a column of mean 3 and std 0.01 feels in its fourth digit, and the
// pass is bound by memory either way.  The chunk's (mean, M2) go to the workspace and a second kernel — one lane per column — merges
// the chunks in ascending order (Chan).  Which lane holds a column, and whether it reads 16 bytes or one element, does not enter a
// column's arithmetic: the result is a function of the values, `rows` and kChunk alone.  No float atomics, no E[x^2] - E[x]^2.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "train_common.hip.h"

using namespace zett;

namespace {

constexpr int kChunk = ZETT_COL_MOMENTS_CHUNK;
constexpr int kMaxGrid = 1 << 18;
static_assert(kChunk == 256, "a workgroup of 256 lanes fills the table of 1 / k, k = 1 .. kChunk, one entry each");

// part: [chunks][2][cols] doubles — the means of a chunk's columns, then their M2.  x points at (row 0, first column of this launch); c_off
// is that column's index among the call's `cols`.
template <typename T, int W>
__global__ __launch_bounds__(256) void col_moments_chunk_kernel(const T* __restrict__ x, int64_t ld, int64_t rows, int nvec, int64_t chunks, int cols, int c_off,
                                                                double* __restrict__ part) {
    __shared__ double s_inv[kChunk];
    s_inv[threadIdx.x] = 1.0 / (double)(threadIdx.x + 1);          // IEEE division: 1 / k rounded once
    __syncthreads();
    const int64_t items = chunks * nvec;
    for (int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x; item < items; item += (int64_t)gridDim.x * 256) {
        const int64_t chunk = item / nvec;
        const int j = (int)(item - chunk * nvec);
        const int64_t r0 = chunk * kChunk;
        const int n = (int)std::min<int64_t>(kChunk, rows - r0);
        const T* p = x + r0 * ld + (int64_t)j * W;
        double mean[W], m2[W];
#pragma unroll
        for (int i = 0; i < W; ++i) mean[i] = m2[i] = 0.0;
        int k = 0;
        for (; k + 4 <= n; k += 4) {
            Pack<T, W> v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = *(const Pack<T, W>*)(p + (int64_t)(k + u) * ld);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double inv = s_inv[k + u];
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const double xf = (double)lo_to_f32<T>(v[u].v[i]);
                    const double d = xf - mean[i];
                    mean[i] = fma(d, inv, mean[i]);
                    m2[i] = fma(d, xf - mean[i], m2[i]);
                }
            }
        }
        for (; k < n; ++k) {
            const Pack<T, W> v = *(const Pack<T, W>*)(p + (int64_t)k * ld);
            const double inv = s_inv[k];
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const double xf = (double)lo_to_f32<T>(v.v[i]);
                const double d = xf - mean[i];
                mean[i] = fma(d, inv, mean[i]);
                m2[i] = fma(d, xf - mean[i], m2[i]);
            }
        }
        double* o = part + chunk * 2 * (int64_t)cols + c_off + j * W;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            o[i] = mean[i];
            o[cols + i] = m2[i];
        }
    }
}

// One lane per column: the chunks in ascending order onto the empty state or onto what `state` holds.
__global__ __launch_bounds__(256) void col_moments_merge_kernel(const double* __restrict__ part, int64_t chunks, int64_t rows, int cols, double* __restrict__ state,
                                                                int accumulate) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    double n = 0.0, mean = 0.0, m2 = 0.0;
    if (accumulate) {
        n = state[3 * c];
        mean = state[3 * c + 1];
        m2 = state[3 * c + 2];
    }
    const double* pm = part + c;
    const int64_t step = 2 * (int64_t)cols;
    auto rows_of = [&](int64_t j) { return (double)std::min<int64_t>(kChunk, rows - j * kChunk); };
    auto merge = [&](double nb, double mb, double qb) {
        const double tot = n + nb, d = mb - mean, r = nb / tot;
        mean = mean + d * r;
        m2 = m2 + qb + d * d * (n * r);
        n = tot;
    };
    int64_t j = 0;
    if (n == 0.0 && chunks > 0) {          // onto an empty state: the first chunk itself, bit for bit
        n = rows_of(0);
        mean = pm[0];
        m2 = pm[cols];
        j = 1;
    }
    // The partials of eight chunks are requested together, then merged one after the other.  The counts, and with them the weight
    // r of a merge, do not depend on the data: the division is off the chain through `mean`, which is one subtraction and one
    // multiply-add per chunk.  (One wave per SIMD at 8 192 columns: the merge is bound by its own instruction count, mostly the division.)
    for (; j + 8 <= chunks; j += 8) {
        double mb[8], qb[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            mb[u] = pm[(j + u) * step];
            qb[u] = pm[(j + u) * step + cols];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) merge(rows_of(j + u), mb[u], qb[u]);
    }
    for (; j < chunks; ++j) merge(rows_of(j), pm[j * step], pm[j * step + cols]);
    state[3 * c] = n;
    state[3 * c + 1] = mean;
    state[3 * c + 2] = m2;
}

__global__ __launch_bounds__(256) void rescaler_fit_kernel(const double* __restrict__ xs, const double* __restrict__ ts, double t_std, double t_mean, int cols,
                                                           float* __restrict__ w, float* __restrict__ b) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    const double sx = sqrt(fmax(xs[3 * c + 2], 0.0) / xs[3 * c]), mx = xs[3 * c + 1];
    if (ts) {
        t_std = sqrt(fmax(ts[3 * c + 2], 0.0) / ts[3 * c]);
        t_mean = ts[3 * c + 1];
    }
    const double ww = t_std / (sx + 1e-8);
    w[c] = (float)ww;
    b[c] = (float)(t_mean - ww * mx);
}

int elem_bytes(int32_t d) { return d == ZETT_F32 ? 4 : 2; }
int64_t chunks_of(int64_t rows) { return (rows + kChunk - 1) / kChunk; }
int64_t workspace_need(int64_t rows, int cols) { return std::max<int64_t>(16, chunks_of(rows) * 2 * (int64_t)cols * 8); }

template <typename T, int W>
void chunk_go(hipStream_t st, const T* x, int64_t ld, int64_t rows, int ncols, int cols, int c_off, double* part) {
    const int nvec = ncols / W;
    if (nvec <= 0) return;
    const int64_t chunks = chunks_of(rows);
    hipLaunchKernelGGL((col_moments_chunk_kernel<T, W>), dim3(grid256(chunks * nvec, kMaxGrid)), dim3(256), 0, st, x + c_off, ld, rows, nvec, chunks, cols, c_off, part);
}

}  // namespace

extern "C" {

int zett_op_col_moments_workspace_bytes(int64_t rows, int32_t cols, int64_t* bytes) {
    if (!bytes || rows < 0 || cols < 1) return fail(ZETT_E_INVALID, "bad column-moments shape (rows = %lld, cols = %d)", (long long)rows, (int)cols);
    *bytes = workspace_need(rows, cols);
    return 0;
}

int zett_op_col_moments(const void* x, int32_t dtype, int64_t ld, int64_t rows, int32_t col0, int32_t cols, void* state, int32_t accumulate, void* workspace,
                        int64_t workspace_bytes, void* stream) {
    if (!is_dtype(dtype)) return fail(ZETT_E_INVALID, "unknown dtype %d", (int)dtype);
    const int es = elem_bytes(dtype);
    if (!state || !workspace || (rows > 0 && !x)) return fail(ZETT_E_INVALID, "null argument");
    if (!aligned(state, 8) || !aligned(workspace, 8) || !aligned(x, es)) return fail(ZETT_E_INVALID, "misaligned x, state or workspace");
    if (rows < 0 || cols < 1 || col0 < 0) return fail(ZETT_E_INVALID, "the moments need rows >= 0, cols >= 1 and col0 >= 0 (rows = %lld, cols = %d, col0 = %d)", (long long)rows, (int)cols, (int)col0);
    if ((int64_t)col0 + cols > ld) return fail(ZETT_E_INVALID, "columns [%d, %lld) do not fit the leading dimension %lld", (int)col0, (long long)col0 + cols, (long long)ld);
    if (workspace_bytes < workspace_need(rows, cols))
        return fail(ZETT_E_INVALID, "the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes, (long long)workspace_need(rows, cols));
    if (rows == 0 && accumulate) return 0;
    hipStream_t st = (hipStream_t)stream;
    double* part = (double*)workspace;
    if (rows > 0) {
        // columns in front of the first 16-byte aligned one (element reads), whole vectors of 16 bytes, the rest (element reads);
        // no aligned column, or rows that do not keep the alignment: element reads for all
        const int w = 16 / es;
        const uintptr_t at = (uintptr_t)x + (uintptr_t)col0 * es;
        int head = cols, body = 0;
        if ((ld * es) % 16 == 0) {
            head = (int)std::min<int64_t>(cols, (int64_t)((16 - at % 16) % 16) / es);
            body = (cols - head) / w * w;
        }
        with_dtype(dtype, [&](auto dt) {
            using T = elem_t<decltype(dt)::value>;
            constexpr int W = 16 / (int)sizeof(T);
            const T* x0 = (const T*)x + col0;
            chunk_go<T, 1>(st, x0, ld, rows, head, cols, 0, part);
            chunk_go<T, W>(st, x0, ld, rows, body, cols, head, part);
            chunk_go<T, 1>(st, x0, ld, rows, cols - head - body, cols, head + body, part);
        });
    }
    hipLaunchKernelGGL(col_moments_merge_kernel, dim3(grid256(cols, kMaxGrid)), dim3(256), 0, st, (const double*)part, chunks_of(rows), rows, (int)cols, (double*)state,
                       accumulate ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_rescaler_fit(const void* x_state, int32_t cols, const void* target_state, double target_std, double target_mean, float* w, float* b, void* stream) {
    if (!x_state || !w || !b) return fail(ZETT_E_INVALID, "null argument");
    if (cols < 1) return fail(ZETT_E_INVALID, "the fit needs cols >= 1 (cols = %d)", (int)cols);
    if (!aligned(x_state, 8) || !aligned(target_state, 8) || !aligned(w, 4) || !aligned(b, 4)) return fail(ZETT_E_INVALID, "misaligned state, w or b");
    hipStream_t st = (hipStream_t)stream;
    double count[2] = {1.0, 1.0};          // every column of a state holds the same count: the first is read back
    HIP_TRY(hipMemcpyAsync(&count[0], x_state, sizeof(double), hipMemcpyDeviceToHost, st));
    if (target_state) HIP_TRY(hipMemcpyAsync(&count[1], target_state, sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!(count[0] >= 1.0) || !(count[1] >= 1.0))
        return fail(ZETT_E_INVALID, "a state of count 0 has no mean and no std (x: %.0f rows%s)", count[0], target_state ? (count[1] >= 1.0 ? "" : ", target: 0 rows") : "");
    hipLaunchKernelGGL(rescaler_fit_kernel, dim3(grid256(cols, kMaxGrid)), dim3(256), 0, st, (const double*)x_state, (const double*)target_state, target_std, target_mean, (int)cols, w,
                       b);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
