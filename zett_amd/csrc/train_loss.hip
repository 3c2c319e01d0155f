// train_loss.hip — the language-model loss of the reference's train_step / eval_step over predicted output embeddings
// (train.py:1039-1056, 874-912, 1226-1255), between the library's GEMMs:
//
//     logits = hidden . pred_out^T + addend            zett_op_gemm_lo / zett_op_gemm_f32, the addend through the bias epilogue
//     loss   = sum_t w_t (lse_t - logits[t, label_t]) / sum_t w_t
//
// What is here is the row kernel between the contractions and the small kernels around it: the softmax cross-entropy rows pass
// (statistics per row and, when gradients are wanted, the gradient operand G = w (softmax - onehot) in the operand type of the
// training GEMMs), the finalise, a column sum of G for the bias gradient, the scale by upstream / sum(w) and the operand cast.
//
// The rows pass is memory-bound: a workgroup of 1024 lanes per row, 16 bytes per lane and load.  A row of up to 32 768 columns is
// read ONCE and stays in registers (up to 8 float4 per lane: 16 would spill under the 128 registers of a 1024-lane workgroup) between the statistics and the store of G; a longer row is read
// twice.  Both paths run the same arithmetic in the same order — per lane an online (max, sum of exp, first argmax) over the
// lane's vectors in column order, then a fixed combination tree — so they give the same bits.  No float atomics anywhere: the
// same inputs give the same bits on every run.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "train_common.hip.h"

using namespace zett;

namespace {

constexpr int kBlock = 1024;                  // lanes of a rows-pass workgroup
constexpr int kWaves = kBlock / 64;
constexpr int kOnceMaxVec = 8;                // float4 per lane the read-once path keeps: 8 * 1024 * 4 = ZETT_CE_ONCE_MAX_COLS columns
constexpr int kMaxGrid = 2048;
constexpr float kMaskFill = -100000.f;        // NEGATIVE_INF_FILL_VALUE, zett/utils.py:23
static_assert(kOnceMaxVec * kBlock * 4 == ZETT_CE_ONCE_MAX_COLS, "header and kernel disagree on the read-once limit");

// ---- the running statistics of a softmax row ---------------------------------------------------------------------------------
struct RowStat {
    float m;      // maximum so far (kLowest: nothing seen)
    float s;      // sum of exp(z - m)
    int idx;      // column of the FIRST maximum (jnp.argmax)
};
constexpr float kLowest = -3.4028234664e38f;      // a finite "nothing seen": exp(kLowest - m) and exp(-inf - kLowest) are 0, never NaN

__device__ __forceinline__ float rescale(float s, float m, float M) { return m == M ? s : s * __expf(m - M); }

__device__ __forceinline__ RowStat combine(const RowStat a, const RowStat b) {
#pragma clang fp contract(off)
    RowStat r;
    r.m = fmaxf(a.m, b.m);
    r.idx = a.m > b.m ? a.idx : (b.m > a.m ? b.idx : min(a.idx, b.idx));
    r.s = rescale(a.s, a.m, r.m) + rescale(b.s, b.m, r.m);
    return r;
}

// The four columns c .. c+3 of a row; columns at or beyond v do not exist (a vector that lies wholly beyond v changes nothing).
// Straight-line code: the vectors of a lane were all requested before the first is absorbed, and a branch around a use would make
// the compiler wait for EVERY outstanding memory operation there (loads and stores share one counter).
__device__ __forceinline__ void absorb(RowStat& r, float4 z, int c, int v) {
    const float ninf = -INFINITY;
    z.x = c < v ? z.x : ninf;
    z.y = c + 1 < v ? z.y : ninf;
    z.z = c + 2 < v ? z.z : ninf;
    z.w = c + 3 < v ? z.w : ninf;
    const float m4 = fmaxf(fmaxf(z.x, z.y), fmaxf(z.z, z.w));
    const bool up = m4 > r.m;
    const float m = up ? m4 : r.m;
    r.s = r.s * __expf(r.m - m);                      // (not up: exp(0) = 1 exactly)
    r.idx = up ? (z.x == m4 ? c : (z.y == m4 ? c + 1 : (z.z == m4 ? c + 2 : c + 3))) : r.idx;
    r.m = m;
    r.s += (__expf(z.x - m) + __expf(z.y - m)) + (__expf(z.z - m) + __expf(z.w - m));
}

// all lanes of the workgroup end with the statistics of the whole row (the same bits in every lane: combine is commutative)
__device__ __forceinline__ RowStat block_combine(RowStat r, float* sm, float* ss, int* si) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        RowStat o;
        o.m = __shfl_xor(r.m, off, 64);
        o.s = __shfl_xor(r.s, off, 64);
        o.idx = __shfl_xor(r.idx, off, 64);
        r = combine(r, o);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[wave] = r.m; ss[wave] = r.s; si[wave] = r.idx; }
    __syncthreads();
    const int e = threadIdx.x & (kWaves - 1);          // the sixteen wave results, one per lane of each group of sixteen: a second butterfly
    RowStat t{sm[e], ss[e], si[e]};
#pragma unroll
    for (int off = kWaves / 2; off > 0; off >>= 1) {
        RowStat o;
        o.m = __shfl_xor(t.m, off, 64);
        o.s = __shfl_xor(t.s, off, 64);
        o.idx = __shfl_xor(t.idx, off, 64);
        t = combine(t, o);
    }
    return t;
}

// G[c .. c+3] = w (exp(z - lse) - [c == label]); zero at columns at or beyond v and in a row of weight 0
__device__ __forceinline__ float4 grad4(float4 z, int c, int v, float lse, float w, int label) {
#pragma clang fp contract(off)
    const bool live = w != 0.f;
    float4 g;
    g.x = live && c < v ? w * (__expf(z.x - lse) - (c == label ? 1.f : 0.f)) : 0.f;
    g.y = live && c + 1 < v ? w * (__expf(z.y - lse) - (c + 1 == label ? 1.f : 0.f)) : 0.f;
    g.z = live && c + 2 < v ? w * (__expf(z.z - lse) - (c + 2 == label ? 1.f : 0.f)) : 0.f;
    g.w = live && c + 3 < v ? w * (__expf(z.w - lse) - (c + 3 == label ? 1.f : 0.f)) : 0.f;
    return g;
}

// One workgroup per row.  NV > 0: the read-once path, NV float4 per lane kept in registers (v_padded <= NV * 4096);
// NV == 0: the two-read path.  GT: zett_dtype of G, -1: no gradient operand is written.
// A lane whose vector index lies beyond the row loads the row's last vector instead (no branch around a load) and ignores it.
// G may be the logits themselves (fp32): a lane stores only vectors it has loaded itself, after its last use of them.
template <int NV, int GT>
__global__ __launch_bounds__(kBlock) void ce_rows_kernel(float* logits, int64_t ld_z, const int32_t* __restrict__ labels, const float* __restrict__ weight,
                                                         int64_t rows, int v, int v_padded, void* gout, int64_t ld_g, float* __restrict__ row_loss,
                                                         float* __restrict__ lse_out, int32_t* __restrict__ argmax_out) {
    constexpr int GD = GT < 0 ? ZETT_F32 : GT;
    constexpr int kUnroll = 4;                         // vectors per lane in flight in the loops of the two-read path
    using G = elem_t<GD>;
    __shared__ float sm[kWaves], ss[kWaves];
    __shared__ int si[kWaves];
    const int tid = threadIdx.x;
    const int nvec = v_padded >> 2;
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x) {
        const float* z = logits + r * ld_z;
        const int label = labels[r];
        const float w = weight ? weight[r] : 1.f;
        const bool hit = label >= 0 && label < v;          // anything else is an all-zero one-hot (jax.nn.one_hot); never an index
        float zl = 0.f;
        if (tid == 0 && hit) zl = z[label];
        RowStat st{kLowest, 0.f, 0x7fffffff};
        float4 keep[NV > 0 ? NV : 1];
        if (NV > 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) keep[i] = *(const float4*)(z + 4 * min(i * kBlock + tid, nvec - 1));
#pragma unroll
            for (int i = 0; i < NV; ++i) absorb(st, keep[i], 4 * (i * kBlock + tid), v);
        } else {
            for (int q0 = tid; 4 * q0 < v; q0 += kUnroll * kBlock) {
                float4 zz[kUnroll];
#pragma unroll
                for (int j = 0; j < kUnroll; ++j) zz[j] = *(const float4*)(z + 4 * min(q0 + j * kBlock, nvec - 1));
#pragma unroll
                for (int j = 0; j < kUnroll; ++j) absorb(st, zz[j], 4 * (q0 + j * kBlock), v);
            }
        }
        st = block_combine(st, sm, ss, si);
        const float lse = st.m + logf(st.s);
        if (tid == 0) {
            lse_out[r] = lse;
            argmax_out[r] = st.idx;
            row_loss[r] = w == 0.f ? 0.f : w * (lse - zl);
        }
        if (GT >= 0) {
            G* g = (G*)gout + r * ld_g;
            if (NV > 0) {
                float4 o[NV > 0 ? NV : 1];
#pragma unroll
                for (int i = 0; i < NV; ++i) o[i] = grad4(keep[i], 4 * (i * kBlock + tid), v, lse, w, label);
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int q = i * kBlock + tid;
                    if (q < nvec) store4(g + 4 * q, o[i]);
                }
            } else {
                for (int q0 = tid; q0 < nvec; q0 += kUnroll * kBlock) {
                    float4 zz[kUnroll];
#pragma unroll
                    for (int j = 0; j < kUnroll; ++j) zz[j] = *(const float4*)(z + 4 * min(q0 + j * kBlock, nvec - 1));
#pragma unroll
                    for (int j = 0; j < kUnroll; ++j) zz[j] = grad4(zz[j], 4 * (q0 + j * kBlock), v, lse, w, label);
#pragma unroll
                    for (int j = 0; j < kUnroll; ++j) {
                        const int q = q0 + j * kBlock;
                        if (q < nvec) store4(g + 4 * q, zz[j]);
                    }
                }
            }
        }
        __syncthreads();          // the next row reuses the LDS words
    }
}

// record = { loss, sum w, 1 / sum w, int32 n_correct, int32 n_counted, 0, 0, 0 }: one workgroup, double sums in a fixed order
__global__ __launch_bounds__(256) void ce_finalize_kernel(const float* __restrict__ row_loss, const float* __restrict__ weight, const int32_t* __restrict__ labels,
                                                          const int32_t* __restrict__ argmax, int64_t n, float* __restrict__ record) {
    __shared__ double red[256];
    double sl = 0.0, sw = 0.0, nc = 0.0, nn = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const float w = weight ? weight[i] : 1.f;
        sl += (double)row_loss[i];
        sw += (double)w;
        if (w > 0.f) {
            nn += 1.0;
            if (argmax[i] == labels[i]) nc += 1.0;
        }
    }
    sl = block_sum_f64(sl, red);
    sw = block_sum_f64(sw, red);
    nc = block_sum_f64(nc, red);
    nn = block_sum_f64(nn, red);
    if (threadIdx.x == 0) {
        const bool empty = sw == 0.0;          // the reference divides 0 by 0 here; this loss and every gradient are 0
        record[0] = empty ? 0.f : (float)(sl / sw);
        record[1] = (float)sw;
        record[2] = empty ? 0.f : (float)(1.0 / sw);
        ((int32_t*)record)[3] = (int32_t)nc;
        ((int32_t*)record)[4] = (int32_t)nn;
        record[5] = record[6] = record[7] = 0.f;
    }
}

// out[c] = (vocab_mask ? (vocab_mask[c] ? 0 : -100000) : 0) + bias[c] + priors[c], 0 for v <= c < v_padded
__global__ __launch_bounds__(256) void ce_addend_kernel(const float* __restrict__ bias, const float* __restrict__ priors, const uint8_t* __restrict__ vocab_mask, int v,
                                                        int v_padded, float* __restrict__ out) {
#pragma clang fp contract(off)
    for (int c = blockIdx.x * 256 + threadIdx.x; c < v_padded; c += gridDim.x * 256) {
        float a = 0.f;
        if (c < v) {
            if (vocab_mask) a = vocab_mask[c] ? 0.f : kMaskFill;
            if (bias) a += bias[c];
            if (priors) a += priors[c];
        }
        out[c] = a;
    }
}

// out[c] (+)= sum_r g[r, c]: a workgroup takes 64 columns, its four waves every fourth row; the four partial sums are added in a fixed order
// (the column sum of zett_op_colsum_f32 too: launch_colsum)
template <typename G>
__global__ __launch_bounds__(256) void colsum_kernel(const G* __restrict__ g, int64_t ld_g, int64_t rows, int v, float* __restrict__ out, int accumulate) {
    __shared__ float part[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    float s = 0.f;
    if (c < v)
        for (int64_t r = wave; r < rows; r += 4) s += load1(g + r * ld_g + c);
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c < v) {
        const float t = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        out[c] = accumulate ? out[c] + t : t;
    }
}

// out[i] = in[i] * (upstream[0] * record[2]), written as O
template <typename O>
__global__ __launch_bounds__(256) void ce_scale_kernel(const float* __restrict__ in, int64_t n, const float* __restrict__ record, const float* __restrict__ upstream,
                                                       O* __restrict__ o, int vec_ok) {
    const float f = upstream[0] * record[2];
    const int64_t stride = (int64_t)gridDim.x * 256, t0 = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t tail = 0;
    if (vec_ok) {
        tail = n & ~(int64_t)3;
        for (int64_t i = t0 * 4; i < tail; i += stride * 4) {
            const float4 x = *(const float4*)(in + i);
            store4(o + i, make_float4(x.x * f, x.y * f, x.z * f, x.w * f));
        }
    }
    for (int64_t i = tail + t0; i < n; i += stride) store1(o + i, in[i] * f);
}

// out[r, c] = (O) in[r, c] for c < cols, 0 for cols <= c < cols_padded: every pair of types goes through float
// (the general path of zett_op_convert_lo too: launch_cast)
template <typename I, typename O>
__global__ __launch_bounds__(256) void cast_kernel(const I* __restrict__ in, int64_t ld_in, O* __restrict__ out, int64_t ld_out, int64_t rows, int cols, int cols_padded) {
    const int64_t total = rows * cols_padded;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
        const int64_t r = i / cols_padded;
        const int c = (int)(i - r * cols_padded);
        store1(out + r * ld_out + c, c < cols ? load1(in + r * ld_in + c) : 0.f);
    }
}

template <int NV>
void rows_go(int gt, int grid, hipStream_t st, float* logits, int64_t ld_z, const int32_t* labels, const float* weight, int64_t rows, int v, int v_padded, void* g,
             int64_t ld_g, float* row_loss, float* lse, int32_t* argmax) {
    const auto go = [&](auto dt) {
        hipLaunchKernelGGL((ce_rows_kernel<NV, decltype(dt)::value>), dim3(grid), dim3(kBlock), 0, st, logits, ld_z, labels, weight, rows, v, v_padded, g, ld_g, row_loss, lse, argmax);
    };
    if (!g) go(std::integral_constant<int, -1>{});
    else with_dtype(gt, go);
}

}  // namespace

void zett::launch_colsum(int32_t dtype, const void* in, int64_t ld, int64_t rows, int cols, float* out, int accumulate, hipStream_t st) {
    with_dtype(dtype, [&](auto dt) {
        using G = elem_t<decltype(dt)::value>;
        hipLaunchKernelGGL(colsum_kernel<G>, dim3((cols + 63) / 64), dim3(256), 0, st, (const G*)in, ld, rows, cols, out, accumulate);
    });
}

void zett::launch_cast(int32_t in_dtype, int32_t out_dtype, const void* in, int64_t ld_in, void* out, int64_t ld_out, int64_t rows, int cols, int cols_padded, hipStream_t st) {
    const int grid = (int)std::min<int64_t>((rows * cols_padded + 255) / 256, kMaxGrid * 4);
    with_dtype(in_dtype, [&](auto it) {
        with_dtype(out_dtype, [&](auto ot) {
            using I = elem_t<decltype(it)::value>;
            using O = elem_t<decltype(ot)::value>;
            hipLaunchKernelGGL((cast_kernel<I, O>), dim3(grid), dim3(256), 0, st, (const I*)in, ld_in, (O*)out, ld_out, rows, cols, cols_padded);
        });
    });
}

extern "C" {

int zett_op_ce_addend(const float* bias, const float* priors, const uint8_t* vocab_mask, int32_t v, int32_t v_padded, float* out, void* stream) {
    if (!out) return fail(ZETT_E_INVALID, "null argument");
    if (v <= 0 || v_padded < v) return fail(ZETT_E_INVALID, "the addend needs 0 < v <= v_padded (v = %d, v_padded = %d)", (int)v, (int)v_padded);
    hipLaunchKernelGGL(ce_addend_kernel, dim3(std::min((v_padded + 255) / 256, kMaxGrid)), dim3(256), 0, (hipStream_t)stream, bias, priors, vocab_mask, v, v_padded, out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_ce_rows(float* logits, int64_t ld_z, const int32_t* labels, const float* weight, int64_t rows, int32_t v, int32_t v_padded, void* g, int32_t g_dtype,
                    int64_t ld_g, float* row_loss, float* lse, int32_t* argmax, int32_t path, void* stream) {
    if (!logits || !labels || !row_loss || !lse || !argmax) return fail(ZETT_E_INVALID, "null argument");
    if (rows < 0 || rows >= (int64_t)0x7fffffff) return fail(ZETT_E_INVALID, "bad row count %lld", (long long)rows);
    if (v <= 0 || v_padded < v || v_padded % 4 || v_padded > (1 << 30)) return fail(ZETT_E_INVALID, "the rows pass needs 0 < v <= v_padded, v_padded a multiple of 4 (v = %d, v_padded = %d)", (int)v, (int)v_padded);
    if (ld_z < v_padded || ld_z % 4 || ((uintptr_t)logits & 15)) return fail(ZETT_E_INVALID, "logits rows must be 16-byte aligned and hold v_padded columns (ld = %lld)", (long long)ld_z);
    if (g) {
        if (!is_dtype(g_dtype)) return fail(ZETT_E_INVALID, "unknown dtype %d of the gradient operand", (int)g_dtype);
        if (ld_g < v_padded || ld_g % 4 || ((uintptr_t)g & (g_dtype == ZETT_F32 ? 15 : 7)))
            return fail(ZETT_E_INVALID, "rows of the gradient operand must be aligned to four elements and hold v_padded columns (ld = %lld)", (long long)ld_g);
        if (g == (void*)logits && (g_dtype != ZETT_F32 || ld_g != ld_z)) return fail(ZETT_E_INVALID, "only an fp32 gradient operand with the logits' leading dimension may overwrite them");
    }
    if (path != ZETT_CE_AUTO && path != ZETT_CE_ONCE && path != ZETT_CE_TWICE) return fail(ZETT_E_INVALID, "unknown rows-pass path %d", (int)path);
    if (path == ZETT_CE_ONCE && v_padded > ZETT_CE_ONCE_MAX_COLS) return fail(ZETT_E_INVALID, "the read-once path holds at most %d columns, v_padded = %d", ZETT_CE_ONCE_MAX_COLS, (int)v_padded);
    if (rows == 0) return 0;
    const bool once = path == ZETT_CE_ONCE || (path == ZETT_CE_AUTO && v_padded <= ZETT_CE_ONCE_MAX_COLS);
    const int grid = (int)std::min<int64_t>(rows, 65536);
    hipStream_t st = (hipStream_t)stream;
    const int per_lane = once ? (v_padded / 4 + kBlock - 1) / kBlock : 0;
    auto go = rows_go<0>;                              // the two-read path
    if (once) {
        if (per_lane <= 1) go = rows_go<1>;
        else if (per_lane <= 2) go = rows_go<2>;
        else if (per_lane <= 4) go = rows_go<4>;
        else go = rows_go<8>;
    }
    go(g_dtype, grid, st, logits, ld_z, labels, weight, rows, v, v_padded, g, ld_g, row_loss, lse, argmax);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_ce_finalize(const float* row_loss, const float* weight, const int32_t* labels, const int32_t* argmax, int64_t n, float* record, void* stream) {
    if (!row_loss || !labels || !argmax || !record) return fail(ZETT_E_INVALID, "null argument");
    if (n <= 0) return fail(ZETT_E_INVALID, "the loss needs at least one row");
    hipLaunchKernelGGL(ce_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, row_loss, weight, labels, argmax, n, record);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_ce_colsum(const void* g, int32_t g_dtype, int64_t ld_g, int64_t rows, int32_t v, float* out, int32_t accumulate, void* stream) {
    if (!g || !out) return fail(ZETT_E_INVALID, "null argument");
    if (!is_dtype(g_dtype)) return fail(ZETT_E_INVALID, "unknown dtype %d of the gradient operand", (int)g_dtype);
    if (v <= 0 || rows < 0 || ld_g < v) return fail(ZETT_E_INVALID, "bad column-sum shape (rows = %lld, v = %d, ld = %lld)", (long long)rows, (int)v, (long long)ld_g);
    launch_colsum(g_dtype, g, ld_g, rows, v, out, accumulate, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_ce_scale(const float* in, int64_t n, const float* record, const float* upstream, void* out, int32_t out_dtype, void* stream) {
    if (!in || !record || !upstream || !out) return fail(ZETT_E_INVALID, "null argument");
    if (!is_dtype(out_dtype)) return fail(ZETT_E_INVALID, "unknown output dtype %d", (int)out_dtype);
    if (n < 0) return fail(ZETT_E_INVALID, "bad element count");
    if (n == 0) return 0;
    const int vec_ok = ((uintptr_t)in & 15) == 0 && ((uintptr_t)out & (out_dtype == ZETT_F32 ? 15 : 7)) == 0;
    const dim3 grid((unsigned)std::min<int64_t>((n + 1023) / 1024, kMaxGrid));
    with_dtype(out_dtype, [&](auto dt) {
        using O = elem_t<decltype(dt)::value>;
        hipLaunchKernelGGL(ce_scale_kernel<O>, grid, dim3(256), 0, (hipStream_t)stream, in, n, record, upstream, (O*)out, vec_ok);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_ce_cast(const void* in, int32_t in_dtype, int64_t ld_in, void* out, int32_t out_dtype, int64_t ld_out, int64_t rows, int32_t cols, int32_t cols_padded,
                    void* stream) {
    if (!in || !out) return fail(ZETT_E_INVALID, "null argument");
    if (!is_dtype(in_dtype) || !is_dtype(out_dtype)) return fail(ZETT_E_INVALID, "unknown dtype (%d -> %d)", (int)in_dtype, (int)out_dtype);
    if (rows < 0 || cols <= 0 || cols_padded < cols || ld_in < cols || ld_out < cols_padded) return fail(ZETT_E_INVALID, "bad cast shape");
    if (rows == 0) return 0;
    launch_cast(in_dtype, out_dtype, in, ld_in, out, ld_out, rows, cols, cols_padded, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
