// train_adafactor.hip — the second branch of the reference's optimizer (train.py:631-656): optax.chain(clip_by_global_norm,
// multi_transform({train: adafactor, freeze: set_to_zero})) with optax.adafactor's defaults (factored second moments for matrices whose
// smaller dimension is >= 128, decay 1 - t^-0.8, block-RMS clip at 1, parameter scale, no momentum) as one host call that launches six
// multi-tensor kernels.  DESIGN.md §7a′ has the derivation and the bytes each pass moves.
//
// Work items.  A tensor spans many work items, a work item never spans tensors:
//   * a FACTORED tensor [R, C] (not frozen, min(R, C) >= 128) is cut into tiles of kTileRows x kTileCols = 64 x 256 elements; tile
//     (tr, tc) is item tr * nTC + tc of the tensor.  Wave w of the workgroup owns rows 16 w .. 16 w + 15 of the tile, lane l owns columns
//     4 l .. 4 l + 3: one 16-byte access per lane and row where the pointer and C allow it, four 4-byte accesses of the same elements
//     otherwise — both forms add in the same order, so alignment never changes a bit of the result;
//   * every other tensor (1-D, a matrix with a dimension below 128, a frozen one) is flat: chunks of ZETT_MT_CHUNK elements, summed
//     and cleared by the helpers train_step.hip's sumsq_kernel / adamw_kernel use (train_optim.hip.h).
//
// Sums (fp32 unless said otherwise, no atomics; depth = the longest chain of additions behind one result):
//   tile row sum of g^2      (x0 + x1) + (x2 + x3) per lane, wave_sum                                          depth 8, 256 terms
//   tile column sum of g^2   per lane its wave's 16 rows top to bottom, the four waves (w0 + w1) + (w2 + w3)    depth 18, 64 terms
//   tile sum of g^2          block_sum_pairwise of the 256 column sums                                         depth 26
//   tile sum of p^2, of u^2  per lane four column sums over 16 rows, (a0 + a1) + (a2 + a3), block_sum_pairwise  depth 26
//   chunk sums               chunk_sum's order                                                                 depth 74 (16-byte aligned) / 266
//   segment sum of v_row     block_sum_pairwise of 256 consecutive new v_row values                            depth 8
//   every second stage       (tile partials of a row or column, items of a tensor, segments of v_row, all items of the list) in
//                            float64 in index order (a thread's strided terms, then block_sum_f64's tree), rounded to fp32 once.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/zett_hip.h"
#include "train_optim.hip.h"      // (and through it train_common.hip.h, common.hip.h)

using namespace zett;

namespace {

constexpr int kGroup = ZETT_ADAFACTOR_GROUP;    // tensors per launch: the lists travel as kernel arguments (< 4 KB)
constexpr int kTileRows = ZETT_ADAFACTOR_TILE_ROWS, kTileCols = ZETT_ADAFACTOR_TILE_COLS, kSeg = 256;
constexpr int kMinFactor = 128;                 // optax.adafactor min_dim_size_to_factor
constexpr float kEpsScale = 1e-3f;              // eps_scale of optax.scale_by_param_block_rms
constexpr double kEps = 1e-30;                  // eps of optax.scale_by_factored_rms
static_assert(kTileRows == 64 && kTileCols == 256, "the tile is four waves of sixteen rows, four columns per lane");

enum : uint8_t { kFactored = 4, kNormRows = 8 };      // beside ZETT_ADAMW_DECAY | ZETT_ADAMW_FROZEN in AfList::flags

// One launch group.  va / vb: a factored tensor's statistics by geometry — va[R] the mean of q over each row, vb[C] over each column
// (kNormRows: va is optax's v_row, the one divided by its mean; else vb is); a flat tensor's full-size v is va.
struct AfList {
    float* p[kGroup];
    float* g[kGroup];
    float* va[kGroup];
    float* vb[kGroup];
    int64_t n[kGroup];
    int64_t ws[kGroup];                // factored: float offset of rowpart [nTC, R] | colpart [nTR, C] | vpart [segments] in the workspace
    int32_t rows[kGroup], cols[kGroup];
    int32_t item_start[kGroup + 1];    // first work item of the tensor in this launch
    int32_t seg_start[kGroup + 1];     // first statistics segment (256 entries of va, then of vb) of the tensor in this launch
    uint8_t flags[kGroup];
    int32_t n_tensors;
    int32_t tensor_base;               // tensors (with elements) of the launches before this one
    int64_t item_base;                 // work items of the launches before this one
};
struct AfWs {                          // float offsets into the workspace
    int64_t gpart, ppart, upart;       // one float per work item of the list
    int64_t ts;                        // four floats per tensor: mean(v_row), s, lr s / max(1, RMS(u)), RMS(u)
};
struct AfHyper {
    double lr, max_norm;
    float wd;
    int32_t zero_grad;
};
static_assert(sizeof(AfList) + sizeof(AfWs) + sizeof(AfHyper) + 16 < 4096, "tensor lists must fit the kernel-argument limit");

__device__ __forceinline__ int tiles_across(int cols) { return (cols + kTileCols - 1) / kTileCols; }

// elements c .. c + 3 of a row of `cols` elements, zeros past its end
__device__ __forceinline__ float4 load_row4(const float* __restrict__ row, int c, int cols, bool vec) {
    if (vec) return c < cols ? *(const float4*)(row + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 x;
    x.x = c < cols ? row[c] : 0.f;
    x.y = c + 1 < cols ? row[c + 1] : 0.f;
    x.z = c + 2 < cols ? row[c + 2] : 0.f;
    x.w = c + 3 < cols ? row[c + 3] : 0.f;
    return x;
}
__device__ __forceinline__ void store_row4(float* __restrict__ row, int c, int cols, bool vec, float4 x) {
    if (vec) {
        if (c < cols) *(float4*)(row + c) = x;
        return;
    }
    if (c < cols) row[c] = x.x;
    if (c + 1 < cols) row[c + 1] = x.y;
    if (c + 2 < cols) row[c + 2] = x.z;
    if (c + 3 < cols) row[c + 3] = x.w;
}
__device__ __forceinline__ bool tile_vec(const float* a, const float* b, int cols) {
    return ((((uintptr_t)a | (uintptr_t)b) & 15) == 0) && (cols & 3) == 0;
}

// ---- pass 1: one read of g and p ---------------------------------------------------------------------------------------------------
// gpart[item] = sum g^2, ppart[item] = sum p^2 (0 for a frozen tensor: its p is not read); a tile also leaves its 64 row sums and 256
// column sums of g^2 in rowpart [tc, r] and colpart [tr, c].
__global__ __launch_bounds__(256) void af_pass1_kernel(const AfList a, const AfWs w, float* __restrict__ ws) {
    __shared__ float cs[4][kTileCols];
    __shared__ float red[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = a.item_start[a.n_tensors];
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int t = tensor_of(a.item_start, a.n_tensors, item);
        const int local = item - a.item_start[t];
        const int flags = a.flags[t];
        float sg, sp = 0.f;
        if (flags & kFactored) {
            const int R = a.rows[t], C = a.cols[t], ntc = tiles_across(C);
            const int tr = local / ntc, tc = local - tr * ntc;
            const float* g = a.g[t];
            const float* p = a.p[t];
            const bool vec = tile_vec(g, p, C);
            float* rowpart = ws + a.ws[t];
            float* colpart = rowpart + (int64_t)ntc * R;
            const int c = tc * kTileCols + lane * 4;
            float4 cg = make_float4(0.f, 0.f, 0.f, 0.f), cp = cg;
            for (int k = 0; k < 16; ++k) {
                const int r = tr * kTileRows + wave * 16 + k;
                if (r >= R) break;                                   // (the same for the whole wave)
                const float4 x = load_row4(g + (int64_t)r * C, c, C, vec), y = load_row4(p + (int64_t)r * C, c, C, vec);
                const float4 q = make_float4(x.x * x.x, x.y * x.y, x.z * x.z, x.w * x.w);
                const float rs = wave_sum((q.x + q.y) + (q.z + q.w));
                if (lane == 0) rowpart[(int64_t)tc * R + r] = rs;
                cg.x += q.x; cg.y += q.y; cg.z += q.z; cg.w += q.w;
                cp.x += y.x * y.x; cp.y += y.y * y.y; cp.z += y.z * y.z; cp.w += y.w * y.w;
            }
            __syncthreads();                                         // (cs of the previous item has been read)
            *(float4*)&cs[wave][lane * 4] = cg;
            __syncthreads();
            const int j = threadIdx.x, col = tc * kTileCols + j;
            const float colsum = (cs[0][j] + cs[1][j]) + (cs[2][j] + cs[3][j]);
            if (col < C) colpart[(int64_t)tr * C + col] = colsum;
            sg = block_sum_pairwise(colsum, red);
            sp = block_sum_pairwise((cp.x + cp.y) + (cp.z + cp.w), red);
        } else {
            const int64_t off = (int64_t)local * kChunk;
            const int len = (int)std::min<int64_t>(kChunk, a.n[t] - off);
            sg = chunk_sumsq(a.g[t] + off, len, red);
            if (!(flags & ZETT_ADAMW_FROZEN)) sp = chunk_sumsq(a.p[t] + off, len, red);
        }
        if (threadIdx.x == 0) {
            ws[w.gpart + a.item_base + item] = sg;
            ws[w.ppart + a.item_base + item] = sp;
        }
    }
}

// record = { norm, coef, skip (int32), count (int32), beta, 1 - beta, 0, 0 }: norm_words; the count t before this step is the number
// of updates applied so far and beta = 1 - (t + 1)^-0.8 (optax.scale_by_factored_rms: decay_rate 0.8, step t + 1), the power taken in
// float64 and rounded to fp32 once (word 5), beta = (float)(1 - power).
__global__ __launch_bounds__(256) void af_norm_kernel(const float* __restrict__ gpart, int64_t total, double max_norm, float* __restrict__ record) {
    __shared__ double red[256];
    const double s = strided_sum_f64(gpart, total, red);
    if (threadIdx.x == 0) {
        const double pw = pow((double)norm_words(s, max_norm, record).before + 1.0, -0.8);
        record[4] = (float)(1.0 - pw);
        record[5] = (float)pw;
        record[6] = record[7] = 0.f;
    }
}

// the new v_row / v_col of the factored tensors, one 256-entry segment per work item: v = beta v + (1 - beta) (coef^2 sum / count + 1e-30)
// with the tile partials of the entry summed in float64 in tile order; the segments of optax's v_row also leave their sum in vpart.
__global__ __launch_bounds__(256) void af_stats_kernel(const AfList a, float* __restrict__ ws, const float* __restrict__ record) {
    __shared__ float red[4];
    if (((const int32_t*)record)[2] != 0) return;
    const double coef = (double)record[1], c2 = coef * coef;
    const float beta = record[4], omb = record[5];
    const int total = a.seg_start[a.n_tensors];
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int t = tensor_of(a.seg_start, a.n_tensors, item);
        const int R = a.rows[t], C = a.cols[t], ntc = tiles_across(C), ntr = (R + kTileRows - 1) / kTileRows;
        const int segs_a = (R + kSeg - 1) / kSeg;
        int seg = item - a.seg_start[t];
        const bool side_b = seg >= segs_a;
        if (side_b) seg -= segs_a;
        const float* rowpart = ws + a.ws[t];
        const float* colpart = rowpart + (int64_t)ntc * R;
        float* vpart = ws + a.ws[t] + (int64_t)ntc * R + (int64_t)ntr * C;
        const float* part = side_b ? colpart : rowpart;
        const int len = side_b ? C : R, parts = side_b ? ntr : ntc, count = side_b ? R : C;
        float* v = side_b ? a.vb[t] : a.va[t];
        const int i = seg * kSeg + threadIdx.x;
        float vn = 0.f;
        if (i < len) {
            double s = 0.0;
#pragma unroll 8                                                     // (as in strided_sum_f64: loads in flight, the same order)
            for (int k = 0; k < parts; ++k) s += (double)part[(int64_t)k * len + i];
            const float mq = (float)(c2 * s / (double)count + kEps);
            vn = beta * v[i] + omb * mq;
            v[i] = vn;
        }
        const bool normalised = side_b != (bool)(a.flags[t] & kNormRows);
        if (normalised) {                                            // (the same for the whole workgroup)
            const float s = block_sum_pairwise(vn, red);
            if (threadIdx.x == 0) vpart[seg] = s;
        }
    }
}

// one workgroup per tensor.  stage 0 (before pass 2): ts[0] = mean(v_row), ts[1] = s = max(sqrt(mean p^2), 1e-3).  stage 1 (after it):
// ts[3] = RMS(u), ts[2] = lr s / max(1, RMS(u)).  float64 sums in index order, one rounding each.
__global__ __launch_bounds__(256) void af_tensor_kernel(const AfList a, const AfWs w, const AfHyper h, int stage, float* __restrict__ ws,
                                                        const float* __restrict__ record) {
    __shared__ double red[256];
    if (((const int32_t*)record)[2] != 0) return;
    const int t = blockIdx.x;
    const int flags = a.flags[t];
    if (flags & ZETT_ADAMW_FROZEN) return;
    float* ts = ws + w.ts + 4 * (int64_t)(a.tensor_base + t);
    const int64_t first = a.item_base + a.item_start[t], items = a.item_start[t + 1] - a.item_start[t];
    const float* part = ws + (stage == 0 ? w.ppart : w.upart) + first;
    const double s = strided_sum_f64(part, items, red);
    if (stage == 0) {
        double m = 0.0;
        int len = 1;
        if (flags & kFactored) {
            const int R = a.rows[t], C = a.cols[t], ntc = tiles_across(C), ntr = (R + kTileRows - 1) / kTileRows;
            const float* vpart = ws + a.ws[t] + (int64_t)ntc * R + (int64_t)ntr * C;
            len = (flags & kNormRows) ? R : C;
            const int segs = (len + kSeg - 1) / kSeg;
            for (int i = threadIdx.x; i < segs; i += 256) m += (double)vpart[i];
        }
        m = block_sum_f64(m, red);
        if (threadIdx.x == 0) {
            ts[0] = (float)(m / (double)len);
            ts[1] = fmaxf((float)sqrt(s / (double)a.n[t]), kEpsScale);
        }
    } else if (threadIdx.x == 0) {
        const double rms = sqrt(s / (double)a.n[t]);
        ts[3] = (float)rms;
        ts[2] = (float)(h.lr * (double)ts[1] / fmax(1.0, rms));
    }
}

// What passes 2 and 3 both compute: u of a tile row from g, the row's factor and the lane's four column factors.  first = optax's
// r_factor, (v_row / mean(v_row))^-1/2, second = its c_factor, v_col^-1/2: u = ((coef g) first) second.
struct TileFactors {
    float4 cf;            // of the lane's four columns
    bool rows_first;      // the row factor is optax's r_factor
};
__device__ __forceinline__ float factor(float v) { return 1.f / sqrtf(v); }
__device__ __forceinline__ float u1(float g, float coef, float rf, float cf, bool rows_first) {
    const float gp = g * coef;
    return rows_first ? (gp * rf) * cf : (gp * cf) * rf;
}
__device__ __forceinline__ float4 u4(float4 g, float coef, float rf, const TileFactors& f) {
    return make_float4(u1(g.x, coef, rf, f.cf.x, f.rows_first), u1(g.y, coef, rf, f.cf.y, f.rows_first), u1(g.z, coef, rf, f.cf.z, f.rows_first),
                       u1(g.w, coef, rf, f.cf.w, f.rows_first));
}
// rf[0 .. 64) (LDS) = the factors of the tile's rows, -> the lane's column factors.  Entries past the tensor's edge are 0.
__device__ __forceinline__ TileFactors tile_factors(const AfList& a, int t, int tr, int tc, float mean, float* rf) {
    const int R = a.rows[t], C = a.cols[t];
    TileFactors f;
    f.rows_first = a.flags[t] & kNormRows;
    __syncthreads();                                                 // (rf of the previous item has been read)
    if (threadIdx.x < kTileRows) {
        const int r = tr * kTileRows + threadIdx.x;
        rf[threadIdx.x] = r < R ? factor(f.rows_first ? a.va[t][r] / mean : a.va[t][r]) : 0.f;
    }
    const int c = tc * kTileCols + (threadIdx.x & 63) * 4;
    float x[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) x[k] = c + k < C ? factor(f.rows_first ? a.vb[t][c + k] : a.vb[t][c + k] / mean) : 0.f;
    f.cf = make_float4(x[0], x[1], x[2], x[3]);
    __syncthreads();
    return f;
}

// a flat tensor's v: five IEEE operations, none fused — at t = 0 (beta = 0, 1 - beta = 1) v is q = fl(fl(g'^2) + 1e-30) to the bit
__device__ __forceinline__ float v_new(float v, float g, float coef, float beta, float omb) {
#pragma clang fp contract(off)
    const float gp = g * coef;
    return beta * v + omb * (gp * gp + (float)kEps);
}

// ---- pass 2: upart[item] = sum u^2; the flat tensors' v is updated here ----------------------------------------------------------------
__global__ __launch_bounds__(256) void af_pass2_kernel(const AfList a, const AfWs w, float* __restrict__ ws, const float* __restrict__ record) {
    __shared__ float rf[kTileRows];
    __shared__ float red[4];
    if (((const int32_t*)record)[2] != 0) return;
    const float coef = record[1], beta = record[4], omb = record[5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = a.item_start[a.n_tensors];
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int t = tensor_of(a.item_start, a.n_tensors, item);
        const int local = item - a.item_start[t];
        const int flags = a.flags[t];
        if (flags & ZETT_ADAMW_FROZEN) continue;
        float su;
        if (flags & kFactored) {
            const int R = a.rows[t], C = a.cols[t], ntc = tiles_across(C);
            const int tr = local / ntc, tc = local - tr * ntc;
            const float* g = a.g[t];
            const bool vec = tile_vec(g, a.p[t], C);
            const TileFactors f = tile_factors(a, t, tr, tc, ws[w.ts + 4 * (int64_t)(a.tensor_base + t)], rf);
            const int c = tc * kTileCols + lane * 4;
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int k = 0; k < 16; ++k) {
                const int r = tr * kTileRows + wave * 16 + k;
                if (r >= R) break;
                const float4 u = u4(load_row4(g + (int64_t)r * C, c, C, vec), coef, rf[wave * 16 + k], f);
                acc.x += u.x * u.x; acc.y += u.y * u.y; acc.z += u.z * u.z; acc.w += u.w * u.w;
            }
            su = block_sum_pairwise((acc.x + acc.y) + (acc.z + acc.w), red);
        } else {
            const int64_t off = (int64_t)local * kChunk;
            const int len = (int)std::min<int64_t>(kChunk, a.n[t] - off);
            const float* g = a.g[t] + off;
            float* v = a.va[t] + off;
            auto one = [&](int i) {
                const float vn = v_new(v[i], g[i], coef, beta, omb);
                v[i] = vn;
                const float u = (g[i] * coef) * factor(vn);
                return u * u;
            };
            su = chunk_sum(len, (((uintptr_t)g | (uintptr_t)v) & 15) == 0, red,
                           [&](int i) {
                               const float4 x = *(const float4*)(g + i);
                               float4 vv = *(const float4*)(v + i);
                               vv = make_float4(v_new(vv.x, x.x, coef, beta, omb), v_new(vv.y, x.y, coef, beta, omb), v_new(vv.z, x.z, coef, beta, omb),
                                                v_new(vv.w, x.w, coef, beta, omb));
                               *(float4*)(v + i) = vv;
                               const float4 u = make_float4((x.x * coef) * factor(vv.x), (x.y * coef) * factor(vv.y), (x.z * coef) * factor(vv.z), (x.w * coef) * factor(vv.w));
                               return make_float4(u.x * u.x, u.y * u.y, u.z * u.z, u.w * u.w);
                           },
                           one);
        }
        if (threadIdx.x == 0) ws[w.upart + a.item_base + item] = su;
    }
}

__device__ __forceinline__ float p_new(float p, float u, float scale, float wd) { return p - (scale * u + wd * p); }

// ---- pass 3: p -= scale u + (decay ? wd p : 0); gradients cleared where asked — those of frozen tensors and of a skipped step too ------
__global__ __launch_bounds__(256) void af_pass3_kernel(const AfList a, const AfWs w, const AfHyper h, float* __restrict__ ws, const float* __restrict__ record) {
    __shared__ float rf[kTileRows];
    const bool skip = ((const int32_t*)record)[2] != 0;
    if (skip && !h.zero_grad) return;
    const float coef = record[1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int total = a.item_start[a.n_tensors];
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int item = blockIdx.x; item < total; item += gridDim.x) {
        const int t = tensor_of(a.item_start, a.n_tensors, item);
        const int local = item - a.item_start[t];
        const int flags = a.flags[t];
        const float wd = (flags & ZETT_ADAMW_DECAY) ? h.wd : 0.f;
        const float* ts = ws + w.ts + 4 * (int64_t)(a.tensor_base + t);
        if (flags & kFactored) {
            const int R = a.rows[t], C = a.cols[t], ntc = tiles_across(C);
            const int tr = local / ntc, tc = local - tr * ntc;
            float* g = a.g[t];
            float* p = a.p[t];
            const bool vec = tile_vec(g, p, C);
            const int c = tc * kTileCols + lane * 4;
            if (skip) {
                for (int k = 0; k < 16; ++k) {
                    const int r = tr * kTileRows + wave * 16 + k;
                    if (r < R) store_row4(g + (int64_t)r * C, c, C, vec, zero);
                }
                continue;
            }
            const TileFactors f = tile_factors(a, t, tr, tc, ts[0], rf);
            const float scale = ts[2];
            for (int k = 0; k < 16; ++k) {
                const int r = tr * kTileRows + wave * 16 + k;
                if (r >= R) break;
                const float4 u = u4(load_row4(g + (int64_t)r * C, c, C, vec), coef, rf[wave * 16 + k], f);
                const float4 y = load_row4(p + (int64_t)r * C, c, C, vec);
                store_row4(p + (int64_t)r * C, c, C, vec, make_float4(p_new(y.x, u.x, scale, wd), p_new(y.y, u.y, scale, wd), p_new(y.z, u.z, scale, wd), p_new(y.w, u.w, scale, wd)));
                if (h.zero_grad) store_row4(g + (int64_t)r * C, c, C, vec, zero);
            }
            continue;
        }
        const int64_t off = (int64_t)local * kChunk;
        const int len = (int)std::min<int64_t>(kChunk, a.n[t] - off);
        float* g = a.g[t] + off;
        if (skip || (flags & ZETT_ADAMW_FROZEN)) {
            if (h.zero_grad) zero_chunk(g, len);
            continue;
        }
        float* p = a.p[t] + off;
        const float* v = a.va[t] + off;
        const float scale = ts[2];
        int tail = 0;
        if ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)v) & 15) == 0) {
            tail = len & ~3;
            for (int i = threadIdx.x * 4; i < tail; i += 1024) {
                const float4 x = *(const float4*)(g + i), vv = *(const float4*)(v + i);
                float4 y = *(const float4*)(p + i);
                y = make_float4(p_new(y.x, (x.x * coef) * factor(vv.x), scale, wd), p_new(y.y, (x.y * coef) * factor(vv.y), scale, wd),
                                p_new(y.z, (x.z * coef) * factor(vv.z), scale, wd), p_new(y.w, (x.w * coef) * factor(vv.w), scale, wd));
                *(float4*)(p + i) = y;
                if (h.zero_grad) *(float4*)(g + i) = zero;
            }
        }
        for (int i = tail + threadIdx.x; i < len; i += 256) {
            p[i] = p_new(p[i], (g[i] * coef) * factor(v[i]), scale, wd);
            if (h.zero_grad) g[i] = 0.f;
        }
    }
}

// ---- host: the layout of the list ------------------------------------------------------------------------------------------------------
struct Plan {
    std::vector<AfList> lists;
    std::vector<std::vector<int>> entry;      // per list: the caller's index of each of its tensors
    AfWs ws{};
    int64_t items = 0, floats = 0;
    int32_t tensors = 0;
};

bool is_factored(int64_t rows, int64_t cols, uint8_t flags) { return !(flags & ZETT_ADAMW_FROZEN) && std::min(rows, cols) >= kMinFactor; }

int make_plan(const int64_t* rows, const int64_t* cols, const uint8_t* flags, int32_t n_tensors, Plan* plan) {
    if (n_tensors < 0 || (n_tensors && (!rows || !cols || !flags))) return fail(ZETT_E_INVALID, "null argument");
    Carve carve;      // (in floats here: every array starts on a multiple of 16 floats)
    std::vector<int64_t> region(n_tensors, 0);
    int64_t items = 0, tensors = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (rows[i] < 0 || cols[i] < 0 || rows[i] >= 0x7fffffff || cols[i] >= 0x7fffffff) return fail(ZETT_E_INVALID, "tensor %d: bad shape [%lld, %lld]", i, (long long)rows[i], (long long)cols[i]);
        if (flags[i] & ~(ZETT_ADAMW_DECAY | ZETT_ADAMW_FROZEN)) return fail(ZETT_E_INVALID, "tensor %d: unknown flags %d", i, (int)flags[i]);
        const int64_t n = rows[i] * cols[i];
        if (!n) continue;
        ++tensors;
        if (is_factored(rows[i], cols[i], flags[i])) {
            const int64_t ntr = (rows[i] + kTileRows - 1) / kTileRows, ntc = (cols[i] + kTileCols - 1) / kTileCols;
            items += ntr * ntc;
            region[i] = carve.take(ntc * rows[i] + ntr * cols[i] + (std::min(rows[i], cols[i]) + kSeg - 1) / kSeg);
        } else {
            items += chunk_items(n);
        }
        if (items >= 0x7fffffff) return fail(ZETT_E_INVALID, "too many elements");
    }
    plan->ws.gpart = carve.take(items);
    plan->ws.ppart = carve.take(items);
    plan->ws.upart = carve.take(items);
    plan->ws.ts = carve.take(4 * tensors);
    plan->floats = carve.bytes;
    plan->items = items;
    plan->tensors = (int32_t)tensors;
    AfList a{};
    std::vector<int> entry;
    int seg = 0;
    for_each_group(n_tensors, kGroup, a.item_start,
                   [&](int k, int i) {
                       const int64_t n = rows[i] * cols[i];
                       if (!n) return 0;
                       a.n[k] = n;
                       a.rows[k] = (int32_t)rows[i];
                       a.cols[k] = (int32_t)cols[i];
                       a.flags[k] = flags[i];
                       a.seg_start[k] = seg;
                       a.ws[k] = region[i];
                       entry.push_back(i);
                       if (!is_factored(rows[i], cols[i], flags[i])) return (int)chunk_items(n);
                       a.flags[k] |= kFactored | (rows[i] <= cols[i] ? kNormRows : 0);
                       seg += (int)((rows[i] + kSeg - 1) / kSeg + (cols[i] + kSeg - 1) / kSeg);
                       return (int)(((rows[i] + kTileRows - 1) / kTileRows) * ((cols[i] + kTileCols - 1) / kTileCols));
                   },
                   [&](int k, int group_items) {
                       a.seg_start[k] = seg;
                       a.n_tensors = k;
                       plan->lists.push_back(a);
                       plan->entry.push_back(entry);
                       a.tensor_base += k;          // (for the next group: tensors and work items of the launches before it)
                       a.item_base += group_items;
                       entry.clear();
                       seg = 0;
                   });
    return 0;
}

}  // namespace

extern "C" {

int zett_op_adafactor_workspace_floats(const int64_t* rows, const int64_t* cols, const uint8_t* flags, int32_t n_tensors, int64_t* floats) {
    if (!floats) return fail(ZETT_E_INVALID, "null argument");
    Plan plan;
    if (int rc = make_plan(rows, cols, flags, n_tensors, &plan)) return rc;
    *floats = std::max<int64_t>(plan.floats, 16);
    return 0;
}

int zett_op_adafactor_step(void* const* params, void* const* grads, void* const* v_row, void* const* v_col, void* const* v, const int64_t* rows, const int64_t* cols,
                           const uint8_t* flags, int32_t n_tensors, double lr, double weight_decay, double max_norm, int32_t zero_grad, float* workspace,
                           int64_t workspace_floats, float* record, void* stream) {
    if (!record || (n_tensors > 0 && (!params || !grads || !v_row || !v_col || !v))) return fail(ZETT_E_INVALID, "null argument");
    Plan plan;
    if (int rc = make_plan(rows, cols, flags, n_tensors, &plan)) return rc;
    if (!(max_norm > 0)) return fail(ZETT_E_INVALID, "max_norm must be positive (infinity: no clip)");
    if (plan.floats > workspace_floats || !workspace) return fail(ZETT_E_INVALID, "the workspace holds %lld floats, %lld are needed (zett_op_adafactor_workspace_floats)",
                                                                  (long long)workspace_floats, (long long)plan.floats);
    if ((uintptr_t)workspace & 15) return fail(ZETT_E_INVALID, "the workspace must be 16-byte aligned");
    for (size_t l = 0; l < plan.lists.size(); ++l) {
        AfList& a = plan.lists[l];
        for (int k = 0; k < a.n_tensors; ++k) {
            const int i = plan.entry[l][k];
            const bool frozen = a.flags[k] & ZETT_ADAMW_FROZEN, factored = a.flags[k] & kFactored;
            if (!grads[i] || (!frozen && (!params[i] || (factored ? (!v_row[i] || !v_col[i]) : !v[i]))))
                return fail(ZETT_E_INVALID, "tensor %d: null parameter, gradient or statistics pointer", i);
            if ((((uintptr_t)grads[i] | (uintptr_t)params[i] | (uintptr_t)v_row[i] | (uintptr_t)v_col[i] | (uintptr_t)v[i]) & 3)) return fail(ZETT_E_INVALID, "tensor %d: a pointer is not 4-byte aligned", i);
            a.p[k] = (float*)params[i];
            a.g[k] = (float*)grads[i];
            if (factored) {      // optax's v_row belongs to the smaller dimension: the rows' statistics when rows <= cols
                const bool norm_rows = a.flags[k] & kNormRows;
                a.va[k] = (float*)(norm_rows ? v_row[i] : v_col[i]);
                a.vb[k] = (float*)(norm_rows ? v_col[i] : v_row[i]);
            } else {
                a.va[k] = (float*)v[i];
                a.vb[k] = nullptr;
            }
        }
    }
    hipStream_t st = (hipStream_t)stream;
    AfHyper h{};
    h.lr = lr; h.max_norm = max_norm; h.wd = (float)weight_decay; h.zero_grad = zero_grad;
    float* ws = workspace;
    for (const AfList& a : plan.lists) hipLaunchKernelGGL(af_pass1_kernel, dim3(std::min<int>(a.item_start[a.n_tensors], kMaxGrid)), dim3(256), 0, st, a, plan.ws, ws);
    hipLaunchKernelGGL(af_norm_kernel, dim3(1), dim3(256), 0, st, (const float*)(ws + plan.ws.gpart), plan.items, max_norm, record);
    for (const AfList& a : plan.lists)
        if (a.seg_start[a.n_tensors]) hipLaunchKernelGGL(af_stats_kernel, dim3(std::min<int>(a.seg_start[a.n_tensors], kMaxGrid)), dim3(256), 0, st, a, ws, (const float*)record);
    for (const AfList& a : plan.lists) hipLaunchKernelGGL(af_tensor_kernel, dim3(a.n_tensors), dim3(256), 0, st, a, plan.ws, h, 0, ws, (const float*)record);
    for (const AfList& a : plan.lists) hipLaunchKernelGGL(af_pass2_kernel, dim3(std::min<int>(a.item_start[a.n_tensors], kMaxGrid)), dim3(256), 0, st, a, plan.ws, ws, (const float*)record);
    for (const AfList& a : plan.lists) hipLaunchKernelGGL(af_tensor_kernel, dim3(a.n_tensors), dim3(256), 0, st, a, plan.ws, h, 1, ws, (const float*)record);
    for (const AfList& a : plan.lists) hipLaunchKernelGGL(af_pass3_kernel, dim3(std::min<int>(a.item_start[a.n_tensors], kMaxGrid)), dim3(256), 0, st, a, plan.ws, h, ws, (const float*)record);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
