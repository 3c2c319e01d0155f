// train_attention.hip — masked attention forward and backward of the training step (include/zett_hip.h, "training use"), with
// eager semantics: finfo.min on masked keys, uniform rows when every key is masked.  Dense (the reference's [N, L', H] layout) or
// packed (only the positions a row keeps), all positions as queries or position 0 only.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "train_common.hip.h"

using namespace zett;

namespace {

// ---- masked attention (eager semantics), dense or packed ------------------------------------------------------------------
// What both kernels are given.  The positions of row n are rows [t0, t1) of k / v (and of q / ctx
// unless cls_only): t0 = row_offset[n], t1 = row_offset[n + 1] (packed: only the positions the row keeps), or n * seq and
// (n + 1) * seq when row_offset is null (the reference's dense layout).  mask[t] = 1: position t is visible as a key.
// cls_only: the query is position 0 only, q and ctx hold ONE row per vocabulary row (the position-0-only last layer).
// probs [n_rows, heads, seq, seq] (row-major in the padded seq) is kept for the backward.  t1 - t0 <= seq <= ATT_MAX_L.
constexpr int ATT_MAX_L = 32;

// One WAVE per (vocabulary row, head), four heads per workgroup; no LDS, no barrier.  A lane owns head-dim columns lane + 64 e
// (e < DV: head dims up to 64 DV); the row's keys and values live in registers (LMAX positions, loops over positions fully
// unrolled with wave-uniform guards, so the arrays are never indexed dynamically), every load of the row is in flight before
// the first reduction, and each query position is one pass: LMAX dot products (butterfly sums leave every lane with the
// result), the softmax computed redundantly by all lanes, the weighted sum of the values.
template <int LMAX, int DV>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, const float* __restrict__ v, int ld,
                                                       const uint8_t* __restrict__ mask, const int32_t* __restrict__ row_offset, int seq, int heads, int d,
                                                       float scaling, int cls_only, float* __restrict__ ctx, int ld_ctx, float* __restrict__ probs,
                                                       void* __restrict__ ctx_lo, int lo_kind) {
    const int groups = (heads + 3) >> 2;
    const int n = blockIdx.x / groups, hd = (blockIdx.x % groups) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (hd >= heads) return;
    const size_t base = row_offset ? (size_t)row_offset[n] : (size_t)n * seq;
    const int L = row_offset ? row_offset[n + 1] - row_offset[n] : seq;
    const int nq = cls_only ? 1 : L;
    const size_t qbase = cls_only ? (size_t)n : base;
    float kr[LMAX][DV], vr[LMAX][DV], bias[LMAX];
#pragma unroll
    for (int j = 0; j < LMAX; ++j) {
        bias[j] = 0.f;
#pragma unroll
        for (int e = 0; e < DV; ++e) { kr[j][e] = 0.f; vr[j][e] = 0.f; }
        if (j < L) {
            bias[j] = mask[base + j] ? 0.f : -FLT_MAX;             // finfo(float32).min on masked keys
#pragma unroll
            for (int e = 0; e < DV; ++e) {
                const int c = lane + 64 * e;
                if (c < d) { kr[j][e] = k[(base + j) * ld + hd * d + c]; vr[j][e] = v[(base + j) * ld + hd * d + c]; }
            }
        }
    }
    for (int i = 0; i < nq; ++i) {
        float qr[DV];
#pragma unroll
        for (int e = 0; e < DV; ++e) { const int c = lane + 64 * e; qr[e] = c < d ? q[(qbase + i) * ldq + hd * d + c] : 0.f; }
        float sc[LMAX];
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < LMAX; ++j) {
            sc[j] = 0.f;
            if (j < L) {
                float p = 0.f;
#pragma unroll
                for (int e = 0; e < DV; ++e) p += qr[e] * kr[j][e];
                sc[j] = wave_sum(p) * scaling + bias[j];
                mx = fmaxf(mx, sc[j]);
            }
        }
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < LMAX; ++j)
            if (j < L) { sc[j] = expf(sc[j] - mx); sum += sc[j]; }
        float acc[DV];
#pragma unroll
        for (int e = 0; e < DV; ++e) acc[e] = 0.f;
        float* prow = probs + (((size_t)n * heads + hd) * seq + i) * seq;
#pragma unroll
        for (int j = 0; j < LMAX; ++j)
            if (j < L) {
                const float p = sc[j] / sum;
                if (lane == 0) prow[j] = p;
#pragma unroll
                for (int e = 0; e < DV; ++e) acc[e] += p * vr[j][e];
            }
#pragma unroll
        for (int e = 0; e < DV; ++e) {
            const int c = lane + 64 * e;
            if (c < d) {
                const size_t o = (qbase + i) * ld_ctx + hd * d + c;
                // lo_kind != 0: the context only feeds a contraction (and its transposed twin in the backward): written as that 16-bit
                // operand, its fp32 form is never stored
                if (lo_kind == 0) ctx[o] = acc[e];
                else if (lo_kind == 1) ((bf16_t*)ctx_lo)[o] = f32_to_bf16(acc[e]);
                else ((f16_t*)ctx_lo)[o] = (f16_t)acc[e];
            }
        }
    }
}

// dv_j = sum_i p_ij dctx_i;  dp_ij = dctx_i . v_j;  ds_ij = p_ij (dp_ij - sum_j' p_ij' dp_ij');
// dq_i = scaling sum_j ds_ij k_j;  dk_j = scaling sum_i ds_ij q_i.   Same layout as the forward: keys, values and the running
// dk / dv of the row in registers, one pass per query position.
template <int LMAX, int DV>
__global__ __launch_bounds__(256) void attn_bwd_kernel(const float* __restrict__ dctx, int ld_ctx, const float* __restrict__ q, int ldq, const float* __restrict__ k,
                                                       const float* __restrict__ v, int ld, const float* __restrict__ probs, const int32_t* __restrict__ row_offset,
                                                       int seq, int heads, int d, float scaling, int cls_only, float* __restrict__ dq, int ld_dq,
                                                       float* __restrict__ dk, float* __restrict__ dv, int ld_d) {
    const int groups = (heads + 3) >> 2;
    const int n = blockIdx.x / groups, hd = (blockIdx.x % groups) * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (hd >= heads) return;
    const size_t base = row_offset ? (size_t)row_offset[n] : (size_t)n * seq;
    const int L = row_offset ? row_offset[n + 1] - row_offset[n] : seq;
    const int nq = cls_only ? 1 : L;
    const size_t qbase = cls_only ? (size_t)n : base;
    float kr[LMAX][DV], vr[LMAX][DV], dkr[LMAX][DV], dvr[LMAX][DV];
#pragma unroll
    for (int j = 0; j < LMAX; ++j) {
#pragma unroll
        for (int e = 0; e < DV; ++e) { kr[j][e] = 0.f; vr[j][e] = 0.f; dkr[j][e] = 0.f; dvr[j][e] = 0.f; }
        if (j < L) {
#pragma unroll
            for (int e = 0; e < DV; ++e) {
                const int c = lane + 64 * e;
                if (c < d) { kr[j][e] = k[(base + j) * ld + hd * d + c]; vr[j][e] = v[(base + j) * ld + hd * d + c]; }
            }
        }
    }
    for (int i = 0; i < nq; ++i) {
        float qr[DV], gr[DV];
#pragma unroll
        for (int e = 0; e < DV; ++e) {
            const int c = lane + 64 * e;
            qr[e] = c < d ? q[(qbase + i) * ldq + hd * d + c] : 0.f;
            gr[e] = c < d ? dctx[(qbase + i) * ld_ctx + hd * d + c] : 0.f;
        }
        const float* prow = probs + (((size_t)n * heads + hd) * seq + i) * seq;
        float pr[LMAX], dp[LMAX];
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < LMAX; ++j) {
            pr[j] = 0.f; dp[j] = 0.f;
            if (j < L) {
                pr[j] = prow[j];
                float a = 0.f;
#pragma unroll
                for (int e = 0; e < DV; ++e) a += gr[e] * vr[j][e];
                dp[j] = wave_sum(a);
                dot += pr[j] * dp[j];
            }
        }
        float aq[DV];
#pragma unroll
        for (int e = 0; e < DV; ++e) aq[e] = 0.f;
#pragma unroll
        for (int j = 0; j < LMAX; ++j)
            if (j < L) {
                const float dsv = pr[j] * (dp[j] - dot);
#pragma unroll
                for (int e = 0; e < DV; ++e) {
                    aq[e] += dsv * kr[j][e];
                    dkr[j][e] += dsv * qr[e];
                    dvr[j][e] += pr[j] * gr[e];
                }
            }
#pragma unroll
        for (int e = 0; e < DV; ++e) { const int c = lane + 64 * e; if (c < d) dq[(qbase + i) * ld_dq + hd * d + c] = aq[e] * scaling; }
    }
#pragma unroll
    for (int j = 0; j < LMAX; ++j)
        if (j < L) {
#pragma unroll
            for (int e = 0; e < DV; ++e) {
                const int c = lane + 64 * e;
                if (c < d) { dk[(base + j) * ld_d + hd * d + c] = dkr[j][e] * scaling; dv[(base + j) * ld_d + hd * d + c] = dvr[j][e]; }
            }
        }
}

// The register layout of both kernels: f(std::integral_constant<int, LMAX>{}, std::integral_constant<int, DV>{}) with the positions
// rounded up to LMAX = 2 / 4 / 8 / 16 / 32 and DV = 1 / 2 / 4 64-column slices of the head dim (seq <= ATT_MAX_L, head_dim <= 256: the
// callers' checks)
template <typename F> void with_att_layout(int seq, int head_dim, F&& f) {
    auto slices = [&](auto lmax) {
        if (head_dim <= 64) f(lmax, std::integral_constant<int, 1>{});
        else if (head_dim <= 128) f(lmax, std::integral_constant<int, 2>{});
        else f(lmax, std::integral_constant<int, 4>{});
    };
    if (seq <= 2) slices(std::integral_constant<int, 2>{});
    else if (seq <= 4) slices(std::integral_constant<int, 4>{});
    else if (seq <= 8) slices(std::integral_constant<int, 8>{});
    else if (seq <= 16) slices(std::integral_constant<int, 16>{});
    else slices(std::integral_constant<int, 32>{});
}

}  // namespace

extern "C" {

int zett_op_attention_fwd_f32(const float* q, int32_t ldq, const float* k, const float* v, int32_t ld, const uint8_t* mask, const int32_t* row_offset,
                              int64_t n_rows, int32_t seq, int32_t heads, int32_t head_dim, int32_t cls_only, float* ctx, int32_t ld_ctx, float* probs,
                              void* ctx_lo, int32_t prec, void* stream) {
    if (!q || !k || !v || !mask || (!ctx && !ctx_lo) || !probs) return fail(ZETT_E_INVALID, "null argument");
    if (const int rc = ctx_lo ? lo_prec_ok(prec, "the 16-bit context takes") : 0) return rc;
    if (seq < 1 || seq > ATT_MAX_L) return fail(ZETT_E_INVALID, "training attention handles 1 <= L <= %d positions, got %d", ATT_MAX_L, seq);
    if (heads < 1 || head_dim < 1 || head_dim > 256) return fail(ZETT_E_INVALID, "training attention handles head dims up to 256, got %d", head_dim);
    if (n_rows <= 0) return 0;
    const dim3 grid((unsigned)(n_rows * ((heads + 3) / 4)));
    const float scaling = 1.0f / sqrtf((float)head_dim);
    const int lo_kind = !ctx_lo ? 0 : (prec == ZETT_PREC_BF16 ? 1 : 2);
    with_att_layout(seq, head_dim, [&](auto lmax, auto slices) {
        hipLaunchKernelGGL((attn_fwd_kernel<decltype(lmax)::value, decltype(slices)::value>), grid, dim3(256), 0, (hipStream_t)stream, q, ldq, k, v, ld, mask, row_offset, seq,
                           heads, head_dim, scaling, cls_only, ctx, ld_ctx, probs, ctx_lo, lo_kind);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_attention_bwd_f32(const float* dctx, int32_t ld_ctx, const float* q, int32_t ldq, const float* k, const float* v, int32_t ld, const float* probs,
                              const int32_t* row_offset, int64_t n_rows, int32_t seq, int32_t heads, int32_t head_dim, int32_t cls_only, float* dq, int32_t ld_dq,
                              float* dk, float* dv, int32_t ld_d, void* stream) {
    if (!dctx || !q || !k || !v || !probs || !dq || !dk || !dv) return fail(ZETT_E_INVALID, "null argument");
    if (seq < 1 || seq > ATT_MAX_L) return fail(ZETT_E_INVALID, "training attention handles 1 <= L <= %d positions, got %d", ATT_MAX_L, seq);
    if (heads < 1 || head_dim < 1 || head_dim > 256) return fail(ZETT_E_INVALID, "training attention handles head dims up to 256, got %d", head_dim);
    if (head_dim > 128 && seq > 16) return fail(ZETT_E_INVALID, "training attention backward: head dims above 128 are handled for up to 16 positions, got %d", seq);
    if (n_rows <= 0) return 0;
    const dim3 grid((unsigned)(n_rows * ((heads + 3) / 4)));
    const float scaling = 1.0f / sqrtf((float)head_dim);
    with_att_layout(seq, head_dim, [&](auto lmax, auto slices) {
        constexpr int LMAX = decltype(lmax)::value, DV = decltype(slices)::value;
        if constexpr (LMAX < 32 || DV < 4)      // (<32, 4> would not fit its registers: refused above)
            hipLaunchKernelGGL((attn_bwd_kernel<LMAX, DV>), grid, dim3(256), 0, (hipStream_t)stream, dctx, ld_ctx, q, ldq, k, v, ld, probs, row_offset, seq, heads, head_dim,
                               scaling, cls_only, dq, ld_dq, dk, dv, ld_d);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
