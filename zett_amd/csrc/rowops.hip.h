// rowops.hip.h — the HBM-bound kernels of the hypernet forward (gfx950).
//
//   pair_rows       the plan (plan.hip.h; made by the kernels of plan.hip) per buffer row of a chunk
//   gather_src      A2/A3: source-embedding gather + in_scaler + fallback select
//   layernorm_rows  LayerNorm over H (+ the RobertaEmbeddings add for the embed variant)
//   attention_rows  per-row bidirectional attention over <= L' packed positions
//   (the position-0 readout + bias head is the last LayerNorm launch: layernorm_rows with LnReadout)
//
// All of them are one-pass streaming kernels: 16-byte vector accesses, one
// workgroup (or wave) per row, no inter-workgroup communication.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "elem.hip.h"
#include "plan.hip.h"
#include "scan.hip.h"

namespace zett {

// (the kernels that are not templates are `static`: this header is part of more than one translation unit — zett_hip.hip and
//  rowops_entry.hip — and each gets its own copy)

// pair slot per BUFFER row of a chunk (position 0 first, chunk_row below): what the residual epilogue of layer 0 indexes with
__device__ __forceinline__ int chunk_row(int t_rel, int row_rel, bool first, int rows, const int32_t* cls_slot);
static __global__ void pair_rows_kernel(int m, int tok0, int64_t row0, int rows, PlanArrays p, int32_t* __restrict__ brow_pair,
                                        const int32_t* __restrict__ cls_slot) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    const int n = p.tok_row[tok0 + t];
    brow_pair[chunk_row(t, (int)(n - row0), p.row_offset[n] == tok0 + t, rows, cls_slot)] = p.tok_pair[tok0 + t];
}

// ---------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// sum over a 256-thread workgroup; every thread gets the result
__device__ __forceinline__ float block_sum_256(float v, float* red /* [4] */) {
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

template <typename T> __device__ __forceinline__ void store_lo4(T* dst, float4 v);
template <> __device__ __forceinline__ void store_lo4<float>(float* dst, float4 v) { *(float4*)dst = v; }
template <> __device__ __forceinline__ void store_lo4<bf16_t>(bf16_t* dst, float4 v) {
    *(uint2*)dst = make_uint2(pack2_lo<bf16_t>(v.x, v.y), pack2_lo<bf16_t>(v.z, v.w));
}
template <> __device__ __forceinline__ void store_lo4<f16_t>(f16_t* dst, float4 v) {
    *(uint2*)dst = make_uint2(pack2_lo<f16_t>(v.x, v.y), pack2_lo<f16_t>(v.z, v.w));
}

template <int SRC_DTYPE> __device__ __forceinline__ float4 load_src4(const void* base, size_t elem);
template <> __device__ __forceinline__ float4 load_src4<0>(const void* base, size_t e) {
    return *(const float4*)((const float*)base + e);
}
template <> __device__ __forceinline__ float4 load_src4<1>(const void* base, size_t e) {   // fp16
    const uint2 u = *(const uint2*)((const uint16_t*)base + e);
    typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
    const f16x4 hv = __builtin_bit_cast(f16x4, u);
    return make_float4((float)hv[0], (float)hv[1], (float)hv[2], (float)hv[3]);
}
template <> __device__ __forceinline__ float4 load_src4<2>(const void* base, size_t e) {   // bf16
    const uint2 u = *(const uint2*)((const uint16_t*)base + e);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                       __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
}

// ---------------------------------------------------------------------------
// A2 + A3 (modeling_hypernet.py:170-188): one workgroup per distinct id.
//   id <  V0 : x = in_scaler.w * source_embeddings[id] + in_scaler.b   (if rescale)
//   id >= V0 : x = fallback_embeddings[id - V0]                         (never rescaled)
// ---------------------------------------------------------------------------
template <typename T, int SRC_DTYPE>
__global__ __launch_bounds__(256) void gather_src_kernel(const int32_t* __restrict__ id_list, int slot0, int n_slots,
                                                         const void* __restrict__ src, int e_in, int v0,
                                                         const float* __restrict__ fallback,
                                                         const float* __restrict__ sc_w, const float* __restrict__ sc_b,
                                                         T* __restrict__ out, int32_t* __restrict__ range_flag) {
    const int s = blockIdx.x;
    if (s >= n_slots) return;
    const int id = id_list[slot0 + s];
    T* dst = out + (size_t)s * e_in;
    bool bad = false;          // range guard: a value that does not fit the operand type (f16 only), ZETT_RANGE_SOURCE
    auto chk = [&](float4 v) {
        if (LoRange<T>::checked)
            bad |= out_of_range(v.x, LoRange<T>::limit) | out_of_range(v.y, LoRange<T>::limit) | out_of_range(v.z, LoRange<T>::limit) |
                   out_of_range(v.w, LoRange<T>::limit);
    };
    if (id >= v0) {
        const float* f = fallback + (size_t)(id - v0) * e_in;
        for (int c = threadIdx.x * 4; c < e_in; c += 1024) { const float4 v = *(const float4*)(f + c); chk(v); store_lo4<T>(dst + c, v); }
    } else {
        const size_t base = (size_t)id * e_in;
        for (int c = threadIdx.x * 4; c < e_in; c += 1024) {
            float4 v = load_src4<SRC_DTYPE>(src, base + c);
            if (sc_w) {
                const float4 w = *(const float4*)(sc_w + c), b = *(const float4*)(sc_b + c);
                v.x = w.x * v.x + b.x; v.y = w.y * v.y + b.y; v.z = w.z * v.z + b.z; v.w = w.w * v.w + b.w;
            }
            chk(v);
            store_lo4<T>(dst + c, v);
        }
    }
    range_report(range_flag, bad, ZETT_RANGE_BIT_SOURCE);
}

// ---------------------------------------------------------------------------
// LayerNorm over H for one row per workgroup (256 threads, float4 per thread, the row
// is held in registers for H <= 8192 and re-read otherwise).  Two-pass mean/variance
// like torch.nn.LayerNorm.
//   plain variant : x = in[row]
//   embed variant : RobertaEmbeddings (x + token_type[0] + position[pos]) where
//                   x = table[slot] or, for the language token (slot < 0),
//                   lang - (token_type[0] + position[L])   (modeling_hypernet.py:192-199)
// ---------------------------------------------------------------------------
struct LnEmbed {
    const float* table;        // [D, H] hoisted input projection
    const int32_t* tok_slot;
    const int32_t* tok_pos;
    const float* type0;        // [H]
    const float* pos_emb;      // [max_positions, H]
    const float* lang;         // [H] or null
    int lang_pos;              // L
    const int32_t* tok_row;    // [T] row of a packed position             } where the embed variant writes a position:
    const int32_t* row_offset; // [N+1]                                     } chunk_row() below
    int64_t row0;              // first vocabulary row of the chunk
    int rows;                  // vocabulary rows in the chunk
    // (r6) the table as the LayerNorm-fold producer left it: the 16-bit copy of the ProjectorBlock's PRE-LayerNorm sum, (mean, rstd)
    // per table row, and the block's gamma / beta — the embed variant normalises a table row as it reads it (ln_affine), so the
    // ProjectorBlock's LayerNorm is not a launch and a table element is 2 bytes instead of 4 on both sides.  null: `table` is fp32.
    const void* table_lo;      // [D, H] of the launch's operand type
    const float* table_stats;  // [D] (mean, rstd)
    const float* table_gamma;  // [H] input_projection.1.ln.weight
    const float* table_beta;   // [H]
    const int32_t* cls_slot;   // [rows] buffer row of position 0 of each vocabulary row of the chunk (chunk_row() below), or null: the row itself
};

// Row order of a chunk's hidden-state buffers: POSITION 0 FIRST.  A chunk covers vocabulary rows [row0, row0 + rows) =
// packed positions [tok0, tok0 + m) of the plan.  Buffer row r < rows holds position 0 of vocabulary row row0 + r; the other
// m - rows packed positions follow in plan order.  Only position 0 is read out (modeling_hypernet.py:234), so what the
// last layer and the output heads consume is then simply the first `rows` rows of every buffer — no gather in front of
// the last layer's query GEMM, none in front of the heads; GEMMs and LayerNorms do not care about the order of rows.
//   t_rel = packed position - tok0, row_rel = its vocabulary row - row0, first = it is the row's position 0
// cls_slot != null (lever 5, zett_hip.hip Forward::plan_single_rows): the position-0 block is a permutation of the chunk's rows —
// position 0 of vocabulary row row0 + r sits in buffer row cls_slot[r], rows with a single kept position first — and whoever reads
// the block out maps buffer rows back to vocabulary rows.  The other positions keep their place.
__device__ __forceinline__ int chunk_row(int t_rel, int row_rel, bool first, int rows, const int32_t* cls_slot) {
    return first ? (cls_slot ? cls_slot[row_rel] : row_rel) : rows + t_rel - row_rel - 1;
}

// Position-0 readout fused into the LAST LayerNorm launch (which runs on the first `rows` buffer rows only): the bias
// head (modeling_hypernet.py:260-265) is a dot product of the fp32 LayerNorm output the kernel holds anyway.
struct LnReadout {
    const float* bias_w;       // [H] bias_projection.weight, or null (predict_bias off: the bias output is 0)
    const float* bias_b;       // [1]
    float* out_bias;           // [rows] (already offset to the chunk's first row), or null: no readout
    const void* in_lo;         // 16-bit residual stream: the rows come from here ([rows, ld_in] of the launch's operand type) instead of `in`
    // (zett_forward_into: the instantiations with a destination type BT) the bias of row r goes to element bias_rows[r] (< 0: not written; null:
    // r) of out_bias, which then points at the caller's destination of the kernel's destination type
    const int64_t* bias_rows;
    int32_t* range_flag;       // ZETT_RANGE_DEST: a finite bias that became inf in an f16 destination
};

// The bias of row r: today's fp32 store (BT = void), or the destination store of zett_forward_into (BT = float / f16_t / bf16_t:
// the same fp32 value rounded to nearest even)
template <typename BT> __device__ __forceinline__ void ln_readout_store(const LnReadout& ro, int r, float v) {
    if constexpr (std::is_void<BT>::value) {
        ro.out_bias[r] = v;
    } else {
        const int64_t d = ro.bias_rows ? ro.bias_rows[r] : (int64_t)r;
        if (d < 0) return;
        ((BT*)ro.out_bias)[d] = to_lo<BT>(v);
        range_report(ro.range_flag, dest_overflow<BT>(v), ZETT_RANGE_BIT_DEST);
    }
}

constexpr int LN_MAX_VEC = 8;   // 8 float4 x 256 threads = 8192 columns in registers

// TPR = threads per row: 256 (one workgroup per row, two LDS reductions) for wide rows, 64 (one wave per
// row, four rows per workgroup, shuffle reductions only) for H <= 2048, where a 256-thread group would
// leave lanes idle and spend its time in the two barriers.
// Outputs (each optional): out_lo = the normalised row as the 16-bit operand of the next GEMM; out_f32 = the
// normalised row in fp32 (hoisted table, output heads); stats_out = (mean, rstd) of the row, from which the residual
// epilogues and the position-0 readout recompute the fp32 row with ln_affine instead of reading it back;
// sum_out (embed variant) = the pre-LayerNorm sum itself, which those consumers then read.
// The embed variant takes packed position tok0 + r and writes buffer row chunk_row(...) (position 0 first).
// READOUT: the instantiation that also carries the bias head (LnReadout); the others ignore the argument.
template <typename T, bool EMBED, int TPR = 256, bool READOUT = false, typename BT = void>
__global__ __launch_bounds__(256) void layernorm_rows_kernel(const float* __restrict__ in, int ld_in, int rows, int H,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float eps,
                                                             float* __restrict__ out_f32, T* __restrict__ out_lo,
                                                             float* __restrict__ stats_out, float* __restrict__ sum_out,
                                                             LnEmbed emb, int tok0, LnReadout readout) {
    __shared__ float red[4];
    const int r = blockIdx.x * (256 / TPR) + (int)threadIdx.x / TPR;
    if (r >= rows) return;                 // TPR = 64: whole waves leave, and no barrier follows
    const int nvec = H >> 2;
    const int tid = threadIdx.x % TPR;
    auto row_sum = [&](float x_) { return TPR == 256 ? block_sum_256(x_, red) : wave_sum(x_); };
    const float* x = nullptr;
    const float* posr = nullptr;
    bool is_lang = false;
    int ro = r;                            // output row
    const T* tbl_lo = nullptr;             // EMBED on the 16-bit table: the row's 16-bit pre-LayerNorm sum and its statistics
    float2 tbl_st = make_float2(0.f, 1.f);
    if constexpr (EMBED) {
        const int slot = emb.tok_slot[tok0 + r];
        is_lang = slot < 0;
        if (emb.table_lo && !is_lang) {
            tbl_lo = (const T*)emb.table_lo + (size_t)slot * H;
            tbl_st = *(const float2*)(emb.table_stats + 2 * (size_t)slot);
            x = emb.lang;                  // (not read)
        } else
        x = is_lang ? emb.lang : emb.table + (size_t)slot * H;
        posr = emb.pos_emb + (size_t)emb.tok_pos[tok0 + r] * H;
        if (emb.tok_row) {                 // (null: rows are pairs, written in place)
            const int n = emb.tok_row[tok0 + r];
            ro = chunk_row(r, (int)(n - emb.row0), emb.row_offset[n] == tok0 + r, emb.rows, emb.cls_slot);
        }
    } else {
        x = in + (size_t)r * ld_in;
    }
    auto load = [&](int v) -> float4 {
        if constexpr (READOUT && sizeof(T) == 2) {
            if (readout.in_lo) {
                const uint2 u = *(const uint2*)((const T*)readout.in_lo + (size_t)r * ld_in + v * 4);
                float4 a;
                unpack2_lo<T>(u.x, a.x, a.y); unpack2_lo<T>(u.y, a.z, a.w);
                return a;
            }
        }
        float4 a;
        if constexpr (EMBED && sizeof(T) == 2) {
            if (tbl_lo) {          // (uniform per row: a table row of the 16-bit table, normalised on the fly)
                const uint2 u = *(const uint2*)(tbl_lo + v * 4);
                unpack2_lo<T>(u.x, a.x, a.y); unpack2_lo<T>(u.y, a.z, a.w);
                const float4 g = *(const float4*)(emb.table_gamma + v * 4), b = *(const float4*)(emb.table_beta + v * 4);
                a = make_float4(ln_affine(a.x, tbl_st.x, tbl_st.y, g.x, b.x), ln_affine(a.y, tbl_st.x, tbl_st.y, g.y, b.y),
                                ln_affine(a.z, tbl_st.x, tbl_st.y, g.z, b.z), ln_affine(a.w, tbl_st.x, tbl_st.y, g.w, b.w));
            } else {
                a = *(const float4*)(x + v * 4);
            }
        } else {
            a = *(const float4*)(x + v * 4);
        }
        if constexpr (EMBED) {
            const float4 t0 = *(const float4*)(emb.type0 + v * 4);
            const float4 p = *(const float4*)(posr + v * 4);
            if (is_lang) {   // lang -= type0 + pos[L]   (then the embeddings add them back)
                const float4 pl = *(const float4*)(emb.pos_emb + (size_t)emb.lang_pos * H + v * 4);
                a.x -= (t0.x + pl.x); a.y -= (t0.y + pl.y); a.z -= (t0.z + pl.z); a.w -= (t0.w + pl.w);
            }
            a.x = (a.x + t0.x) + p.x; a.y = (a.y + t0.y) + p.y; a.z = (a.z + t0.z) + p.z; a.w = (a.w + t0.w) + p.w;
        }
        return a;
    };
    float4 v[LN_MAX_VEC];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAX_VEC; ++j) {
        const int idx = tid + TPR * j;
        if (idx < nvec) { v[j] = load(idx); s += (v[j].x + v[j].y) + (v[j].z + v[j].w); }
    }
    for (int idx = tid + TPR * LN_MAX_VEC; idx < nvec; idx += TPR) { const float4 a = load(idx); s += (a.x + a.y) + (a.z + a.w); }
    const float mean = row_sum(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAX_VEC; ++j) {
        const int idx = tid + TPR * j;
        if (idx < nvec) {
            const float a = v[j].x - mean, b = v[j].y - mean, c = v[j].z - mean, d = v[j].w - mean;
            q += (a * a + b * b) + (c * c + d * d);
        }
    }
    for (int idx = tid + TPR * LN_MAX_VEC; idx < nvec; idx += TPR) {
        const float4 t = load(idx);
        const float a = t.x - mean, b = t.y - mean, c = t.z - mean, d = t.w - mean;
        q += (a * a + b * b) + (c * c + d * d);
    }
    const float var = row_sum(q) / (float)H;
    const float rstd = 1.0f / sqrtf(var + eps);
    if (stats_out && tid == 0) *(float2*)(stats_out + 2 * (size_t)ro) = make_float2(mean, rstd);
    float dot = 0.f;
    auto emit = [&](int idx, float4 a) {
        const float4 g = *(const float4*)(gamma + idx * 4), b = *(const float4*)(beta + idx * 4);
        const float4 o = make_float4(ln_affine(a.x, mean, rstd, g.x, b.x), ln_affine(a.y, mean, rstd, g.y, b.y),
                                     ln_affine(a.z, mean, rstd, g.z, b.z), ln_affine(a.w, mean, rstd, g.w, b.w));
        if (EMBED && sum_out) *(float4*)(sum_out + (size_t)ro * H + idx * 4) = a;
        if (out_f32) *(float4*)(out_f32 + (size_t)ro * H + idx * 4) = o;
        if (out_lo) store_lo4<T>(out_lo + (size_t)ro * H + idx * 4, o);
        if (READOUT && readout.bias_w) {
            const float4 w = *(const float4*)(readout.bias_w + idx * 4);
            dot += (o.x * w.x + o.y * w.y) + (o.z * w.z + o.w * w.w);
        }
    };
#pragma unroll
    for (int j = 0; j < LN_MAX_VEC; ++j) {
        const int idx = tid + TPR * j;
        if (idx < nvec) emit(idx, v[j]);
    }
    for (int idx = tid + TPR * LN_MAX_VEC; idx < nvec; idx += TPR) emit(idx, load(idx));
    if constexpr (READOUT) {
        if (readout.out_bias) {            // (uniform over the launch: every thread of the row takes the reduction)
            const float tot = row_sum(dot);
            if (tid == 0) ln_readout_store<BT>(readout, r, readout.bias_w ? tot + readout.bias_b[0] : 0.f);
        }
    }
}

// ---------------------------------------------------------------------------
// (r2: keeping the <= 8 K/V vectors of a row in registers instead of re-reading them per query was measured and
//  rejected — 172 VGPRs, two waves per SIMD, 0.99 ms instead of 0.54 ms per launch: the re-reads hit L1/L2, and at
//  0.54 ms the kernel already moves its algorithmic 2.5 GB at 4.7 TB/s.)
// Attention over the packed positions of one row (A6).  One wave handles one row and
// one group of 512 hidden columns (8 per lane): 512/d heads at a time, head-local
// reductions by xor-shuffles over d/8 lanes.  Two passes over the keys (row max, then
// exp / sum / PV) reproduce softmax(QKᵀ·d^-½ + mask)·V of eager_attention_forward; keys
// with ids == pad contribute exactly 0 (their exp underflows to 0 in the reference),
// uniform rows weigh every position equally.
// ---------------------------------------------------------------------------
template <typename T> struct Vec8 { float v[8]; };

template <typename T> __device__ __forceinline__ void load8(const T* p, float (&o)[8]);
template <> __device__ __forceinline__ void load8<float>(const float* p, float (&o)[8]) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}
template <typename T> __device__ __forceinline__ void load8_16bit(const T* p, float (&o)[8]) {
    const uint4 u = *(const uint4*)p;
    unpack2_lo<T>(u.x, o[0], o[1]); unpack2_lo<T>(u.y, o[2], o[3]);
    unpack2_lo<T>(u.z, o[4], o[5]); unpack2_lo<T>(u.w, o[6], o[7]);
}
template <> __device__ __forceinline__ void load8<bf16_t>(const bf16_t* p, float (&o)[8]) { load8_16bit<bf16_t>(p, o); }
template <> __device__ __forceinline__ void load8<f16_t>(const f16_t* p, float (&o)[8]) { load8_16bit<f16_t>(p, o); }
template <typename T> __device__ __forceinline__ void store8(T* p, const float (&o)[8]);
template <> __device__ __forceinline__ void store8<float>(float* p, const float (&o)[8]) {
    *(float4*)p = make_float4(o[0], o[1], o[2], o[3]);
    *(float4*)(p + 4) = make_float4(o[4], o[5], o[6], o[7]);
}
template <typename T> __device__ __forceinline__ void store8_16bit(T* p, const float (&o)[8]) {
    *(uint4*)p = make_uint4(pack2_lo<T>(o[0], o[1]), pack2_lo<T>(o[2], o[3]), pack2_lo<T>(o[4], o[5]), pack2_lo<T>(o[6], o[7]));
}
template <> __device__ __forceinline__ void store8<bf16_t>(bf16_t* p, const float (&o)[8]) { store8_16bit<bf16_t>(p, o); }
template <> __device__ __forceinline__ void store8<f16_t>(f16_t* p, const float (&o)[8]) { store8_16bit<f16_t>(p, o); }

// ---- narrow rows (r6): layernorm_rows_kernel for 16-bit operand types and H <= 2048, EIGHT columns per lane -------------------
// The one-wave-per-row instantiation above (TPR = 64, float4 / 8-byte accesses) is latency-bound on the narrow hypernets: at
// H = 768 a wave has 1.5 KB in flight and four waves fit a SIMD (106 VGPRs) — 1.8 TB/s on XLM-R's embeddings launch.  Here a lane
// takes 8 consecutive columns (16-byte accesses on the 16-bit side, two float4 on the fp32 side) and a row takes TPR = 32 lanes
// for H <= 1024 (two rows per wave) or 64 for H <= 2048: H = 8 * TPR * NV with NV <= 4 vectors per lane.  Element for element the
// arithmetic of layernorm_rows_kernel (the same load / ln_affine / emit expressions); only the ORDER in which a row's values are
// added up for its mean and variance differs (8 per lane, then a butterfly over TPR lanes).
template <int TPR>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = TPR / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// lanes per row of layernorm_rows8_kernel for rows of H columns, or 0: the row does not fit (H = 8 * TPR * NV, NV <= 4)
inline int ln_rows8_tpr(int H) {
    if (H % 256 == 0 && H <= 1024) return 32;
    if (H % 512 == 0 && H <= 2048) return 64;
    return 0;
}

template <typename T, bool EMBED, int TPR, bool READOUT, typename BT = void>
__global__ __launch_bounds__(256) void layernorm_rows8_kernel(const float* __restrict__ in, int ld_in, int rows, int H,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float eps,
                                                              float* __restrict__ out_f32, T* __restrict__ out_lo,
                                                              float* __restrict__ stats_out, float* __restrict__ sum_out,
                                                              LnEmbed emb, int tok0, LnReadout readout) {
    static_assert(sizeof(T) == 2 && (TPR == 32 || TPR == 64), "16-bit operand types, 32 or 64 lanes per row");
    constexpr int NVMAX = 4;
    const int r = blockIdx.x * (256 / TPR) + (int)threadIdx.x / TPR;
    if (r >= rows) return;                 // (a lane group leaves: the reductions below stay inside a group)
    const int nv = H / (8 * TPR);          // vectors of 8 columns per lane, <= NVMAX (the launcher checks)
    const int tid = threadIdx.x % TPR;
    const float* x = nullptr;
    const float* posr = nullptr;
    bool is_lang = false;
    int ro = r;
    const T* tbl_lo = nullptr;
    float2 tbl_st = make_float2(0.f, 1.f);
    if constexpr (EMBED) {
        const int slot = emb.tok_slot[tok0 + r];
        is_lang = slot < 0;
        if (emb.table_lo && !is_lang) {
            tbl_lo = (const T*)emb.table_lo + (size_t)slot * H;
            tbl_st = *(const float2*)(emb.table_stats + 2 * (size_t)slot);
            x = emb.lang;                  // (not read)
        } else
        x = is_lang ? emb.lang : emb.table + (size_t)slot * H;
        posr = emb.pos_emb + (size_t)emb.tok_pos[tok0 + r] * H;
        if (emb.tok_row) {
            const int n = emb.tok_row[tok0 + r];
            ro = chunk_row(r, (int)(n - emb.row0), emb.row_offset[n] == tok0 + r, emb.rows, emb.cls_slot);
        }
    } else {
        x = in + (size_t)r * ld_in;
    }
    auto load = [&](int c, float (&a)[8]) {          // the 8 values of columns [c, c + 8)
        bool have = false;
        if constexpr (READOUT) {
            if (readout.in_lo) { load8<T>((const T*)readout.in_lo + (size_t)r * ld_in + c, a); have = true; }
        }
        if constexpr (EMBED) {
            if (tbl_lo) {          // a row of the 16-bit table, normalised on the fly
                load8<T>(tbl_lo + c, a);
                float g[8], b[8];
                load8<float>(emb.table_gamma + c, g);
                load8<float>(emb.table_beta + c, b);
#pragma unroll
                for (int k = 0; k < 8; ++k) a[k] = ln_affine(a[k], tbl_st.x, tbl_st.y, g[k], b[k]);
                have = true;
            }
        }
        if (!have) load8<float>(x + c, a);
        if constexpr (EMBED) {
            float t0[8], p[8];
            load8<float>(emb.type0 + c, t0);
            load8<float>(posr + c, p);
            if (is_lang) {   // lang -= type0 + pos[L]   (then the embeddings add them back)
                float pl[8];
                load8<float>(emb.pos_emb + (size_t)emb.lang_pos * H + c, pl);
#pragma unroll
                for (int k = 0; k < 8; ++k) a[k] -= (t0[k] + pl[k]);
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] = (a[k] + t0[k]) + p[k];
        }
    };
    float v[NVMAX][8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NVMAX; ++j) {
        if (j < nv) {
            load((tid + TPR * j) * 8, v[j]);
            s += ((v[j][0] + v[j][1]) + (v[j][2] + v[j][3])) + ((v[j][4] + v[j][5]) + (v[j][6] + v[j][7]));
        }
    }
    const float mean = group_sum<TPR>(s) / (float)H;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < NVMAX; ++j) {
        if (j < nv) {
            float d[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) { d[k] = v[j][k] - mean; d[k] *= d[k]; }
            q += ((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7]));
        }
    }
    const float var = group_sum<TPR>(q) / (float)H;
    const float rstd = 1.0f / sqrtf(var + eps);
    if (stats_out && tid == 0) *(float2*)(stats_out + 2 * (size_t)ro) = make_float2(mean, rstd);
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < NVMAX; ++j) {
        if (j < nv) {
            const int c = (tid + TPR * j) * 8;
            float g[8], b[8], o[8];
            load8<float>(gamma + c, g);
            load8<float>(beta + c, b);
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = ln_affine(v[j][k], mean, rstd, g[k], b[k]);
            if (EMBED && sum_out) store8<float>(sum_out + (size_t)ro * H + c, v[j]);
            if (out_f32) store8<float>(out_f32 + (size_t)ro * H + c, o);
            if (out_lo) store8<T>(out_lo + (size_t)ro * H + c, o);
            if (READOUT && readout.bias_w) {
                float w[8];
                load8<float>(readout.bias_w + c, w);
                dot += ((o[0] * w[0] + o[1] * w[1]) + (o[2] * w[2] + o[3] * w[3])) + ((o[4] * w[4] + o[5] * w[5]) + (o[6] * w[6] + o[7] * w[7]));
            }
        }
    }
    if constexpr (READOUT) {
        if (readout.out_bias) {
            const float tot = group_sum<TPR>(dot);
            if (tid == 0) ln_readout_store<BT>(readout, r, readout.bias_w ? tot + readout.bias_b[0] : 0.f);
        }
    }
}

// ---- fast path of the attention kernel (16-bit operands, rows of at most ATT_FAST_KEYS packed positions: every row of the
// BASELINE workloads, hn_surface_maxlen 7 + language token) ----------------------------------------------------------------
// (r4) The generic loop below walks (query, key) pairs one after the other: a K and a V load, a shuffle reduction through the
// LDS crossbar and two expf chains per pair, each waiting for the one before — ~0.3 ns per pair and wave whatever the width,
// which on the narrow hypernets is 2-3 TB/s (XLM-R shape: 0.33 ms per launch for 1.04 GB).  Here the row's keys and values
// are fetched ONCE, all at the start (packed 16-bit, 8 registers per position), and a query handles all keys side by side:
// independent v_dot2 chains, head sums by DPP (no LDS), one v_exp_f32 per key, no running-maximum correction.
constexpr int ATT_FAST_KEYS = 8;

template <typename T> __device__ __forceinline__ float dot8_lo(const uint4& a, const uint4& b);
template <> __device__ __forceinline__ float dot8_lo<f16_t>(const uint4& a, const uint4& b) {
    typedef __attribute__((ext_vector_type(2))) _Float16 h2;
    float s = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, a.x), __builtin_bit_cast(h2, b.x), 0.f, false);
    s = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, a.y), __builtin_bit_cast(h2, b.y), s, false);
    s = __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, a.z), __builtin_bit_cast(h2, b.z), s, false);
    return __builtin_amdgcn_fdot2(__builtin_bit_cast(h2, a.w), __builtin_bit_cast(h2, b.w), s, false);
}
template <> __device__ __forceinline__ float dot8_lo<bf16_t>(const uint4& a, const uint4& b) {
    float x[8], y[8];
    unpack2_lo<bf16_t>(a.x, x[0], x[1]); unpack2_lo<bf16_t>(a.y, x[2], x[3]); unpack2_lo<bf16_t>(a.z, x[4], x[5]); unpack2_lo<bf16_t>(a.w, x[6], x[7]);
    unpack2_lo<bf16_t>(b.x, y[0], y[1]); unpack2_lo<bf16_t>(b.y, y[2], y[3]); unpack2_lo<bf16_t>(b.z, y[4], y[5]); unpack2_lo<bf16_t>(b.w, y[6], y[7]);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) s = fmaf(x[c], y[c], s);
    return s;
}
template <> __device__ __forceinline__ float dot8_lo<float>(const uint4&, const uint4&) { return 0.f; }     // (never called: the fast path is 16-bit only)

// sum over the `lph` lanes of a head (lph = head_dim / 8, a power of two): DPP inside a row of 16 lanes, ds_swizzle (no LDS
// access) across 16, a bpermute only for a head that spans the whole wave.  Every lane of the head ends with the same bits.
__device__ __forceinline__ float head_sum(float s, int lph) {
    auto dpp = [](float v, auto ctrl) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), decltype(ctrl)::value, 0xf, 0xf, true));
    };
    if (lph >= 2) s += dpp(s, std::integral_constant<int, 0xB1>{});         // quad_perm [1,0,3,2]
    if (lph >= 4) s += dpp(s, std::integral_constant<int, 0x4E>{});         // quad_perm [2,3,0,1]
    if (lph >= 8) s += dpp(s, std::integral_constant<int, 0x141>{});        // row_half_mirror
    if (lph >= 16) s += dpp(s, std::integral_constant<int, 0x140>{});       // row_mirror
    if (lph >= 32) s += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, s), (16 << 10) | 0x1f));
    if (lph >= 64) s += __shfl_xor(s, 32, 64);
    return s;
}

// How the (row, 512-column group) work of the attention kernel maps to waves: `full` waves of one row and one whole group each
// (full_groups per row), then — `pack`, and the last group is 256 / 128 / 64 columns wide — waves that take that group of
// 64 / lanes_per_row rows at a time; otherwise the partial group is one more "full" wave per row with idle lanes.
struct AttentionWaves { int64_t total, full; int full_groups, lanes_per_row; };
__host__ __device__ inline AttentionWaves attention_waves(int rows, int H, bool pack) {
    const int rem = H & 511, gfull = H >> 9;
    AttentionWaves a;
    if (pack && (rem == 256 || rem == 128 || rem == 64)) {
        a.full_groups = gfull; a.lanes_per_row = rem >> 3;
        a.full = (int64_t)rows * gfull;
        const int per = 64 / a.lanes_per_row;
        a.total = a.full + (rows + per - 1) / per;
    } else {
        a.full_groups = (H + 511) >> 9; a.lanes_per_row = 64;
        a.full = (int64_t)rows * a.full_groups;
        a.total = a.full;
    }
    return a;
}

// Rows of q / k / v / ctx are BUFFER rows (position 0 first, chunk_row above); the plan arrays are indexed by packed position.
// q: [T, ldq] per packed position, or (cls_only) [rows, ldq] holding the query of position 0
// of each row; k, v: [T, ldkv]; ctx: [T or rows, H].  cls_only: compute query 0 only and
// write it at ctx[row_local] (compact [rows, H] output for the last layer).
// cls_slot != null (lever 5): position 0 of row_local lives in buffer row cls_slot[row_local] instead — q of a cls_only launch and
// its ctx included.  flags bit 3: a row with ONE kept position takes ctx = v without loading q or k (their cells were never written).
template <typename T>
__global__ __launch_bounds__(256) void attention_rows_kernel(const T* __restrict__ qbase, size_t ldq,
                                                             const T* __restrict__ kbase, const T* __restrict__ vbase,
                                                             size_t ldkv, int H, int head_dim,
                                                             const int32_t* __restrict__ row_offset,
                                                             const uint8_t* __restrict__ row_uniform,
                                                             const uint8_t* __restrict__ tok_key, int64_t row0,
                                                             int rows, int tok0, float scaling,
                                                             int flags /* bit 0: cls_only, bit 1: fast path on, bit 2: pack a narrow last group, bit 3: single rows copy v */,
                                                             const int32_t* __restrict__ tok_pair, T* __restrict__ ctx, const int32_t* __restrict__ cls_slot) {
    const int cls_only = flags & 1;
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    // (r6) a last column group of 256 / 128 / 64 columns (H = 768: the XLM-R shape) used to leave half or more of its wave's
    // lanes idle; with flag bit 2 such a wave takes that group of 2 / 4 / 8 ROWS instead (`lpr` lanes per row, `base` = the first
    // lane of this lane's row).  Everything per row below (t0, t1, the key mask, the pair slots) is then per lane group; heads
    // never straddle a group (the group's width is a multiple of head_dim), so the head sums stay inside it.  Same arithmetic
    // per element: same bits.
    const AttentionWaves aw = attention_waves(rows, H, (flags & 4) != 0);
    if (w >= aw.total) return;
    int rl, grp, li = lane, base = 0, lpr = 64;
    bool valid = true;
    if (w < aw.full) { rl = (int)(w / aw.full_groups); grp = (int)(w % aw.full_groups); }
    else {
        lpr = aw.lanes_per_row;
        const int sub = lane / lpr;
        li = lane - sub * lpr;
        base = sub * lpr;
        rl = (int)(w - aw.full) * (64 / lpr) + sub;
        grp = aw.full_groups;
        valid = rl < rows;
        if (!valid) rl = rows - 1;                     // (a lane group past the last row repeats it and stores nothing)
    }
    const int col = grp * 512 + li * 8;
    const bool active = valid && col < H;
    const int lph = head_dim >> 3;                     // lanes per head (power of two)
    const int64_t n = row0 + rl;
    const int t0 = row_offset[n] - tok0, t1 = row_offset[n + 1] - tok0;
    const bool uniform = row_uniform[n];
    const int nq = cls_only ? 1 : (t1 - t0);
    const int ccol = active ? col : 0;
    // buffer row of packed position t of this row (position 0 first: chunk_row above)
    // (position 0's row — the one indexed load of the row map — and the offset of the others, up front: rl itself is not kept)
    const int slot0 = chunk_row(t0, rl, true, rows, cls_slot), rest = chunk_row(0, rl, false, rows, nullptr);
    auto brow = [&](int t) -> size_t { return (size_t)(t == t0 ? slot0 : rest + t); };
    // row of q / k / v of packed position t: its buffer row, or — layer 0 with the pair lever — the row of its
    // (source id, position) pair, whose Q/K/V were computed once
    // (the row's first 64 pair slots are fetched once, one per lane, and handed out by shuffle: an index load in front of
    //  every key would put a second memory round trip into the loop; a row with more than 64 packed positions —
    //  hn_surface_maxlen >= 64 is legal, max_positions is 514 — reads the slots past the 64th directly: t is
    //  wave-uniform, so the branch is too)
    int pslot = 0;
    if (tok_pair) { const int t = t0 + li; pslot = t < t1 ? tok_pair[tok0 + t] : 0; }
    auto qrow = [&](int t) -> size_t {
        if (!tok_pair) return brow(t);
        return t - t0 < lpr ? (size_t)__shfl(pslot, base + (t - t0), 64) : (size_t)tok_pair[tok0 + t];
    };
    const int nk = t1 - t0;
    if ((flags & 8) && nk == 1) {
        // One kept position (never a uniform row: the caller takes this path only when seq + lang > 1): its one key is visible, the
        // softmax weight is exactly 1 and the context is the value row — fma(1, v, 0) * (1 / 1) in the fast path, fma(0, 0, 1 * v) in the
        // generic one: v + 0 either way (a negative zero leaves as a positive one).  q and k are not loaded.
        const size_t vr = qrow(t0);
        if (active) {
            float v[8];
            load8<T>(vbase + vr * ldkv + ccol, v);
#pragma unroll
            for (int c = 0; c < 8; ++c) v[c] += 0.f;
            store8<T>(ctx + brow(t0) * H + col, v);
        }
        return;
    }
    if constexpr (sizeof(T) == 2) {
        if (nk <= ATT_FAST_KEYS && (flags & 2)) {
            // which keys count: lane j asks for key j, the answer is a wave-uniform bit mask
            const bool mine = li < nk && (uniform || tok_key[tok0 + t0 + li] != 0);
            const unsigned on = (unsigned)(__ballot(mine) >> base) & (lpr >= 32 ? 0xffffffffu : ((1u << lpr) - 1u));
            uint4 kk[ATT_FAST_KEYS], vv[ATT_FAST_KEYS], qq[ATT_FAST_KEYS];
#pragma unroll
            for (int j = 0; j < ATT_FAST_KEYS; ++j) {
                if (j < nk) {
                    const size_t kr = qrow(t0 + j);
                    kk[j] = *(const uint4*)(kbase + kr * ldkv + ccol);
                    vv[j] = *(const uint4*)(vbase + kr * ldkv + ccol);
                    if (!cls_only) qq[j] = *(const uint4*)(qbase + kr * ldq + ccol);
                }
            }
            if (cls_only) qq[0] = *(const uint4*)(qbase + brow(t0) * ldq + ccol);
            const float sc2 = scaling * 1.4426950408889634f;       // softmax in base 2: exp(x) = 2^(x log2 e)
#pragma unroll
            for (int qi = 0; qi < ATT_FAST_KEYS; ++qi) {
                if (qi < nq) {
                    float sj[ATT_FAST_KEYS];
                    float mx = -INFINITY;
#pragma unroll
                    for (int j = 0; j < ATT_FAST_KEYS; ++j) {
                        sj[j] = -INFINITY;
                        if (j < nk && ((on >> j) & 1u)) {
                            const float d = head_sum(dot8_lo<T>(qq[qi], kk[j]), lph);
                            sj[j] = uniform ? 0.f : d * sc2;
                            mx = fmaxf(mx, sj[j]);
                        }
                    }
                    float l = 0.f, acc[8];
#pragma unroll
                    for (int c = 0; c < 8; ++c) acc[c] = 0.f;
#pragma unroll
                    for (int j = 0; j < ATT_FAST_KEYS; ++j) {
                        if (j < nk && ((on >> j) & 1u)) {
                            const float pj = __builtin_amdgcn_exp2f(sj[j] - mx);
                            l += pj;
                            float v[8];
                            unpack2_lo<T>(vv[j].x, v[0], v[1]); unpack2_lo<T>(vv[j].y, v[2], v[3]);
                            unpack2_lo<T>(vv[j].z, v[4], v[5]); unpack2_lo<T>(vv[j].w, v[6], v[7]);
#pragma unroll
                            for (int c = 0; c < 8; ++c) acc[c] = fmaf(pj, v[c], acc[c]);
                        }
                    }
                    const float inv = 1.0f / l;
#pragma unroll
                    for (int c = 0; c < 8; ++c) acc[c] *= inv;
                    if (active) {
                        const size_t orow = brow(t0 + qi);      // (cls_only: qi = 0, the row's position-0 slot)
                        store8<T>(ctx + orow * H + col, acc);
                    }
                }
            }
            return;
        }
    }
    for (int qi = 0; qi < nq; ++qi) {
        float q[8];
        load8<T>(qbase + (cls_only ? brow(t0) : qrow(t0 + qi)) * ldq + ccol, q);
        // one pass over the keys with a running maximum (online softmax): K and V are read once
        float mx = -INFINITY, l = 0.f, acc[8];
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] = 0.f;
        for (int kj = t0; kj < t1; ++kj) {
            if (!uniform && !tok_key[tok0 + kj]) continue;
            float k[8], v[8];
            const size_t kr = qrow(kj);
            load8<T>(kbase + kr * ldkv + ccol, k);
            load8<T>(vbase + kr * ldkv + ccol, v);
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) s = fmaf(q[c], k[c], s);
            for (int off = 1; off < lph; off <<= 1) s += __shfl_xor(s, off, 64);
            s = uniform ? 0.f : s * scaling;
            const float nm = fmaxf(mx, s);
            const float corr = expf(mx - nm);          // first key: exp(-inf) = 0 on an all-zero state
            const float p = expf(s - nm);
            l = fmaf(l, corr, p);
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] = fmaf(acc[c], corr, p * v[c]);
            mx = nm;
        }
        const float inv = 1.0f / l;
#pragma unroll
        for (int c = 0; c < 8; ++c) acc[c] *= inv;
        if (active) {
            const size_t orow = brow(t0 + qi);      // (cls_only: qi = 0, the row's position-0 slot)
            store8<T>(ctx + orow * H + col, acc);
        }
    }
}

// ---------------------------------------------------------------------------
// LayerNorm fold: the LayerNorm between two GEMMs without a kernel that reads the fp32 rows again.
//   ln_stats_kernel   (mean, rstd) per row from the per-128-column partials the producer GEMM's epilogue wrote
//   fold_weight_kernel  one-off, at zett_finalize: W'[n,k] = lo(W[n,k] * gamma[k]),  c[n] = sum_k W'[n,k],
//                       b'[n] = b[n] + sum_k W[n,k] * beta[k]     so that   LN(x) W^T + b = rstd (x W'^T - mean c) + b'
// ---------------------------------------------------------------------------
// (r6: a version with four threads per row — every fourth partial each, combined through LDS — was 2-3 x faster on a 12-16 us kernel
//  and changed the summation order: bf16 mode, which sits ON its 1e-2 tolerance, went from 0.99e-2 to 1.002e-2 on the Llama-3 sample.
//  The sequential order of rounds 3-5 stays.)
// (r6, second version: the partials of a row are still ADDED in their sequential order — same bits — but FETCHED eight at a time:
//  the loop of rounds 3-5 waited for every load before it issued the next, 32 dependent round trips at H = 4096.  64-thread
//  workgroups, so that a 4 096-row shard's 9.7 k rows reach 150 CUs instead of 38.)
static __global__ __launch_bounds__(64) void ln_stats_kernel(const float2* __restrict__ part, int parts, int ld_part, int rows, int H, float eps,
                                                      float* __restrict__ stats) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    float s = 0.f, q = 0.f;
    const float2* col = part + r;
    int p = 0;
    for (; p + 8 <= parts; p += 8) {
        float2 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = col[(size_t)(p + j) * ld_part];
#pragma unroll
        for (int j = 0; j < 8; ++j) { s += v[j].x; q += v[j].y; }
    }
    {
        float2 v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = p + j < parts ? col[(size_t)(p + j) * ld_part] : make_float2(0.f, 0.f);
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (p + j < parts) { s += v[j].x; q += v[j].y; }
    }
    const float mean = s / (float)H;
    const float var = fmaxf(q / (float)H - mean * mean, 0.f);
    *(float2*)(stats + 2 * (size_t)r) = make_float2(mean, 1.0f / sqrtf(var + eps));
}

template <typename T>
__global__ __launch_bounds__(256) void fold_weight_kernel(const float* __restrict__ w, int K, const float* __restrict__ gamma,
                                                          const float* __restrict__ beta, const float* __restrict__ bias,
                                                          T* __restrict__ w_fold, float* __restrict__ c_out, float* __restrict__ b_out,
                                                          int32_t* __restrict__ range_flag) {
    __shared__ float red[4];
    const int n = blockIdx.x;
    const float* row = w + (size_t)n * K;
    float cs = 0.f, bs = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float x = row[k];
        if (LoRange<T>::checked) range_report(range_flag, out_of_range(x * gamma[k], LoRange<T>::limit), ZETT_RANGE_BIT_WEIGHT);
        const T lo = to_lo<T>(x * gamma[k]);
        w_fold[(size_t)n * K + k] = lo;
        cs += lo_to_f32<T>(lo);
        bs = fmaf(x, beta[k], bs);
    }
    const float ct = block_sum_256(cs, red);
    const float bt = block_sum_256(bs, red);
    if (threadIdx.x == 0) { c_out[n] = ct; b_out[n] = bias[n] + bt; }
}

// ---------------------------------------------------------------------------
// Lever 6: layer 0's Q/K/V once per distinct source id.  The embeddings' sum is x = t + c_p (t the hoisted table row,
// c_p = type0 + pos[p]) and the LayerNorm's centring is linear, so with W' = gamma (.) W of layer 0's fused qkv
//     qkv(row)[col] = r_x * ( U[slot][col] + C[p][col] - mu_x * cW[col] ) + bq[col]
// where U = t W'^T is ONE LayerNorm-fold consumer GEMM over the distinct table rows, and C = c_p W'^T, cW = colsum(W'),
// bq = beta W^T + b depend on the weights only.
//   pos_qkv_kernel   one-off, at zett_finalize: C [n_pos, N], cW [N], bq [N] in fp32 from the fp32 weight (one workgroup per
//                    output column n, its row gamma (.) W[n] in LDS, a wave per position, lanes stride k, butterfly sum)
//   pair_qkv_kernel  per forward: the rows of [q | k | v] from U, (mu_x, r_x) of the embeddings' LayerNorm, C, cW, bq
// ---------------------------------------------------------------------------
static __global__ __launch_bounds__(256) void pos_qkv_kernel(const float* __restrict__ w, int K, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, const float* __restrict__ bias,
                                                             const float* __restrict__ type0, const float* __restrict__ pos_emb, int n_pos, int N,
                                                             float* __restrict__ c_pos, float* __restrict__ c_w, float* __restrict__ b_q) {
#pragma clang fp contract(off)
    extern __shared__ float pq_row[];          // [K] gamma[k] * W[n, k]
    const int n = blockIdx.x;
    const float* row = w + (size_t)n * K;
    for (int k = threadIdx.x; k < K; k += 256) pq_row[k] = row[k] * gamma[k];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (wave == 0) {
        float cs = 0.f, bs = 0.f;
        for (int k = lane; k < K; k += 64) { cs += pq_row[k]; bs = fmaf(row[k], beta[k], bs); }
        cs = wave_sum(cs); bs = wave_sum(bs);
        if (lane == 0) { c_w[n] = cs; b_q[n] = bias[n] + bs; }
    }
    for (int p = wave; p < n_pos; p += 4) {
        const float* pr = pos_emb + (size_t)p * K;
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s = fmaf(type0[k] + pr[k], pq_row[k], s);
        s = wave_sum(s);
        if (lane == 0) c_pos[(size_t)p * N + n] = s;
    }
}

// A workgroup owns a block of PQ_COLS = 2048 columns of [q | k | v] (eight per lane, 16-byte accesses on the 16-bit side) and walks
// rows blockIdx.y, blockIdx.y + gridDim.y, ..., four at a time.  What depends on the column only is read ONCE per workgroup: cW and bq
// of the lane's columns stay in registers, C's rows of the first PQ_LDS_POS positions in LDS (a lane reads back only what it wrote
// itself: no barrier); a position beyond them reads its C row from memory.
// Output row j in [0, n):
//   tok_row == null (pair rows): slot[j], pos[j], statistics and output row j
//   tok_row != null (buffer rows of a chunk): packed position t0 + j, written to its buffer row chunk_row(...) — position 0 first,
//     the order the embeddings' LayerNorm wrote the statistics in
// The arithmetic of one element, in this order, contraction off (the compiler may not fuse the first three):
//     a = f32(U[slot][col]) + C[p][col];  b = mu_x * cW[col];  d = a - b;  v = fma(r_x, d, bq[col]);  out = to_lo(v)
// |v| beyond the f16 range (or NaN) sets ZETT_RANGE_ACTIVATION's bit, as every 16-bit writer of an activation does.
constexpr int PQ_COLS = 2048;
constexpr int PQ_LDS_POS = 8;
constexpr int PQ_UNROLL = 4;
struct PairQkvRows {
    const int32_t* slot;        // [t0 + n] table slot (row of U)
    const int32_t* pos;         // [t0 + n] position (row of C)
    int t0;
    const int32_t* tok_row;     // [t0 + n] or null
    const int32_t* row_offset;  // with tok_row
    int64_t row0; int rows;     // the chunk's first vocabulary row and its number of rows
    const int32_t* cls_slot;    // chunk_row()
};
template <typename T>
__global__ __launch_bounds__(256) void pair_qkv_kernel(const T* __restrict__ U, PairQkvRows rw, int n, const float* __restrict__ stats,
                                                       const float* __restrict__ c_pos, int n_pos_lds, const float* __restrict__ c_w,
                                                       const float* __restrict__ b_q, int N, T* __restrict__ out, size_t ld_out,
                                                       int32_t* __restrict__ range_flag) {
#pragma clang fp contract(off)
    extern __shared__ float4 pq_c[];           // [n_pos_lds][2][256]: the two float4 of lane l's columns at [p][0][l], [p][1][l]
    const int col = blockIdx.x * PQ_COLS + (int)threadIdx.x * 8;
    if (col >= N) return;                      // (N % 8 == 0; no barrier follows)
    float cw[8], bq[8];
    load8<float>(c_w + col, cw);
    load8<float>(b_q + col, bq);
    for (int p = 0; p < n_pos_lds; ++p) {
        pq_c[(p * 2) * 256 + threadIdx.x] = *(const float4*)(c_pos + (size_t)p * N + col);
        pq_c[(p * 2 + 1) * 256 + threadIdx.x] = *(const float4*)(c_pos + (size_t)p * N + col + 4);
    }
    bool bad = false;
    for (int j0 = blockIdx.y; j0 < n; j0 += PQ_UNROLL * gridDim.y) {
        int slot[PQ_UNROLL], pos[PQ_UNROLL], ro[PQ_UNROLL];
        float2 st[PQ_UNROLL];
        float u[PQ_UNROLL][8];
#pragma unroll
        for (int i = 0; i < PQ_UNROLL; ++i) {
            const int j = j0 + i * gridDim.y;
            if (j >= n) { ro[i] = -1; continue; }
            const int t = rw.t0 + j;
            slot[i] = rw.slot[t];
            pos[i] = rw.pos[t];
            ro[i] = j;
            if (rw.tok_row) {
                const int r = rw.tok_row[t];
                ro[i] = chunk_row(j, (int)(r - rw.row0), rw.row_offset[r] == t, rw.rows, rw.cls_slot);
            }
        }
#pragma unroll
        for (int i = 0; i < PQ_UNROLL; ++i) {
            if (ro[i] < 0) continue;
            st[i] = *(const float2*)(stats + 2 * (size_t)ro[i]);
            load8<T>(U + (size_t)slot[i] * N + col, u[i]);
        }
#pragma unroll
        for (int i = 0; i < PQ_UNROLL; ++i) {
            if (ro[i] < 0) continue;
            float c[8];
            if (pos[i] < n_pos_lds) {
                const float4 a = pq_c[(pos[i] * 2) * 256 + threadIdx.x], b = pq_c[(pos[i] * 2 + 1) * 256 + threadIdx.x];
                c[0] = a.x; c[1] = a.y; c[2] = a.z; c[3] = a.w; c[4] = b.x; c[5] = b.y; c[6] = b.z; c[7] = b.w;
            } else {
                load8<float>(c_pos + (size_t)pos[i] * N + col, c);
            }
            float v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float a = u[i][e] + c[e];
                const float b = st[i].x * cw[e];
                const float d = a - b;
                v[e] = __builtin_fmaf(st[i].y, d, bq[e]);
                if (LoRange<T>::checked) bad |= out_of_range(v[e], LoRange<T>::limit);
            }
            store8<T>(out + (size_t)ro[i] * ld_out + col, v);
        }
    }
    range_report(range_flag, bad, ZETT_RANGE_BIT_ACTIVATION);
}

// Lever 6 on a caller's table: rows id_slot[id_list[s]] of the folded table (16-bit sums, (mean, rstd)) -> rows s = 0 .. n - 1 of the
// handle's own table; one workgroup per row, 16-byte copies (H % 8 == 0, 16-byte aligned bases)
template <typename T>
__global__ __launch_bounds__(256) void table_gather_kernel(const T* __restrict__ table, const float* __restrict__ stats, const int32_t* __restrict__ id_slot,
                                                           const int32_t* __restrict__ id_list, int n, int H, T* __restrict__ out, float* __restrict__ out_stats) {
    const int s = blockIdx.x;
    if (s >= n) return;
    const int g = id_slot[id_list[s]];
    const uint4* src = (const uint4*)(table + (size_t)g * H);
    uint4* dst = (uint4*)(out + (size_t)s * H);
    for (int c = threadIdx.x; c < H / 8; c += 256) dst[c] = src[c];
    if (threadIdx.x == 0) *(float2*)(out_stats + 2 * (size_t)s) = *(const float2*)(stats + 2 * (size_t)g);
}

// dtype conversion used when weights are uploaded
template <typename T>
__global__ void convert_f32_to_lo_kernel(const float* __restrict__ in, T* __restrict__ out, size_t n, int32_t* __restrict__ range_flag) {
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    bool bad = false;          // range guard: a weight that does not fit the operand type (f16 only), ZETT_RANGE_WEIGHT
    for (; i + 3 < n; i += stride) {
        const float4 v = *(const float4*)(in + i);
        if (LoRange<T>::checked)
            bad |= out_of_range(v.x, LoRange<T>::limit) | out_of_range(v.y, LoRange<T>::limit) | out_of_range(v.z, LoRange<T>::limit) |
                   out_of_range(v.w, LoRange<T>::limit);
        store_lo4<T>(out + i, v);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (size_t j = n & ~(size_t)3; j < n; ++j) { out[j] = to_lo<T>(in[j]); if (LoRange<T>::checked) bad |= out_of_range(in[j], LoRange<T>::limit); }
    }
    range_report(range_flag, bad, ZETT_RANGE_BIT_WEIGHT);
}
template <int SRC_DTYPE>
__global__ void convert_to_f32_kernel(const void* __restrict__ in, float* __restrict__ out, size_t n) {
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        if constexpr (SRC_DTYPE == 1) out[i] = (float)((const _Float16*)in)[i];
        else out[i] = __uint_as_float(((uint32_t)((const uint16_t*)in)[i]) << 16);
    }
}

// ---- zett_forward_into: the destination stores that are not fused into a GEMM epilogue ------------------------------------
// Four fp32 values converted to OT (round to nearest even) in one store: 16 bytes for fp32, 8 for a 16-bit type.
template <typename OT> __device__ __forceinline__ void store4_dst(OT* d, float4 v) {
    if constexpr (std::is_same<OT, float>::value) *(float4*)d = v;
    else *(uint2*)d = make_uint2(pack2_lo<OT>(v.x, v.y), pack2_lo<OT>(v.z, v.w));
}

// The fallback of the destination store (include/zett_hip.h zett_forward_into): fp32 rows staged in the workspace (src, ld_src)
// go to row rows[i] (< 0: skipped; null: i) of the destination, converted to OT.  One workgroup per row; VEC: four values per lane
// and store (cols and both leading dimensions multiples of 4, 16-byte aligned bases), else one.
template <typename OT, bool VEC>
__global__ __launch_bounds__(256) void dest_store_rows_kernel(const float* __restrict__ src, int64_t ld_src, OT* __restrict__ dst, int64_t ld_dst,
                                                              const int64_t* __restrict__ rows, int64_t n_rows, int cols, int32_t* range_flag) {
    bool bad = false;
    for (int64_t i = blockIdx.x; i < n_rows; i += gridDim.x) {
        const int64_t d = rows ? rows[i] : i;
        if (d < 0) continue;
        const float* s = src + i * ld_src;
        OT* o = dst + d * ld_dst;
        if constexpr (VEC) {
            for (int c = (int)threadIdx.x * 4; c < cols; c += 256 * 4) {
                const float4 v = *(const float4*)(s + c);
                store4_dst<OT>(o + c, v);
                bad |= dest_overflow<OT>(v.x) | dest_overflow<OT>(v.y) | dest_overflow<OT>(v.z) | dest_overflow<OT>(v.w);
            }
        } else {
            for (int c = (int)threadIdx.x; c < cols; c += 256) {
                const float v = s[c];
                o[c] = to_lo<OT>(v);
                bad |= dest_overflow<OT>(v);
            }
        }
    }
    range_report(range_flag, bad, ZETT_RANGE_BIT_DEST);
}

// (lever 5 with a caller's row map) out[i] = outer[inner[i]]: the destination row of buffer row i of the position-0 block
static __global__ void compose_rows_kernel(const int64_t* __restrict__ outer, const int64_t* __restrict__ inner, int64_t n, int64_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = outer[inner[i]];
}

// The row map of a destination against its size: err = 1 + (an index i with rows[i] >= n_dest), 0 when every row fits
static __global__ void dest_rows_check_kernel(const int64_t* __restrict__ rows, int64_t n, int64_t n_dest, int32_t* err) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && rows[i] >= n_dest) atomicMax(err, (int)(i < 0x7ffffffe ? i + 1 : 0x7fffffff));
}

}  // namespace zett
