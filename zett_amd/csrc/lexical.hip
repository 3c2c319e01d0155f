// lexical.hip — lexical (FVT / BFVT) embedding transfer on the device (reference scripts/transfer_lexical.py:50-91).
//
// Three stages:
//
//  1. the lexicon (zett_lexical_create): the source tokenizer's bare model as a retokenizer handle WITHOUT special tokens, whose
//     whole-token table (the slot the retokenizer uses for special tokens: same FNV-hashed open-addressing table, load <= 1/8)
//     holds the source tokenizer's full get_vocab() dictionary instead;
//  2. the plan (zett_lexical_plan): the retokenizer's two stages on the NUL-separated target tokens, with the three additions of
//     retok.hip.h's LexPlan — a whole-token hit below R is an exact match, ids >= R are filtered by mode, and the true number of
//     ids kept goes to count[] — then one reduction over count[] (rows set, rows wider than the id matrix, ids in all);
//  3. the rows (zett_lexical_rows_into): a check of ids / row map against their bounds, then one streaming kernel per destination
//     matrix: a lane owns 16 bytes of the source rows' columns (4 fp32 / 8 16-bit values), requests its source rows four at a time, adds them in ids order in fp32,
//     divides once, converts and stores.
//
// THE MEAN: add the rows in `ids` order in fp32, then one IEEE (correctly rounded) division by float(n).  n = 1 is a plain copy.
//
// A translation unit of its own: the kernels and the zett_lexical_* entry points (include/zett_hip.h).  The retokenizer's tables,
// handle and retok_enqueue_call come from retok.hip.h, the typed row loads and destination stores from rowops.hip.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "common.hip.h"
#include "retok.hip.h"
#include "rowops.hip.h"

struct zett_lexical {
    int device = 0;
    zett_retok* rt = nullptr;
    zett::DevBuf words;                  // int64 [0] rows with count > 0, [1] rows with count > width, [2] sum of counts; int32 at [3]: the error words of the rows call
    int64_t* host_pinned = nullptr;      // the same four words on the host
};

namespace zett {

constexpr int LEX_WORDS = 4;

// [0] += rows with count > 0 (transfer_lexical.py:88-91 "Overlapping tokens"), [1] += rows whose ids do not fit `width`, [2] += ids
__global__ __launch_bounds__(256) void lexical_count_kernel(const int32_t* __restrict__ count, int64_t n, int width, unsigned long long* __restrict__ words) {
    __shared__ unsigned long long red[3][4];
    unsigned long long a = 0, b = 0, c = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int v = count[i];
        a += v > 0;
        b += v > width;
        c += (unsigned long long)(v > 0 ? v : 0);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64);
        b += __shfl_down(b, off, 64);
        c += __shfl_down(c, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = a; red[1][wave] = b; red[2][wave] = c; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned long long s = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        if (s) atomicAdd(words + threadIdx.x, s);
    }
}

// The inputs of the rows call against their bounds, nothing trusted: err[0] = 1 + a row with an id outside [0, R) or a destination
// row >= n_dest, err[1] = 1 + a row whose count is negative or exceeds `width` (a row that was not re-planned)
__global__ void lexical_check_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ count, int64_t n_tokens, int width, int64_t n_source_rows,
                                     const int64_t* __restrict__ rows, int64_t n_dest, int32_t* __restrict__ err) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tokens) return;
    const int32_t mark = (int32_t)(i < 0x7ffffffe ? i + 1 : 0x7fffffff);
    const int n = count[i];
    if (n < 0 || n > width) { atomicMax(err + 1, mark); return; }
    bool bad = rows && rows[i] >= n_dest;
    for (int k = 0; k < n; ++k) {
        const int32_t id = ids[i * width + k];
        bad |= id < 0 || id >= n_source_rows;
    }
    if (bad) atomicMax(err, mark);
}

template <int SRC_DTYPE> __device__ __forceinline__ float load_src1(const void* base, size_t e) {
    if constexpr (SRC_DTYPE == 0) return ((const float*)base)[e];
    else if constexpr (SRC_DTYPE == 1) return (float)((const _Float16*)base)[e];
    else return __uint_as_float(((uint32_t)((const uint16_t*)base)[e]) << 16);
}

template <int SRC_DTYPE> struct LexSrc { typedef float type; };
template <> struct LexSrc<1> { typedef f16_t type; };
template <> struct LexSrc<2> { typedef bf16_t type; };
template <int SRC_DTYPE> constexpr int lex_lane_cols() { return SRC_DTYPE == 0 ? 4 : 8; }      // 16 bytes of a source row per lane

// Destination row rows[i] (< 0: skipped; null: i), columns [0, cols): the mean of the count[i] source rows ids[i, :], added in that
// order in fp32 and divided once; count 0: source row fallback_id (< 0: the row is left as it is).  One lane per (row, strip of W
// columns), W = 16 bytes of a source row (4 fp32 / 8 16-bit values) — the work is rows x columns whatever `width` is; the up to
// four source rows of a step are requested before the first is added.  VEC: every access is a vector (16-byte loads; 16- or 2 x
// 16-byte stores, 8-byte for a 16-bit destination of an fp32 source) — the launcher takes it when bases and leading dimensions are
// aligned for it and the width is a multiple of W; otherwise element accesses with a tail on the last strip (a width that is not
// a multiple of W, a destination view at an odd element offset).  Two kernels, not one with a flag: in one body the compiler
// merges the two paths into a dword + dwordx3 pair.
template <int SRC_DTYPE, typename OT, bool VEC>
__global__ __launch_bounds__(256) void lexical_rows_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ count, int64_t n_tokens, int width,
                                                           const void* __restrict__ src, int64_t ld_src, int cols, int64_t fallback_id,
                                                           OT* __restrict__ dst, int64_t ld_dst, const int64_t* __restrict__ rows, int strips) {
    constexpr int W = lex_lane_cols<SRC_DTYPE>();
    typedef typename LexSrc<SRC_DTYPE>::type ST;
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = item / strips;
    if (row >= n_tokens) return;
    const int c0 = (int)(item - row * strips) * W;
    const int64_t d = rows ? rows[row] : row;
    if (d < 0) return;
    const int n = count[row];
    const int32_t* rid = ids + row * width;
    auto load = [&](int64_t r, float (&v)[W]) {
        const size_t e = (size_t)r * (size_t)ld_src + c0;
        if constexpr (VEC && W == 4) {
            const float4 t = load_src4<SRC_DTYPE>(src, e);
            v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
        } else if constexpr (VEC) {
            float t[8];
            load8<ST>((const ST*)src + e, t);
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = t[j];
        } else {
#pragma unroll
            for (int j = 0; j < W; ++j) v[j] = c0 + j < cols ? load_src1<SRC_DTYPE>(src, e + j) : 0.f;
        }
    };
    float acc[W];
    if (n == 0) {
        if (fallback_id < 0) return;
        load(fallback_id, acc);
    } else {
        load(rid[0], acc);
        for (int k0 = 1; k0 < n; k0 += 4) {
            float v[4][W];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k0 + k < n) load(rid[k0 + k], v[k]);
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k0 + k < n) {
#pragma unroll
                    for (int j = 0; j < W; ++j) acc[j] += v[k][j];
                }
        }
        if (n > 1) {
            const float fn = (float)n;
#pragma unroll
            for (int j = 0; j < W; ++j) acc[j] = acc[j] / fn;
        }
    }
    OT* o = dst + d * ld_dst + c0;
    if constexpr (VEC && W == 4) {
        store4_dst<OT>(o, make_float4(acc[0], acc[1], acc[2], acc[3]));
    } else if constexpr (VEC) {
        float t[8];
#pragma unroll
        for (int j = 0; j < W; ++j) t[j] = acc[j];
        store8<OT>(o, t);
    } else {
#pragma unroll
        for (int j = 0; j < W; ++j)
            if (c0 + j < cols) o[j] = to_lo<OT>(acc[j]);
    }
}

template <int SRC_DTYPE, typename OT>
inline void launch_lexical_rows(const int32_t* ids, const int32_t* count, int64_t n_tokens, int width, const void* src, int64_t ld_src, int cols,
                                int64_t fallback_id, void* dst, int64_t ld_dst, const int64_t* rows, hipStream_t st) {
    constexpr int W = lex_lane_cols<SRC_DTYPE>();
    const int strips = (cols + W - 1) / W;
    const size_t src_elem = SRC_DTYPE == 0 ? 4 : 2;
    const size_t dst_align = sizeof(OT) * W < 16 ? sizeof(OT) * W : 16;
    const bool vec = cols % W == 0 && (uintptr_t)src % 16 == 0 && ((size_t)ld_src * src_elem) % 16 == 0 && (uintptr_t)dst % dst_align == 0 &&
                     ((size_t)ld_dst * sizeof(OT)) % dst_align == 0;
    const int64_t items = n_tokens * strips;
    const dim3 grid((unsigned)((items + 255) / 256));
    if (vec)
        hipLaunchKernelGGL((lexical_rows_kernel<SRC_DTYPE, OT, true>), grid, dim3(256), 0, st, ids, count, n_tokens, width, src, ld_src, cols, fallback_id,
                           (OT*)dst, ld_dst, rows, strips);
    else
        hipLaunchKernelGGL((lexical_rows_kernel<SRC_DTYPE, OT, false>), grid, dim3(256), 0, st, ids, count, n_tokens, width, src, ld_src, cols, fallback_id,
                           (OT*)dst, ld_dst, rows, strips);
}

}  // namespace zett

extern "C" {

int zett_lexical_create(const zett_retok_model* model, int32_t n_vocab, const uint8_t* vocab_bytes, const int32_t* vocab_offsets,
                        const int32_t* vocab_ids, int device, zett_lexical** out) {
    using namespace zett;
    if (!model || !out) return fail(ZETT_E_INVALID, "null argument");
    if (n_vocab < 0 || (n_vocab && (!vocab_bytes || !vocab_offsets || !vocab_ids))) return fail(ZETT_E_INVALID, "vocabulary arrays missing");
    zett_retok_model m = *model;      // the bare model: its own special tokens are NOT matched (transfer_lexical.py:77 calls model.tokenize on every string)
    m.n_special = n_vocab;
    m.special_bytes = vocab_bytes;
    m.special_offsets = vocab_offsets;
    m.special_ids = vocab_ids;
    zett_retok* rt = nullptr;
    if (int rc = zett_retok_create(&m, device, &rt)) return rc;
    auto* h = new zett_lexical();
    h->device = device;
    h->rt = rt;
    ::zett::DeviceScope scope(device);
    if (h->words.reserve(LEX_WORDS * 8) || hipHostMalloc((void**)&h->host_pinned, LEX_WORDS * 8, hipHostMallocDefault) != hipSuccess) {
        zett_retok_destroy(rt);
        h->words.release();
        delete h;
        return fail(ZETT_E_HIP, "zett_lexical_create: allocation failed");
    }
    *out = h;
    return 0;
}

int zett_lexical_destroy(zett_lexical* h) {
    if (!h) return 0;
    zett_retok_destroy(h->rt);
    ::zett::DeviceScope scope(h->device);
    h->words.release();
    if (h->host_pinned) (void)hipHostFree(h->host_pinned);
    delete h;
    return 0;
}

int zett_lexical_plan(zett_lexical* h, const uint8_t* token_chars, int64_t n_tokens, int64_t n_text, int64_t n_source_rows, int32_t fvt_mode,
                      int32_t width, int32_t* ids, int32_t* count, int64_t* n_overlap, int64_t* n_wide, int64_t* n_ids, int64_t* bad_token,
                      void* stream) {
    using namespace zett;
    if (!h) return fail(ZETT_E_INVALID, "null handle");
    if (n_overlap) *n_overlap = 0;
    if (n_wide) *n_wide = 0;
    if (n_ids) *n_ids = 0;
    if (bad_token) *bad_token = -1;
    if (n_tokens < 0 || width < 1 || n_source_rows < 0) return fail(ZETT_E_INVALID, "bad shape");
    if (fvt_mode < ZETT_LEXICAL_NO || fvt_mode > ZETT_LEXICAL_BFVT) return fail(ZETT_E_INVALID, "fvt_mode %d: 0 (no), 1 (fvt), 2 (bfvt)", fvt_mode);
    if (n_tokens == 0) return 0;
    if (!ids || !count) return fail(ZETT_E_INVALID, "null argument");
    ZETT_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (h->rt->calls) {                  // results of earlier asynchronous calls nobody asked for: dropped
        int64_t t, c, b;
        (void)zett_retok_result(h->rt, &t, &c, &b);
    }
    HIP_TRY(hipMemsetAsync(count, 0, (size_t)n_tokens * 4, st));
    HIP_TRY(hipMemsetAsync(h->words.p, 0, LEX_WORDS * 8, st));
    const LexPlan lex{count, (int32_t)std::min<int64_t>(n_source_rows, 0x7fffffff), fvt_mode};
    if (int rc = retok_enqueue_call(h->rt, token_chars, nullptr, n_tokens, n_text, width, -1, ids, stream, lex)) return rc;
    hipLaunchKernelGGL(lexical_count_kernel, dim3((unsigned)std::min<int64_t>((n_tokens + 255) / 256, 1024)), dim3(256), 0, st, count, n_tokens, (int)width,
                       h->words.as<unsigned long long>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->host_pinned, h->words.p, LEX_WORDS * 8, hipMemcpyDeviceToHost, st));
    int64_t n_trunc = 0;
    if (int rc = zett_retok_result(h->rt, &n_trunc, nullptr, bad_token)) { (void)hipStreamSynchronize(st); return rc; }
    HIP_TRY(hipStreamSynchronize(st));
    if (n_overlap) *n_overlap = h->host_pinned[0];
    if (n_wide) *n_wide = h->host_pinned[1];
    if (n_ids) *n_ids = h->host_pinned[2];
    return 0;
}

int zett_lexical_rows_into(zett_lexical* h, const int32_t* ids, const int32_t* count, int64_t n_tokens, int32_t width, const void* src_in,
                           int64_t ld_src_in, const void* src_out, int64_t ld_src_out, int32_t src_dtype, int64_t n_source_rows, int32_t n_embd,
                           int64_t fallback_id, const zett_dest* dest, void* stream) {
    using namespace zett;
    if (!h || !dest) return fail(ZETT_E_INVALID, "null argument");
    if (n_tokens < 0 || width < 1 || n_source_rows < 0 || n_embd < 1) return fail(ZETT_E_INVALID, "bad shape");
    if (!is_dtype(src_dtype)) return fail(ZETT_E_INVALID, "unknown source dtype %d", src_dtype);
    if (!is_dtype(dest->dtype)) return fail(ZETT_E_INVALID, "unknown destination dtype %d", dest->dtype);
    if (dest->bias) return fail(ZETT_E_INVALID, "zett_dest.bias must be NULL: the lexical transfer has no bias");
    if (!src_in || !dest->in) return fail(ZETT_E_INVALID, "null source or destination matrix");
    if ((src_out == nullptr) != (dest->out == nullptr)) return fail(ZETT_E_INVALID, "source and destination must both have, or both lack, the output-embedding matrix");
    if (ld_src_in < n_embd || dest->ld_in < n_embd || (src_out && (ld_src_out < n_embd || dest->ld_out < n_embd)))
        return fail(ZETT_E_INVALID, "a leading dimension is smaller than n_embd = %d", n_embd);
    if (dest->n_dest_rows < 0 || (!dest->rows && dest->n_dest_rows < n_tokens))
        return fail(ZETT_E_INVALID, "identity row map: the destination has %lld rows, the plan %lld", (long long)dest->n_dest_rows, (long long)n_tokens);
    if (fallback_id < -1) return fail(ZETT_E_INVALID, "fallback id %lld: a source row, or -1 to leave rows without constituents untouched", (long long)fallback_id);
    if (fallback_id >= n_source_rows) return fail(ZETT_E_INDEX, "fallback id %lld outside the %lld source rows", (long long)fallback_id, (long long)n_source_rows);
    if (n_tokens == 0) return 0;
    if (!ids || !count) return fail(ZETT_E_INVALID, "null argument");
    if (n_tokens * (int64_t)((n_embd + 3) / 4) >= ((int64_t)1 << 39)) return fail(ZETT_E_INVALID, "too many rows x columns for one call");
    ZETT_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    int32_t* err = (int32_t*)(h->words.as<int64_t>() + 3);
    HIP_TRY(hipMemsetAsync(err, 0, 8, st));
    hipLaunchKernelGGL(lexical_check_kernel, dim3((unsigned)((n_tokens + 255) / 256)), dim3(256), 0, st, ids, count, n_tokens, (int)width, n_source_rows,
                       dest->rows, dest->n_dest_rows, err);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->host_pinned + 3, err, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int32_t* he = (const int32_t*)(h->host_pinned + 3);
    if (he[1]) return fail(ZETT_E_INVALID, "row %d: its count is negative or exceeds width = %d (plan it again at the width it needs)", he[1] - 1, width);
    if (he[0]) return fail(ZETT_E_INDEX, "row %d: a source id outside [0, %lld) or a destination row outside [0, %lld)", he[0] - 1, (long long)n_source_rows,
                           (long long)dest->n_dest_rows);
    for (int part = 0; part < (src_out ? 2 : 1); ++part) {
        const void* src = part ? src_out : src_in;
        const int64_t ld_src = part ? ld_src_out : ld_src_in;
        void* dst = part ? dest->out : dest->in;
        const int64_t ld_dst = part ? dest->ld_out : dest->ld_in;
        with_dtype(src_dtype, [&](auto sd) {
            with_dtype(dest->dtype, [&](auto dd) {
                launch_lexical_rows<decltype(sd)::value, elem_t<decltype(dd)::value>>(ids, count, n_tokens, width, src, ld_src, n_embd, fallback_id, dst, ld_dst,
                                                                                      dest->rows, st);
            });
        });
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
