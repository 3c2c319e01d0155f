// train_batch.hip — the batch's sub-vocabulary (include/zett_hip.h, "the batch's sub-vocabulary"; collator.py:207-282 of the
// reference): which ids occur in the batch, the list of N ids to embed (specials, positives ascending, negatives, the specials moved to
// their own row), the inverse table, the remapped ids and the gathered rows of the surface forms and priors.
//
// Integers only.  Presence flags over V are set with an integer OR; the positives' ranks and the ranks of the absent ids in
// negative_order's order come from ONE multi-workgroup scan in three launches (count per segment of 1024 ids, one workgroup over the
// segment counts, place: the shape of scan.hip.h's compaction, here with two predicates in one pass and a payload) — every wave owns a
// contiguous segment, so no launch waits for another workgroup; the inverse table is written
// with an integer max.  OR and max do not depend on arrival order: the same inputs give the same bits.  An id outside [0, V) is
// reported in the status word and never becomes an address.
//
// Two more pieces of the collator live here.  zett_op_label_batch (collator.py:180-205): one streaming pass over the positions writes
// the MLM (or CLM) labels, the masked ids, byte_lengths and integer counts per workgroup; a one-workgroup finalize adds the counts in
// workgroup order and forms the two metrics as quotients of exact integers.  zett_op_pad_vocabulary (collator.py:283-337): one launch
// that copies the vocabulary's rows and fills the rows behind them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "scan.hip.h"
#include "train_common.hip.h"

using namespace zett;

namespace {

constexpr int kListMax = ZETT_SPLICE_MAX_ROWS;
constexpr int kPerLane = kSeg / 64;                   // ids of a lane in its wave's segment (count and place each read them: two launches)
constexpr int kMaxGrid = 1 << 16;
constexpr int kMaxL = 65536;                          // columns of a surface-form row: the copy's indices are 32-bit

struct SpecialList {
    int32_t n;
    int32_t n_low;                  // the first n_low moves insert below the last row; the others (special ids >= N - 1, the end of the ascending order) at N - 1
    int32_t hi_low;                 // the last row any of the first n_low moves touches: rows beyond it are not moved by them
    int32_t tail_lo;                // the first row any of the other moves touches
    int32_t id[kListMax];           // the special ids in the tokenizer's order (the prefix of the pre-list)
    int32_t from[kListMax];         // move m (ascending special id): the row it is taken from ...
    int32_t to[kListMax];           // ... and the row it is inserted at
};
static_assert(sizeof(SpecialList) < 4096 - 256, "the lists must fit the kernel-argument limit");

// workspace, in int32 words
struct Layout {
    int64_t flags, inv, pos, neg, segcnt, segoff, totals, words;
    int64_t nseg;
};
Layout layout(int64_t v, int64_t n) {
    Layout L{};
    L.nseg = compact_segments(v);
    int64_t w = 0;
    L.flags = w; w += v;                   // bit 0: the id occurs in input_ids / labels; bit 1: it is special
    L.inv = w; w += v;                     // id -> its last row of ids_to_embed, -1: none
    L.pos = w; w += n;                     // the positives, ascending
    L.neg = w; w += n;                     // the absent ids in negative_order's order
    L.segcnt = w; w += 2 * L.nseg;         // per segment: positives, absent ids
    L.segoff = w; w += 2 * L.nseg;         // their exclusive scans
    L.totals = w; w += 4;                  // positives, absent ids
    L.words = w;
    return L;
}

__device__ __forceinline__ void store_id(void* out, int wide, int64_t i, int64_t x) {
    if (wide) ((int64_t*)out)[i] = x;
    else ((int32_t*)out)[i] = (int32_t)x;
}

__global__ __launch_bounds__(256) void batch_init_kernel(int* __restrict__ flags, int* __restrict__ inv, int64_t v, int* __restrict__ status) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < v; i += (int64_t)gridDim.x * 256) {
        flags[i] = 0;
        inv[i] = -1;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *status = 0;
}

// a set bit is not set again: most positions of a batch hold an id some earlier position held
__device__ __forceinline__ void mark(int* flags, int64_t id, int bit) {
    if (!(__hip_atomic_load(flags + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(flags + id, bit);
}

__global__ __launch_bounds__(256) void batch_mark_kernel(const void* __restrict__ ids, int ids64, const void* __restrict__ labels, int labels64, int64_t t, int64_t v,
                                                         int* __restrict__ flags, int* __restrict__ status, const SpecialList sp) {
    if (blockIdx.x == 0)
        for (int i = threadIdx.x; i < sp.n; i += 256) mark(flags, sp.id[i], 2);
    int bad = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < t; p += (int64_t)gridDim.x * 256) {
        const int64_t a = load_id(ids, ids64, p), b = load_id(labels, labels64, p);
        if (a >= 0 && a < v) mark(flags, a, 1);
        else bad = 1;
        if (b != -100) {
            if (b >= 0 && b < v) mark(flags, b, 1);
            else bad = 1;
        }
    }
    if (bad) atomicOr(status, ZETT_BATCH_BAD_ID);
}

// The two predicates of a wave's segment, 16 ids per lane (id = seg * 1024 + j * 64 + lane): bit j of `positive` — the id occurs and
// is not special; bit j of `absent` — entry `id` of negative_order is an id of [0, v) that is neither in the batch nor special.
__device__ __forceinline__ void segment_bits(const int* __restrict__ flags, const void* __restrict__ order, int order64, int64_t v, int64_t seg, int lane, int random,
                                             uint32_t& positive, uint32_t& absent, int32_t (&entry)[kPerLane], int& bad) {
    positive = absent = 0;
#pragma unroll
    for (int j = 0; j < kPerLane; ++j) {
        const int64_t i = seg * kSeg + j * 64 + lane;
        entry[j] = 0;
        if (i >= v) continue;
        positive |= (uint32_t)(flags[i] == 1) << j;
        if (random) {
            const int64_t o = load_id(order, order64, i);
            if (o >= 0 && o < v) {
                entry[j] = (int32_t)o;
                absent |= (uint32_t)(flags[o] == 0) << j;
            } else {
                bad = 1;
            }
        }
    }
}

__global__ __launch_bounds__(256) void batch_count_kernel(const int* __restrict__ flags, const void* __restrict__ order, int order64, int64_t v, int64_t nseg, int random,
                                                          int* __restrict__ segcnt, int* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    int bad = 0;
    for (int64_t seg = (int64_t)blockIdx.x * 4 + wave_index(); seg < nseg; seg += (int64_t)gridDim.x * 4) {
        uint32_t positive, absent;
        int32_t entry[kPerLane];
        segment_bits(flags, order, order64, v, seg, lane, random, positive, absent, entry, bad);
        int a = __popc(positive), b = __popc(absent);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_xor(a, off, 64);
            b += __shfl_xor(b, off, 64);
        }
        if (lane == 0) {
            segcnt[seg] = a;
            segcnt[nseg + seg] = b;
        }
    }
    if (bad) atomicOr(status, ZETT_BATCH_BAD_ORDER);
}

// exclusive scans of the two rows of segment counts: one workgroup, 1024 segments (2^20 ids) per round, the carry in registers
__global__ __launch_bounds__(1024) void batch_scan_kernel(const int* __restrict__ segcnt, int64_t nseg, int* __restrict__ segoff, int* __restrict__ totals, int64_t n,
                                                          int n_special, int random, int* __restrict__ n_positive, int* __restrict__ status) {
    __shared__ int s_waves0[16], s_waves1[16];
    const int tid = threadIdx.x;
    int carry0 = 0, carry1 = 0;
    for (int64_t base = 0; base < nseg; base += 1024) {
        const int64_t i = base + tid;
        const int a = i < nseg ? segcnt[i] : 0, b = i < nseg ? segcnt[nseg + i] : 0;
        int round0, round1;
        const int before0 = block_exclusive_scan<1024>(a, s_waves0, &round0), before1 = block_exclusive_scan<1024>(b, s_waves1, &round1);
        if (i < nseg) {
            segoff[i] = carry0 + before0;
            segoff[nseg + i] = carry1 + before1;
        }
        carry0 += round0;
        carry1 += round1;
    }
    if (tid == 0) {
        totals[0] = carry0;
        totals[1] = carry1;
        const int64_t np = (int64_t)n_special + carry0;
        *n_positive = (int)np;
        if (np > n) atomicOr(status, ZETT_BATCH_OVERFLOW);
        else if (random && carry1 < n - np) atomicOr(status, ZETT_BATCH_REPEAT);          // fewer absent entries than absent ids: not a permutation
    }
}

__global__ __launch_bounds__(256) void batch_place_kernel(const int* __restrict__ flags, const void* __restrict__ order, int order64, int64_t v, int64_t nseg, int random,
                                                          const int* __restrict__ segoff, int64_t n, int* __restrict__ pos, int* __restrict__ neg) {
    const int lane = threadIdx.x & 63;
    int bad = 0;
    for (int64_t seg = (int64_t)blockIdx.x * 4 + wave_index(); seg < nseg; seg += (int64_t)gridDim.x * 4) {
        uint32_t positive, absent;
        int32_t entry[kPerLane];
        segment_bits(flags, order, order64, v, seg, lane, random, positive, absent, entry, bad);
        int64_t at0 = segoff[seg], at1 = segoff[nseg + seg];
#pragma unroll
        for (int j = 0; j < kPerLane; ++j) {
            const bool p = (positive >> j) & 1, a = (absent >> j) & 1;
            const uint64_t mp = __ballot(p), ma = __ballot(a);
            const int64_t r0 = at0 + lanes_below(mp), r1 = at1 + lanes_below(ma);
            if (p && r0 < n) pos[r0] = (int)(seg * kSeg + j * 64 + lane);
            if (a && r1 < n) neg[r1] = entry[j];
            at0 += __popcll(mp);
            at1 += __popcll(ma);
        }
    }
}

// the row, before the move (from -> to: Python's del / insert), of what sits in row q after it
__device__ __forceinline__ int64_t undo_move(int64_t q, int64_t from, int64_t to) {
    if (q == to) return from;
    q -= q > to ? 1 : 0;
    return q + (q >= from ? 1 : 0);
}

// The rows.  A wave takes 64 final rows: a lane undoes the specials' moves (last move first) to find its row of the pre-list
// [specials | positives | negatives], reads the id there, writes ids_to_embed, the prior, the mask and inv (integer max: the LAST row
// of an id wins); then the wave copies the 64 surface-form rows with consecutive lanes on consecutive bytes of the output.
// TV: the unit of the copy — uint4 (16 bytes, where the row bytes, the leading dimension and the pointers allow), or one element.
template <typename TV>
__global__ __launch_bounds__(256) void batch_rows_kernel(int64_t n, int64_t v, int random, const int* __restrict__ totals, const int* __restrict__ pos,
                                                         const int* __restrict__ neg, const char* __restrict__ sf, int64_t ld_bytes, int units, const float* __restrict__ priors,
                                                         void* __restrict__ ids_to_embed, int wide, TV* __restrict__ sf_out, float* __restrict__ priors_out,
                                                         uint8_t* __restrict__ mask, int* __restrict__ inv, int* __restrict__ status, const SpecialList sp) {
    const int lane = threadIdx.x & 63;
    const int64_t n_positive = std::min<int64_t>((int64_t)sp.n + totals[0], n);
    const int64_t n_absent = totals[1];
    const int64_t n_tiles = (n + 63) / 64;
    int repeat = 0;
    for (int64_t tile = (int64_t)blockIdx.x * 4 + wave_index(); tile < n_tiles; tile += (int64_t)gridDim.x * 4) {
        const int64_t r = tile * 64 + lane;
        int id = 0;
        if (r < n) {
            int64_t q = r;
            // a move touches the rows between its two ends only: a special id at the end of the vocabulary shifts every row behind its
            // source by one, but no row has to walk the moves that end below it
            if (r >= sp.tail_lo)
                for (int m = sp.n - 1; m >= sp.n_low; --m) q = undo_move(q, sp.from[m], sp.to[m]);
            if (q <= sp.hi_low)
                for (int m = sp.n_low - 1; m >= 0; --m) q = undo_move(q, sp.from[m], sp.to[m]);
            bool filler = false;
            if (q < sp.n) {
                id = sp.id[q];
            } else if (q < n_positive) {
                id = pos[q - sp.n];
            } else {
                const int64_t k = q - n_positive;
                filler = !random;
                id = (random && k < n_absent) ? neg[k] : 0;
            }
            store_id(ids_to_embed, wide, r, id);
            priors_out[r] = priors[id];
            mask[r] = 1;
            // positives_only: the negatives are all id 0, and only the highest of their rows in this wave can be the last one
            const uint64_t fill = __ballot(filler);
            if (!filler || lane == 63 - __clzll((unsigned long long)fill)) {
                const int old = atomicMax(inv + id, (int)r);
                if (random && old >= 0) repeat = 1;
            }
        }
        const int64_t row0 = tile * 64;
        const int rows_here = (int)std::min<int64_t>(64, n - row0);
        for (int e0 = 0; e0 < rows_here * units; e0 += 64) {          // (every lane takes part in the exchange: a lane that is switched off hands out 0)
            const int e = e0 + lane, rr = std::min(e / units, 63), c = e - rr * units;
            const int src = __shfl(id, rr, 64);
            if (e < rows_here * units) sf_out[(row0 + rr) * units + c] = *(const TV*)(sf + (int64_t)src * ld_bytes + (int64_t)c * sizeof(TV));
        }
    }
    if (repeat) atomicOr(status, ZETT_BATCH_REPEAT);
}

__global__ __launch_bounds__(256) void batch_remap_kernel(const void* __restrict__ ids, int ids64, const void* __restrict__ labels, int labels64, int64_t t, int64_t v,
                                                          const int* __restrict__ inv, void* __restrict__ ids_out, void* __restrict__ labels_out) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < t; p += (int64_t)gridDim.x * 256) {
        const int64_t a = load_id(ids, ids64, p), b = load_id(labels, labels64, p);
        store_id(ids_out, ids64, p, (a >= 0 && a < v) ? std::max(inv[a], 0) : 0);
        store_id(labels_out, labels64, p, b == -100 ? -100 : ((b >= 0 && b < v) ? std::max(inv[b], 0) : 0));
    }
}

bool width_ok(int32_t b) { return b == 4 || b == 8; }

int shape_args(int64_t t, int64_t v, int64_t n) {
    if (t < 0 || v <= 0 || n <= 0) return fail(ZETT_E_INVALID, "the batch vocabulary needs t >= 0 positions, v > 0 ids and n > 0 rows (t = %lld, v = %lld, n = %lld)", (long long)t, (long long)v, (long long)n);
    if (t > 0x7fffff00LL || v > 0x7fffff00LL) return fail(ZETT_E_INVALID, "positions and ids are indexed with 32 bits (t = %lld, v = %lld)", (long long)t, (long long)v);
    if (n > v) return fail(ZETT_E_INVALID, "n = %lld rows cannot be filled from v = %lld ids", (long long)n, (long long)v);
    return 0;
}

// ---- labels, byte lengths and metrics of a batch (include/zett_hip.h, "labelling a batch"; collator.py:180-205) ----------------------
constexpr int kLabelGrid = ZETT_LABEL_WORKSPACE_BYTES / 64;          // workgroups of the labelling pass: one row of 8 int64 partials each

struct LabelSpecials {
    int32_t n;
    int32_t id[kListMax];
};
static_assert(kLabelGrid == 256, "label_finalize_kernel has one thread per workgroup of the labelling pass");
static_assert(sizeof(LabelSpecials) < 4096 - 256, "the list must fit the kernel-argument limit");

struct LabelKeys { uint64_t key[4]; uint64_t t_mask, t_replace, t_random; };

__device__ __forceinline__ bool is_special(const LabelSpecials& sp, int64_t id) {
    bool hit = false;
    for (int i = 0; i < sp.n; ++i) hit |= id == sp.id[i];
    return hit;
}

__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One pass over the T = b * s positions.  A thread takes positions p, p + grid * 256, ...; p is the LOGICAL index (row * s + column),
// the addresses use the leading dimensions.  Every count is an integer: lanes, then the four waves (LDS, fixed order), then one row of
// partials per workgroup, which label_finalize_kernel adds in workgroup order.
__global__ __launch_bounds__(256) void label_batch_kernel(const void* ids, int wide, int64_t ld_in, int64_t t, int s, int64_t v, const void* __restrict__ table,
                                                          int table64, int64_t vocab_len, int64_t mask_id, int64_t unk_id, int mlm, const LabelKeys k, void* ids_out,
                                                          int64_t ld_out, void* __restrict__ labels, int64_t* __restrict__ byte_lengths, int64_t* __restrict__ partials,
                                                          const LabelSpecials sp) {
    __shared__ int64_t s_red[4][8];
    int64_t c[8] = {0, 0, 0, 0, 0, 0, 0, 0};          // -, non-special, their bytes, unk, masked, replaced, random, bad
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < t; p += (int64_t)gridDim.x * 256) {
        const int64_t row = (uint32_t)p / (uint32_t)s, col = p - row * s;          // (t < 2^31)
        const int64_t id = load_id(ids, wide, row * ld_in + col);          // (ids_out may be ids: a position is read, then written, by one thread)
        const bool ok = id >= 0 && id < v;
        int64_t out = id, label = id;
        if (mlm) {
            const bool masked = ok && !is_special(sp, id) && (mix64(k.key[0] ^ (uint64_t)p) >> 11) < k.t_mask;
            label = masked ? id : -100;
            if (masked) {
                const bool replaced = (mix64(k.key[1] ^ (uint64_t)p) >> 11) < k.t_replace;
                const bool random = !replaced && (mix64(k.key[2] ^ (uint64_t)p) >> 11) < k.t_random;
                if (replaced) out = mask_id;
                if (random) out = (int64_t)(mix64(k.key[3] ^ (uint64_t)p) % (uint64_t)vocab_len);
                c[4] += 1;
                c[5] += replaced;
                c[6] += random;
            }
        }
        const int64_t bytes = ok ? load_id(table, table64, out) : 0;          // (a replaced id is mask_id or below vocab_len: both inside the table)
        const bool plain = !is_special(sp, out);
        c[1] += plain;
        c[2] += plain ? bytes : 0;
        c[3] += unk_id >= 0 && out == unk_id;
        c[7] |= !ok;
        store_id(ids_out, wide, row * ld_out + col, out);
        store_id(labels, wide, p, label);
        byte_lengths[p] = bytes;
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        const int64_t w = wave_sum_i64(c[i]);
        if (lane == 0) s_red[wave][i] = w;
    }
    __syncthreads();
    if (threadIdx.x >= 1 && threadIdx.x < 8) partials[(int64_t)blockIdx.x * 8 + threadIdx.x] = s_red[0][threadIdx.x] + s_red[1][threadIdx.x] + s_red[2][threadIdx.x] + s_red[3][threadIdx.x];
}

// the record and the two quotients: thread g takes the partials of workgroup g (at most kLabelGrid = 256 of them); lanes, then waves
__global__ __launch_bounds__(256) void label_finalize_kernel(const int64_t* __restrict__ partials, int n_groups, int64_t t, int64_t* __restrict__ record, double* __restrict__ metrics) {
    __shared__ int64_t s_red[4][8];
    __shared__ int64_t s_sum[8];
    const int g = threadIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 1; i < 8; ++i) {
        const int64_t w = wave_sum_i64(g < n_groups ? partials[(int64_t)g * 8 + i] : 0);
        if (lane == 0) s_red[wave][i] = w;
    }
    __syncthreads();
    if (g < 8) {
        int64_t sum = g ? s_red[0][g] + s_red[1][g] + s_red[2][g] + s_red[3][g] : t;
        if (g == 7) sum = sum ? ZETT_LABEL_BAD_ID : 0;
        record[g] = sum;
        s_sum[g] = sum;
    }
    __syncthreads();
    if (g == 0) {
        metrics[0] = (double)s_sum[2] / (double)s_sum[1];          // 0 / 0: NaN, numpy's mean of nothing
        metrics[1] = (double)s_sum[3] / (double)t;
    }
}

// ---- the padded vocabulary (collator.py:283-337) ------------------------------------------------------------------------------------------
template <typename TE, typename TP>
__global__ __launch_bounds__(256) void pad_vocab_kernel(const TE* __restrict__ sf, int64_t ld, int l, int64_t v, int64_t r, const TP* __restrict__ priors, TE* __restrict__ sf_out,
                                                        float* __restrict__ priors_out, uint8_t* __restrict__ mask, int64_t* __restrict__ ids_to_embed) {
    const int64_t total = r * l;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int64_t row = e / l;
        const int col = (int)(e - row * l);
        const bool live = row < v;
        sf_out[e] = live ? sf[row * ld + col] : (TE)0;
        if (col == 0) {
            priors_out[row] = live ? (float)priors[row] : -100000.0f;          // (a float64 prior is rounded once, to nearest even)
            mask[row] = live;
            ids_to_embed[row] = live ? row : 0;
        }
    }
}

}  // namespace

extern "C" {

int zett_op_batch_vocab_workspace_bytes(int64_t t, int64_t v, int64_t n, int64_t* bytes) {
    if (int rc = shape_args(t, v, n)) return rc;
    if (!bytes) return fail(ZETT_E_INVALID, "null argument");
    *bytes = layout(v, n).words * 4;
    return 0;
}

int zett_op_batch_vocab(const void* input_ids, int32_t ids_bytes, const void* labels, int32_t labels_bytes, int64_t t, int64_t v, int64_t n, const void* surface_forms,
                        int32_t sf_bytes, int64_t ld_sf, int32_t l, const float* priors, const void* negative_order, int32_t order_bytes, int32_t mode,
                        const int32_t* special_ids, const int32_t* move_from, const int32_t* move_to, int32_t n_special, void* out_input_ids, void* out_labels,
                        void* ids_to_embed, void* out_surface_forms, float* out_priors, uint8_t* mask, int32_t* n_positive, int32_t* status, void* workspace,
                        int64_t workspace_bytes, void* stream) {
    if (int rc = shape_args(t, v, n)) return rc;
    if (mode != ZETT_BATCH_POSITIVES_ONLY && mode != ZETT_BATCH_RANDOM) return fail(ZETT_E_INVALID, "unknown mode %d", (int)mode);
    const int random = mode == ZETT_BATCH_RANDOM;
    if (!width_ok(ids_bytes) || !width_ok(labels_bytes) || !width_ok(sf_bytes) || (random && !width_ok(order_bytes)))
        return fail(ZETT_E_INVALID, "ids, labels, surface forms and negative_order must be int32 or int64");
    if ((t && (!input_ids || !labels || !out_input_ids || !out_labels)) || !surface_forms || !priors || !ids_to_embed || !out_surface_forms || !out_priors || !mask ||
        !n_positive || !status || (random && !negative_order))
        return fail(ZETT_E_INVALID, "null argument");
    if (l <= 0 || l > kMaxL || ld_sf < l)
        return fail(ZETT_E_INVALID, "surface forms need 0 < l <= %d columns and ld_sf >= l (l = %d, ld_sf = %lld)", kMaxL, (int)l, (long long)ld_sf);
    if (n_special < 0 || n_special > kListMax) return fail(ZETT_E_INVALID, "%d special ids are listed, at most %d travel with a launch", (int)n_special, kListMax);
    if (n_special > n) return fail(ZETT_E_INVALID, "%d special ids do not fit n = %lld rows", (int)n_special, (long long)n);
    if (n_special && (!special_ids || !move_from || !move_to)) return fail(ZETT_E_INVALID, "null argument");
    SpecialList sp{};
    sp.n = n_special;
    sp.n_low = 0;
    sp.hi_low = -1;
    sp.tail_lo = (int32_t)std::min<int64_t>(n, 0x7fffffff);
    for (int i = 0; i < n_special; ++i) {
        if (special_ids[i] < 0 || special_ids[i] >= v) return fail(ZETT_E_INDEX, "special id %d is outside [0, %lld)", (int)special_ids[i], (long long)v);
        if (move_from[i] < 0 || move_from[i] >= n || move_to[i] < 0 || move_to[i] >= n)
            return fail(ZETT_E_INDEX, "move %d (%d -> %d) leaves the %lld rows", i, (int)move_from[i], (int)move_to[i], (long long)n);
        sp.id[i] = special_ids[i];
        sp.from[i] = move_from[i];
        sp.to[i] = move_to[i];
        if (move_to[i] < n - 1 && sp.n_low == i) {
            sp.n_low = i + 1;
            sp.hi_low = std::max(sp.hi_low, std::max(move_from[i], move_to[i]));
        } else {
            sp.tail_lo = std::min(sp.tail_lo, std::min(move_from[i], move_to[i]));
        }
    }
    for (int i = 0; i < n_special; ++i)          // (at most 256 ids: no allocation for a sort)
        for (int j = 0; j < i; ++j)
            if (sp.id[i] == sp.id[j]) return fail(ZETT_E_INVALID, "a special id is listed twice");
    const Layout L = layout(v, n);
    if (!workspace || !aligned(workspace, 4)) return fail(ZETT_E_INVALID, "null or misaligned workspace");
    if (workspace_bytes < L.words * 4) return fail(ZETT_E_INVALID, "the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes, (long long)(L.words * 4));

    hipStream_t st = (hipStream_t)stream;
    int* w = (int*)workspace;
    const int ids64 = ids_bytes == 8, labels64 = labels_bytes == 8, order64 = order_bytes == 8;
    hipLaunchKernelGGL(batch_init_kernel, dim3(grid_for((v + 255) / 256, kMaxGrid)), dim3(256), 0, st, w + L.flags, w + L.inv, v, status);
    hipLaunchKernelGGL(batch_mark_kernel, dim3(grid_for((t + 255) / 256, kMaxGrid)), dim3(256), 0, st, input_ids, ids64, labels, labels64, t, v, w + L.flags, status, sp);
    const int seg_grid = grid_for((L.nseg + 3) / 4, kMaxGrid);
    hipLaunchKernelGGL(batch_count_kernel, dim3(seg_grid), dim3(256), 0, st, (const int*)(w + L.flags), negative_order, order64, v, L.nseg, random, w + L.segcnt, status);
    hipLaunchKernelGGL(batch_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)(w + L.segcnt), L.nseg, w + L.segoff, w + L.totals, n, (int)n_special, random, n_positive,
                       status);
    hipLaunchKernelGGL(batch_place_kernel, dim3(seg_grid), dim3(256), 0, st, (const int*)(w + L.flags), negative_order, order64, v, L.nseg, random,
                       (const int*)(w + L.segoff), n, w + L.pos, w + L.neg);
    const int64_t row_bytes = (int64_t)l * sf_bytes, ld_bytes = ld_sf * sf_bytes;
    const int rows_grid = grid_for(((n + 63) / 64 + 3) / 4, kMaxGrid);
    const bool vec = row_bytes % 16 == 0 && ld_bytes % 16 == 0 && aligned(surface_forms, 16) && aligned(out_surface_forms, 16);
#define ZETT_ROWS(TV)                                                                                                                                                   \
    hipLaunchKernelGGL(batch_rows_kernel<TV>, dim3(rows_grid), dim3(256), 0, st, n, v, random, (const int*)(w + L.totals), (const int*)(w + L.pos), (const int*)(w + L.neg), \
                       (const char*)surface_forms, ld_bytes, (int)(row_bytes / (int64_t)sizeof(TV)), priors, ids_to_embed, ids64, (TV*)out_surface_forms, out_priors, mask,  \
                       w + L.inv, status, sp)
    if (vec) ZETT_ROWS(uint4);
    else if (sf_bytes == 8) ZETT_ROWS(uint64_t);
    else ZETT_ROWS(uint32_t);
#undef ZETT_ROWS
    if (t) hipLaunchKernelGGL(batch_remap_kernel, dim3(grid_for((t + 255) / 256, kMaxGrid)), dim3(256), 0, st, input_ids, ids64, labels, labels64, t, v, (const int*)(w + L.inv),
                              out_input_ids, out_labels);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_label_batch(const void* input_ids, int32_t ids_bytes, int64_t ld_in, int64_t b, int32_t s, const int32_t* special_ids, int32_t n_special,
                        const void* byte_lengths_per_token, int32_t table_bytes, int64_t v, int64_t vocab_len, int64_t mask_token_id, int64_t unk_token_id, int32_t mode,
                        uint64_t t_mask, uint64_t t_replace, uint64_t t_random, uint64_t seed, void* out_input_ids, int64_t ld_out, void* labels, int64_t* byte_lengths,
                        int64_t* record, double* metrics, void* workspace, int64_t workspace_bytes, void* stream) {
    if (b <= 0 || s <= 0 || v <= 0) return fail(ZETT_E_INVALID, "labelling needs b > 0 rows of s > 0 positions and a table of v > 0 ids (b = %lld, s = %d, v = %lld)", (long long)b, (int)s, (long long)v);
    const int64_t t = b * (int64_t)s;
    if (b > 0x7fffff00LL || t > 0x7fffff00LL || v > 0x7fffff00LL) return fail(ZETT_E_INVALID, "positions and ids are indexed with 32 bits (t = %lld, v = %lld)", (long long)t, (long long)v);
    if (mode != ZETT_LABEL_CLM && mode != ZETT_LABEL_MLM) return fail(ZETT_E_INVALID, "unknown mode %d", (int)mode);
    if (!width_ok(ids_bytes) || !width_ok(table_bytes)) return fail(ZETT_E_INVALID, "ids and byte lengths must be int32 or int64");
    if (!input_ids || !byte_lengths_per_token || !out_input_ids || !labels || !byte_lengths || !record || !metrics) return fail(ZETT_E_INVALID, "null argument");
    if (ld_in < s || ld_out < s) return fail(ZETT_E_INVALID, "a row of %d positions needs leading dimensions >= %d (ld_in = %lld, ld_out = %lld)", (int)s, (int)s, (long long)ld_in, (long long)ld_out);
    if (n_special < 0 || n_special > kListMax) return fail(ZETT_E_INVALID, "%d special ids are listed, at most %d travel with a launch", (int)n_special, kListMax);
    if (n_special && !special_ids) return fail(ZETT_E_INVALID, "null argument");
    if (vocab_len <= 0 || vocab_len > v) return fail(ZETT_E_INVALID, "vocab_len = %lld must be in [1, v = %lld]: a random id is an index of the byte-length table", (long long)vocab_len, (long long)v);
    if (unk_token_id < -1) return fail(ZETT_E_INVALID, "unk_token_id is an id or -1 for none, got %lld", (long long)unk_token_id);
    const int mlm = mode == ZETT_LABEL_MLM;
    if (mlm && (mask_token_id < 0 || mask_token_id >= v)) return fail(ZETT_E_INDEX, "mask_token_id %lld is outside [0, %lld)", (long long)mask_token_id, (long long)v);
    const uint64_t one = 1ull << 53;
    if (mlm && (t_mask > one || t_replace > one || t_random > one)) return fail(ZETT_E_INVALID, "a threshold is ceil(probability * 2^53): at most 2^53");
    LabelSpecials sp{};
    sp.n = n_special;
    for (int i = 0; i < n_special; ++i) {
        if (special_ids[i] < 0 || special_ids[i] >= v) return fail(ZETT_E_INDEX, "special id %d is outside [0, %lld)", (int)special_ids[i], (long long)v);
        sp.id[i] = special_ids[i];
    }
    if (!workspace || !aligned(workspace, 8)) return fail(ZETT_E_INVALID, "null or misaligned workspace");
    if (workspace_bytes < ZETT_LABEL_WORKSPACE_BYTES) return fail(ZETT_E_INVALID, "the workspace holds %lld bytes, %d are needed", (long long)workspace_bytes, (int)ZETT_LABEL_WORKSPACE_BYTES);
    LabelKeys k{};
    for (int i = 0; i < 4; ++i) k.key[i] = mix64(seed + (uint64_t)(i + 1) * 0x9E3779B97F4A7C15ull);
    k.t_mask = t_mask;
    k.t_replace = t_replace;
    k.t_random = t_random;
    hipStream_t st = (hipStream_t)stream;
    const int grid = grid256(t, kLabelGrid);
    hipLaunchKernelGGL(label_batch_kernel, dim3(grid), dim3(256), 0, st, input_ids, (int)(ids_bytes == 8), ld_in, t, (int)s, v, byte_lengths_per_token, (int)(table_bytes == 8),
                       vocab_len, mask_token_id, unk_token_id, mlm, k, out_input_ids, ld_out, labels, byte_lengths, (int64_t*)workspace, sp);
    hipLaunchKernelGGL(label_finalize_kernel, dim3(1), dim3(256), 0, st, (const int64_t*)workspace, grid, t, record, metrics);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_pad_vocabulary(const void* surface_forms, int32_t sf_bytes, int64_t ld_sf, int32_t l, int64_t v, int64_t r, const void* priors, int32_t priors_bytes,
                           void* out_surface_forms, float* out_priors, uint8_t* mask, int64_t* ids_to_embed, void* stream) {
    if (v <= 0 || r < v) return fail(ZETT_E_INVALID, "the padded vocabulary needs v > 0 rows and r >= v (v = %lld, r = %lld)", (long long)v, (long long)r);
    if (r > 0x7fffff00LL) return fail(ZETT_E_INVALID, "rows are indexed with 32 bits (r = %lld)", (long long)r);
    if (!width_ok(sf_bytes)) return fail(ZETT_E_INVALID, "surface forms must be int32 or int64");
    if (!width_ok(priors_bytes)) return fail(ZETT_E_INVALID, "priors must be float32 or float64");
    if (l <= 0 || l > kMaxL || ld_sf < l) return fail(ZETT_E_INVALID, "surface forms need 0 < l <= %d columns and ld_sf >= l (l = %d, ld_sf = %lld)", kMaxL, (int)l, (long long)ld_sf);
    if (!surface_forms || !priors || !out_surface_forms || !out_priors || !mask || !ids_to_embed) return fail(ZETT_E_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    const int grid = grid256(r * l, kMaxGrid);
#define ZETT_PAD(TE, TP)                                                                                                                                          \
    hipLaunchKernelGGL((pad_vocab_kernel<TE, TP>), dim3(grid), dim3(256), 0, st, (const TE*)surface_forms, ld_sf, (int)l, v, r, (const TP*)priors, (TE*)out_surface_forms, \
                       out_priors, mask, ids_to_embed)
    if (sf_bytes == 8 && priors_bytes == 8) ZETT_PAD(int64_t, double);
    else if (sf_bytes == 8) ZETT_PAD(int64_t, float);
    else if (priors_bytes == 8) ZETT_PAD(int32_t, double);
    else ZETT_PAD(int32_t, float);
#undef ZETT_PAD
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
