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

}  // extern "C"
