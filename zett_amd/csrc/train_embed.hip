// train_embed.hip — the input side of a training step (include/zett_hip.h, "the input side"): the special rows spliced into the
// predicted matrices (train.py:1014-1017, 1027-1030), the token lookup in the spliced input matrix with its conversion, and the
// backward of that lookup as a fixed-order sum per vocabulary row.
//
// Everything here moves rows: 16-byte accesses per lane on the wider side where pointers, leading dimensions and the row width allow
// it, an element path where they do not (E = 29, a view at an odd offset).  The lookup's backward is output-stationary: an inverted
// index of input_ids (zett_op_embed_lookup_plan: per id, its positions in ascending order — integers only, a pure function of
// input_ids) lets every row of d pred_in be written exactly once as the sum of its positions' gradient rows in ascending order, in
// chunks of ZETT_EMBED_BWD_CHUNK positions so that an id that holds thousands of positions is summed by many waves.  No float
// atomics, no memset pass, no read-modify-write: two runs give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "scan.hip.h"
#include "train_common.hip.h"

using namespace zett;

namespace {

constexpr int kChunk = ZETT_EMBED_BWD_CHUNK;          // positions of one partial sum
constexpr int kListMax = ZETT_SPLICE_MAX_ROWS;        // the longest list: the two lists travel as kernel arguments
constexpr int kMaxGrid = 1 << 18;
static_assert(kChunk == 64, "a chunk is one wave of positions: the plan's tile and the sum's position register are 64 lanes wide");

// ---- splice: listed rows from the source (or zero), every other row copied or left alone ----------------------------------------
struct SpliceList {
    int32_t n;
    int32_t row[kListMax];          // destination rows, distinct
    int32_t ref[kListMax];          // source rows
};
static_assert(sizeof(SpliceList) < 4096 - 128, "the lists must fit the kernel-argument limit");

// One wave per row.  copy_all: a work item is a row of `out` (a listed row comes from the source, or is zero; every other row is
// in's).  Otherwise a work item is a list entry and no other row is touched.  src NULL: the listed rows are zero.
template <typename TS>
__global__ __launch_bounds__(256) void splice_rows_kernel(const float* __restrict__ in, int64_t ld_in, float* __restrict__ out, int64_t ld_out, int64_t v, int e,
                                                          const TS* __restrict__ src, int64_t ld_src, int col0, int copy_all, int vec_ok, const SpliceList list) {
    const int lane = threadIdx.x & 63;
    const int64_t items = copy_all ? v : (int64_t)list.n;
    for (int64_t item = (int64_t)blockIdx.x * 4 + wave_index(); item < items; item += (int64_t)gridDim.x * 4) {
        int64_t r = item;
        int j = -1;
        if (copy_all) {
            for (int k = 0; k < list.n; k += 64) {
                const int idx = k + lane;
                const uint64_t hit = __ballot(idx < list.n && (int64_t)list.row[idx] == r);
                if (hit) { j = k + __ffsll((unsigned long long)hit) - 1; break; }
            }
        } else {
            j = (int)item;
            r = list.row[j];
        }
        float* o = out + r * ld_out;
        const int tail = vec_ok ? (e & ~3) : 0;
        if (j < 0) {
            const float* x = in + r * ld_in;
#pragma unroll 4
            for (int c = lane * 4; c < tail; c += 256) *(float4*)(o + c) = *(const float4*)(x + c);
            for (int c = tail + lane; c < e; c += 64) o[c] = x[c];
        } else if (src) {
            const TS* y = src + (int64_t)list.ref[j] * ld_src + col0;
            for (int c = lane * 4; c < tail; c += 256) *(float4*)(o + c) = load4(y + c);
            for (int c = tail + lane; c < e; c += 64) o[c] = load1(y + c);
        } else {
            for (int c = lane * 4; c < tail; c += 256) *(float4*)(o + c) = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int c = tail + lane; c < e; c += 64) o[c] = 0.f;
        }
    }
}

// ---- the lookup: out[p, :] = convert(table[ids[p], :]) --------------------------------------------------------------------------
// 2^shift threads share a position (256 >> shift positions per workgroup) and stride over its column vectors of W elements.  An id
// outside [0, v) gives a zero row and sets the error word; it is never an address.
template <typename TI, typename TO, int W>
__global__ __launch_bounds__(256) void embed_lookup_kernel(const TI* __restrict__ table, int64_t ld, int64_t v, int e, const void* __restrict__ ids, int ids64, int64_t t,
                                                           TO* __restrict__ out, int shift, int* __restrict__ error_word) {
    const int tpp = 1 << shift, ppb = 256 >> shift;
    const int sub = threadIdx.x >> shift, col = threadIdx.x & (tpp - 1);
    const int nvec = e / W;
    for (int64_t p = (int64_t)blockIdx.x * ppb + sub; p < t; p += (int64_t)gridDim.x * ppb) {
        const int64_t id = load_id(ids, ids64, p);
        const bool ok = id >= 0 && id < v;
        if (!ok && error_word && col == 0) atomicOr(error_word, 1);
        const TI* row = table + (ok ? id : 0) * ld;
        TO* o = out + p * (int64_t)e;
        if (ok) {
#pragma unroll 4
            for (int c = col; c < nvec; c += tpp) {
                const Pack<TI, W> x = *(const Pack<TI, W>*)(row + (int64_t)c * W);
                Pack<TO, W> y;
#pragma unroll
                for (int i = 0; i < W; ++i) y.v[i] = Convert<TO, TI>::go(x.v[i]);
                *(Pack<TO, W>*)(o + (int64_t)c * W) = y;
            }
        } else {
            Pack<TO, W> zero;
#pragma unroll
            for (int i = 0; i < W; ++i) zero.v[i] = TO{};
            for (int c = col; c < nvec; c += tpp) *(Pack<TO, W>*)(o + (int64_t)c * W) = zero;
        }
    }
}

// ---- the plan: the inverted index of input_ids ------------------------------------------------------------------------------------
// Words (int32) of the plan, which the backward reads, and of the scratch buffer that only the plan's own kernels use.
struct PlanLayout {
    int64_t offsets, mstart, pos, mchunk, words;                            // the plan
    int64_t counts, tiles, info, tl_w, tl_cnt, tl_base, scratch_words;      // the scratch
    int64_t maxch;
};
PlanLayout plan_layout(int64_t t, int64_t v) {
    PlanLayout L{};
    // an id with more than kChunk positions has ceil(c / 64) <= c / 64 + c / 65 chunks: fewer than t / 32 in all
    L.maxch = t / 32 + 1;
    int64_t w = 0;
    L.offsets = w; w += v + 1;          // offsets[id] .. offsets[id + 1]: the id's slice of pos
    L.mstart = w; w += v + 1;           // first chunk of the id among the chunks of ids with more than kChunk positions; [v] = their number
    L.pos = w; w += t;                  // positions by id, ascending within an id
    L.mchunk = w; w += L.maxch;         // chunk -> id
    L.words = w;
    w = 0;
    L.counts = w; w += v;               // positions per id
    L.tiles = w; w += v;                // tiles of 64 positions the id occurs in
    L.info = w; w += t;                 // per position: (slot of its tile in the id's tile list) * 64 + rank among the tile's equal ids
    L.tl_w = w; w += t;                 // the id's tile list (in arrival order): tile index,
    L.tl_cnt = w; w += t;               //   positions of the id in that tile,
    L.tl_base = w; w += t;              //   positions of the id in earlier tiles
    L.scratch_words = w;
    return L;
}

// The row a position refers to: ids[p] - id_base where that lies in [0, v), else -1 (in no list, never an address).  id_base and
// id_base + v are 32-bit values (checked on the host), so the comparison cannot overflow whatever a 64-bit id holds.
__device__ __forceinline__ int64_t plan_row(const void* __restrict__ ids, int ids64, int64_t p, int64_t id_base, int64_t v) {
    const int64_t x = load_id(ids, ids64, p);
    return (x >= id_base && x < id_base + v) ? x - id_base : -1;
}

__global__ __launch_bounds__(256) void plan_hist_kernel(const void* __restrict__ ids, int ids64, int64_t t, int64_t id_base, int64_t v, int* __restrict__ counts) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < t; p += (int64_t)gridDim.x * 256) {
        const int64_t id = plan_row(ids, ids64, p, id_base, v);
        if (id >= 0) atomicAdd(counts + id, 1);
    }
}

// exclusive scans of counts and of the chunk numbers of long lists: one workgroup, every thread a contiguous run of ids
__global__ __launch_bounds__(1024) void plan_scan_kernel(const int* __restrict__ counts, int64_t v, int* __restrict__ offsets, int* __restrict__ mstart) {
    __shared__ int s_waves0[16], s_waves1[16];
    const int tid = threadIdx.x;
    const int64_t seg = (v + 1023) / 1024, lo = std::min<int64_t>(tid * seg, v), hi = std::min<int64_t>(lo + seg, v);
    int a = 0, b = 0;
    for (int64_t i = lo; i < hi; ++i) {
        const int c = counts[i];
        a += c;
        b += c > kChunk ? (c + kChunk - 1) / kChunk : 0;
    }
    int r0 = block_exclusive_scan<1024>(a, s_waves0), r1 = block_exclusive_scan<1024>(b, s_waves1);
    for (int64_t i = lo; i < hi; ++i) {
        const int c = counts[i];
        offsets[i] = r0;
        mstart[i] = r1;
        r0 += c;
        r1 += c > kChunk ? (c + kChunk - 1) / kChunk : 0;
    }
    if (tid == 1023) {          // (its run is the last one, or empty behind the last one: r0 / r1 are the totals)
        offsets[v] = r0;
        mstart[v] = r1;
    }
}

// One wave per tile of 64 positions: a position's rank among the tile's positions of its id (ascending by construction), and one
// entry (tile, count) per id of the tile in that id's tile list.  The SLOT of the entry is whatever the atomic hands out; what is
// placed with it (plan_base_kernel, plan_place_kernel) depends on tile indices and counts only.
__global__ __launch_bounds__(256) void plan_tile_kernel(const void* __restrict__ ids, int ids64, int64_t t, int64_t id_base, int64_t v, const int* __restrict__ offsets,
                                                        int* __restrict__ tiles, int* __restrict__ tl_w, int* __restrict__ tl_cnt, int* __restrict__ info) {
    const int lane = threadIdx.x & 63;
    const int64_t n_tiles = (t + 63) / 64;
    for (int64_t w = (int64_t)blockIdx.x * 4 + wave_index(); w < n_tiles; w += (int64_t)gridDim.x * 4) {
        const int64_t p = w * 64 + lane;
        int id = -1;
        if (p < t) id = (int)plan_row(ids, ids64, p, id_base, v);
        int rank = 0, count = 0, first = 64;
#pragma unroll
        for (int k = 0; k < 64; ++k) {
            const bool same = __builtin_amdgcn_readlane(id, k) == id;
            rank += (same && k < lane) ? 1 : 0;
            count += same ? 1 : 0;
            first = (same && first == 64) ? k : first;
        }
        int slot = 0;
        if (id >= 0 && rank == 0) {
            slot = atomicAdd(tiles + id, 1);
            const int64_t at = (int64_t)offsets[id] + slot;          // slot < tiles holding the id <= its positions
            tl_w[at] = (int)w;
            tl_cnt[at] = count;
        }
        slot = __shfl(slot, first, 64);
        if (p < t) info[p] = id >= 0 ? slot * 64 + rank : -1;
    }
}

// One wave per id: positions of the id in the tiles before each of its tiles (O(L^2 / 64) for a list of L tiles: L <= t / 64), and
// the chunk -> id table of the long lists.
__global__ __launch_bounds__(256) void plan_base_kernel(int64_t v, const int* __restrict__ offsets, const int* __restrict__ mstart, const int* __restrict__ counts,
                                                        const int* __restrict__ tiles, const int* __restrict__ tl_w, const int* __restrict__ tl_cnt,
                                                        int* __restrict__ tl_base, int* __restrict__ mchunk) {
    const int lane = threadIdx.x & 63;
    for (int64_t id = (int64_t)blockIdx.x * 4 + wave_index(); id < v; id += (int64_t)gridDim.x * 4) {
        const int c = counts[id], n_tiles = tiles[id];
        const int64_t off = offsets[id];
        if (c > kChunk) {
            const int n = (c + kChunk - 1) / kChunk, m0 = mstart[id];
            for (int j = lane; j < n; j += 64) mchunk[m0 + j] = (int)id;
        }
        for (int i = lane; i < n_tiles; i += 64) {
            const int mine = tl_w[off + i];
            int base = 0;
            for (int m = 0; m < n_tiles; ++m) base += tl_w[off + m] < mine ? tl_cnt[off + m] : 0;
            tl_base[off + i] = base;
        }
    }
}

__global__ __launch_bounds__(256) void plan_place_kernel(const void* __restrict__ ids, int ids64, int64_t t, int64_t id_base, int64_t v, const int* __restrict__ offsets,
                                                         const int* __restrict__ info, const int* __restrict__ tl_base, int* __restrict__ pos) {
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < t; p += (int64_t)gridDim.x * 256) {
        const int64_t id = plan_row(ids, ids64, p, id_base, v);
        if (id < 0) continue;
        const int x = info[p];
        const int64_t off = offsets[id];
        pos[off + tl_base[off + (x >> 6)] + (x & 63)] = (int)p;
    }
}

// ---- the backward: d table[id, :] = the fixed-order sum of g[p, :] over the id's positions -----------------------------------------
template <int W> __device__ __forceinline__ void store_f32(float* p, const float (&a)[W]) {
    if constexpr (W == 1) {
        p[0] = a[0];
    } else {
#pragma unroll
        for (int i = 0; i < W; i += 4) *(float4*)(p + i) = make_float4(a[i], a[i + 1], a[i + 2], a[i + 3]);
    }
}

// A work item is (list segment, slice of 64 * W columns), one wave each; a lane owns W consecutive columns (16 bytes of g).  The
// first maxch * nslices items are the chunks of the long lists (their sums go to `partials`, one row per chunk), the rest the ids
// with at most kChunk positions, whose row of d is written here — zeros for an id that never occurs.  Four rows are requested
// before the first is added; the adds run in ascending position order.  (-0 + x == x for every x: the sum starts with its first term.)
template <typename TG, int W>
__global__ __launch_bounds__(256) void embed_bwd_sum_kernel(const TG* __restrict__ g, int e, int64_t v, const int* __restrict__ offsets, const int* __restrict__ mstart,
                                                            const int* __restrict__ mchunk, const int* __restrict__ pos, int64_t maxch, int nslices,
                                                            float* __restrict__ partials, float* __restrict__ d, int64_t ld_d) {
    const int lane = threadIdx.x & 63;
    const int64_t items = (maxch + v) * nslices;
    const int n_long = mstart[v];
    for (int64_t item = (int64_t)blockIdx.x * 4 + wave_index(); item < items; item += (int64_t)gridDim.x * 4) {
        const int64_t ri = item / nslices;
        const int col = ((int)(item - ri * nslices) * 64 + lane) * W;
        int64_t first;
        int n;
        float* dst;
        if (ri < maxch) {
            if (ri >= n_long) continue;
            const int id = mchunk[ri];
            const int j = (int)ri - mstart[id];
            first = (int64_t)offsets[id] + (int64_t)j * kChunk;
            n = std::min<int64_t>(kChunk, offsets[id + 1] - first);
            dst = partials + ri * (int64_t)e;
        } else {
            const int64_t id = ri - maxch;
            first = offsets[id];
            n = offsets[id + 1] - (int)first;
            if (n > kChunk) continue;          // written by embed_bwd_fin_kernel
            dst = d + id * ld_d;
        }
        // Every lane stays live to the store: the positions are read out of the lanes of `mine`, and a lane beyond the row's end
        // requests the row's first columns and stores nothing.
        const int mine = lane < n ? pos[first + lane] : 0;
        const bool live = col < e;
        const int lcol = live ? col : 0;
        float acc[W];
#pragma unroll
        for (int i = 0; i < W; ++i) acc[i] = n ? -0.f : 0.f;
        for (int k = 0; k < n; k += 4) {
            Pack<TG, W> x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u)          // (straight-line: beyond the end the last row is requested again and ignored)
                x[u] = *(const Pack<TG, W>*)(g + (int64_t)__builtin_amdgcn_readlane(mine, std::min(k + u, n - 1)) * e + lcol);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int i = 0; i < W; ++i) acc[i] = k + u < n ? acc[i] + lo_to_f32<TG>(x[u].v[i]) : acc[i];
            }
        }
        if (live) store_f32<W>(dst + col, acc);
    }
}

// The rows of the long lists: partial sums added in chunk order.  A work item is (chunk, slice); the item of an id's FIRST chunk adds them all.
template <int W>
__global__ __launch_bounds__(256) void embed_bwd_fin_kernel(const float* __restrict__ partials, int e, int64_t v, const int* __restrict__ offsets,
                                                            const int* __restrict__ mstart, const int* __restrict__ mchunk, int64_t maxch, int nslices,
                                                            float* __restrict__ d, int64_t ld_d) {
    const int lane = threadIdx.x & 63;
    const int64_t items = maxch * nslices;
    const int n_long = mstart[v];
    for (int64_t item = (int64_t)blockIdx.x * 4 + wave_index(); item < items; item += (int64_t)gridDim.x * 4) {
        const int64_t k0 = item / nslices;
        const int col = ((int)(item - k0 * nslices) * 64 + lane) * W;
        if (k0 >= n_long) continue;
        const int id = mchunk[k0];
        if (mstart[id] != (int)k0 || col >= e) continue;
        const int n = (offsets[id + 1] - offsets[id] + kChunk - 1) / kChunk;
        const float* x0 = partials + k0 * (int64_t)e + col;
        float acc[W];
#pragma unroll
        for (int i = 0; i < W; ++i) acc[i] = -0.f;
        for (int k = 0; k < n; k += 4) {
            Pack<float, W> x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = *(const Pack<float, W>*)(x0 + (int64_t)std::min(k + u, n - 1) * e);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
#pragma unroll
                for (int i = 0; i < W; ++i) acc[i] = k + u < n ? acc[i] + x[u].v[i] : acc[i];
            }
        }
        store_f32<W>(d + (int64_t)id * ld_d + col, acc);
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
int elem_bytes(int32_t d) { return d == ZETT_F32 ? 4 : 2; }

// W elements per access where W is one of the widths the element type takes (8: 16-bit on both sides), one otherwise
template <typename TI, typename TO>
void lookup_go(int w, hipStream_t st, const void* table, int64_t ld, int64_t v, int e, const void* ids, int ids64, int64_t t, void* out, int* error_word) {
    const int nvec = e / w;
    int shift = 0;
    while (shift < 8 && (1 << shift) < nvec) ++shift;
    const int grid = grid_for((t + (256 >> shift) - 1) / (256 >> shift), kMaxGrid);
    auto kernel = embed_lookup_kernel<TI, TO, 1>;
    if (w == 4) kernel = embed_lookup_kernel<TI, TO, 4>;
    if constexpr (sizeof(TI) == 2 && sizeof(TO) == 2) {
        if (w == 8) kernel = embed_lookup_kernel<TI, TO, 8>;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, (const TI*)table, ld, v, e, ids, ids64, t, (TO*)out, shift, error_word);
}

template <typename TG>
void bwd_sum_go(int w, hipStream_t st, const void* g, int e, int64_t v, const int* plan, const PlanLayout& L, float* partials, float* d, int64_t ld_d) {
    const int nslices = (e + 64 * w - 1) / (64 * w);
    const int grid = grid_for(((L.maxch + v) * nslices + 3) / 4, kMaxGrid);
    auto kernel = embed_bwd_sum_kernel<TG, 1>;
    if (w == 4) kernel = embed_bwd_sum_kernel<TG, 4>;
    if constexpr (sizeof(TG) == 2) {
        if (w == 8) kernel = embed_bwd_sum_kernel<TG, 8>;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, (const TG*)g, e, v, plan + L.offsets, plan + L.mstart, plan + L.mchunk, plan + L.pos, L.maxch, nslices, partials, d, ld_d);
}

int plan_args(int64_t t, int64_t v, const void* plan, int64_t plan_bytes, PlanLayout* L) {
    if (t < 0 || v <= 0) return fail(ZETT_E_INVALID, "the lookup needs t >= 0 positions and v > 0 rows (t = %lld, v = %lld)", (long long)t, (long long)v);
    if (t > 0x7fffff00LL || v > 0x7fffff00LL) return fail(ZETT_E_INVALID, "positions and rows are indexed with 32 bits (t = %lld, v = %lld)", (long long)t, (long long)v);
    *L = plan_layout(t, v);
    if (!plan || !aligned(plan, 4)) return fail(ZETT_E_INVALID, "null or misaligned plan");
    if (plan_bytes < L->words * 4) return fail(ZETT_E_INVALID, "the plan holds %lld bytes, %lld are needed", (long long)plan_bytes, (long long)(L->words * 4));
    return 0;
}

}  // namespace

extern "C" {

int zett_op_splice_rows(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t v, int32_t e, const void* src, int32_t src_dtype, int64_t ld_src,
                        int64_t src_rows, int32_t col0, const int32_t* rows, const int32_t* ref_rows, int32_t n, void* stream) {
    if (!out || n < 0 || (n && !rows)) return fail(ZETT_E_INVALID, "null argument");
    if (n > kListMax) return fail(ZETT_E_INVALID, "%d rows are listed, at most %d travel with a launch", (int)n, kListMax);
    if (v <= 0 || e <= 0 || v > 0x7fffffffLL) return fail(ZETT_E_INVALID, "the matrix needs at least one row and one column (v = %lld, e = %d)", (long long)v, (int)e);
    if (ld_out < e || (in && ld_in < e)) return fail(ZETT_E_INVALID, "a leading dimension is below %d columns", (int)e);
    if (in == out) return fail(ZETT_E_INVALID, "in and out are the same matrix: pass in = NULL to overwrite the rows in place");
    if (src) {
        if (!is_dtype(src_dtype)) return fail(ZETT_E_INVALID, "unknown source dtype %d", (int)src_dtype);
        if (n && !ref_rows) return fail(ZETT_E_INVALID, "null argument");
        if (src_rows <= 0 || col0 < 0 || (int64_t)col0 + e > ld_src) return fail(ZETT_E_INVALID, "columns [%d, %d) do not fit the source's leading dimension", (int)col0, (int)(col0 + e));
    }
    for (int i = 0; i < n; ++i) {
        if (rows[i] < 0 || rows[i] >= v) return fail(ZETT_E_INDEX, "row %d of the list is %d, outside [0, %lld)", i, (int)rows[i], (long long)v);
        if (src && (ref_rows[i] < 0 || ref_rows[i] >= src_rows)) return fail(ZETT_E_INDEX, "source row %d of the list is %d, outside [0, %lld)", i, (int)ref_rows[i], (long long)src_rows);
    }
    std::vector<int32_t> sorted(rows, rows + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(ZETT_E_INVALID, "a row is listed twice: which source row wins would be unspecified");
    if (!in && !n) return 0;
    const int es = src ? elem_bytes(src_dtype) : 4;
    const int vec_ok = aligned(out, 16) && ld_out % 4 == 0 && (!in || (aligned(in, 16) && ld_in % 4 == 0)) &&
                       (!src || (aligned(src, 4 * es) && ld_src % 4 == 0 && col0 % 4 == 0));
    hipStream_t st = (hipStream_t)stream;
    SpliceList list{};
    list.n = n;
    for (int i = 0; i < n; ++i) {
        list.row[i] = rows[i];
        list.ref[i] = src ? ref_rows[i] : 0;
    }
    const int copy_all = in != nullptr;
    const int grid = grid_for(((copy_all ? v : (int64_t)n) + 3) / 4, kMaxGrid);
    with_dtype(src ? src_dtype : ZETT_F32, [&](auto dt) {
        using TS = elem_t<decltype(dt)::value>;
        hipLaunchKernelGGL(splice_rows_kernel<TS>, dim3(grid), dim3(256), 0, st, in, ld_in, out, ld_out, v, (int)e, (const TS*)src, ld_src, (int)col0, copy_all, vec_ok, list);
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_embed_lookup(const void* table, int32_t table_dtype, int64_t ld_table, int64_t v, int32_t e, const void* ids, int32_t ids_bytes, int64_t t, void* out,
                         int32_t out_dtype, int32_t* error_word, void* stream) {
    if (!table || !ids || !out) return fail(ZETT_E_INVALID, "null argument");
    if (!is_dtype(table_dtype) || !is_dtype(out_dtype)) return fail(ZETT_E_INVALID, "unknown dtype %d -> %d", (int)table_dtype, (int)out_dtype);
    if (ids_bytes != 4 && ids_bytes != 8) return fail(ZETT_E_INVALID, "ids must be int32 or int64");
    if (v <= 0 || e <= 0 || t < 0 || ld_table < e) return fail(ZETT_E_INVALID, "the lookup needs v > 0 rows of e > 0 columns, ld_table >= e and t >= 0 (v = %lld, e = %d, ld = %lld, t = %lld)",
                                                               (long long)v, (int)e, (long long)ld_table, (long long)t);
    if (t == 0) return 0;
    // elements per access: 16 bytes on the wider side (8 when both sides are 16-bit), 4 elements where 8 do not divide, else one
    int w = (table_dtype != ZETT_F32 && out_dtype != ZETT_F32) ? 8 : 4;
    while (w > 1 && !(e % w == 0 && ld_table % w == 0 && aligned(table, w * elem_bytes(table_dtype)) && aligned(out, w * elem_bytes(out_dtype)))) w = w == 8 ? 4 : 1;
    hipStream_t st = (hipStream_t)stream;
    with_dtype(table_dtype, [&](auto it) {
        with_dtype(out_dtype, [&](auto ot) {
            lookup_go<elem_t<decltype(it)::value>, elem_t<decltype(ot)::value>>(w, st, table, ld_table, v, e, ids, ids_bytes == 8, t, out, error_word);
        });
    });
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_embed_lookup_workspace_bytes(int64_t t, int64_t v, int32_t e, int64_t* plan_bytes, int64_t* scratch_bytes, int64_t* partial_bytes) {
    if (t < 0 || v <= 0 || e <= 0 || t > 0x7fffff00LL || v > 0x7fffff00LL) return fail(ZETT_E_INVALID, "bad lookup shape (t = %lld, v = %lld, e = %d)", (long long)t, (long long)v, (int)e);
    const PlanLayout L = plan_layout(t, v);
    if (plan_bytes) *plan_bytes = L.words * 4;
    if (scratch_bytes) *scratch_bytes = L.scratch_words * 4;
    if (partial_bytes) *partial_bytes = L.maxch * (int64_t)e * 4;
    return 0;
}

int zett_op_embed_lookup_plan(const void* ids, int32_t ids_bytes, int64_t t, int64_t v, void* plan, int64_t plan_bytes, void* scratch, int64_t scratch_bytes,
                              void* stream) {
    return zett_op_embed_lookup_plan_base(ids, ids_bytes, t, 0, v, plan, plan_bytes, scratch, scratch_bytes, stream);
}

int zett_op_embed_lookup_plan_base(const void* ids, int32_t ids_bytes, int64_t t, int64_t id_base, int64_t v, void* plan, int64_t plan_bytes, void* scratch,
                                   int64_t scratch_bytes, void* stream) {
    PlanLayout L;
    if (int rc = plan_args(t, v, plan, plan_bytes, &L)) return rc;
    if (id_base < -0x80000000LL || id_base > 0x7fffffffLL || id_base + v > 0x80000000LL)
        return fail(ZETT_E_INVALID, "the ids of the rows, [id_base, id_base + v), must be 32-bit values (id_base = %lld, v = %lld)", (long long)id_base, (long long)v);
    if (!scratch || !aligned(scratch, 4)) return fail(ZETT_E_INVALID, "null or misaligned scratch");
    if (scratch_bytes < L.scratch_words * 4) return fail(ZETT_E_INVALID, "the scratch holds %lld bytes, %lld are needed", (long long)scratch_bytes, (long long)(L.scratch_words * 4));
    if ((t && !ids) || (ids_bytes != 4 && ids_bytes != 8)) return fail(ZETT_E_INVALID, "ids must be a non-null int32 or int64 array");
    hipStream_t st = (hipStream_t)stream;
    int* w = (int*)plan;
    int* s = (int*)scratch;
    const int ids64 = ids_bytes == 8;
    HIP_TRY(hipMemsetAsync(s + L.counts, 0, (size_t)(2 * v) * 4, st));          // counts and tiles
    if (t) hipLaunchKernelGGL(plan_hist_kernel, dim3(grid_for((t + 255) / 256, kMaxGrid)), dim3(256), 0, st, ids, ids64, t, id_base, v, s + L.counts);
    hipLaunchKernelGGL(plan_scan_kernel, dim3(1), dim3(1024), 0, st, (const int*)(s + L.counts), v, w + L.offsets, w + L.mstart);
    if (t) {
        hipLaunchKernelGGL(plan_tile_kernel, dim3(grid_for(((t + 63) / 64 + 3) / 4, kMaxGrid)), dim3(256), 0, st, ids, ids64, t, id_base, v, (const int*)(w + L.offsets), s + L.tiles,
                           s + L.tl_w, s + L.tl_cnt, s + L.info);
        hipLaunchKernelGGL(plan_base_kernel, dim3(grid_for((v + 3) / 4, kMaxGrid)), dim3(256), 0, st, v, (const int*)(w + L.offsets), (const int*)(w + L.mstart),
                           (const int*)(s + L.counts), (const int*)(s + L.tiles), (const int*)(s + L.tl_w), (const int*)(s + L.tl_cnt), s + L.tl_base, w + L.mchunk);
        hipLaunchKernelGGL(plan_place_kernel, dim3(grid_for((t + 255) / 256, kMaxGrid)), dim3(256), 0, st, ids, ids64, t, id_base, v, (const int*)(w + L.offsets), (const int*)(s + L.info),
                           (const int*)(s + L.tl_base), w + L.pos);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_op_embed_lookup_bwd(const void* g, int32_t g_dtype, int64_t t, int64_t v, int32_t e, const void* plan, int64_t plan_bytes, float* partials,
                             int64_t partial_bytes, float* d_table, int64_t ld_d, void* stream) {
    PlanLayout L;
    if (int rc = plan_args(t, v, plan, plan_bytes, &L)) return rc;
    if ((t && !g) || !partials || !d_table) return fail(ZETT_E_INVALID, "null argument");
    if (!is_dtype(g_dtype)) return fail(ZETT_E_INVALID, "unknown gradient dtype %d", (int)g_dtype);
    if (e <= 0 || ld_d < e) return fail(ZETT_E_INVALID, "ld_d %lld < %d columns", (long long)ld_d, (int)e);
    if (partial_bytes < L.maxch * (int64_t)e * 4) return fail(ZETT_E_INVALID, "partials holds %lld bytes, %lld are needed", (long long)partial_bytes, (long long)(L.maxch * (int64_t)e * 4));
    // columns per lane: 16 bytes of g; 4 columns (8 bytes of a 16-bit g) where 8 do not divide e; else one
    const int gb = elem_bytes(g_dtype);
    const bool vec_out = aligned(partials, 16) && aligned(d_table, 16) && ld_d % 4 == 0 && e % 4 == 0;
    int vec = vec_out ? 16 / gb : 1;
    while (vec > 1 && !(e % vec == 0 && aligned(g, vec * gb))) vec = vec == 8 ? 4 : 1;
    hipStream_t st = (hipStream_t)stream;
    const int* w = (const int*)plan;
    with_dtype(g_dtype, [&](auto dt) { bwd_sum_go<elem_t<decltype(dt)::value>>(vec, st, g, e, v, w, L, partials, d_table, ld_d); });
    const int wf = vec_out ? 4 : 1;
    const int nslices = (e + 64 * wf - 1) / (64 * wf);
    const int grid = grid_for((L.maxch * nslices + 3) / 4, kMaxGrid);
    if (vec_out)
        hipLaunchKernelGGL((embed_bwd_fin_kernel<4>), dim3(grid), dim3(256), 0, st, (const float*)partials, (int)e, v, w + L.offsets, w + L.mstart, w + L.mchunk, L.maxch, nslices,
                           d_table, ld_d);
    else
        hipLaunchKernelGGL((embed_bwd_fin_kernel<1>), dim3(grid), dim3(256), 0, st, (const float*)partials, (int)e, v, w + L.offsets, w + L.mstart, w + L.mchunk, L.maxch, nslices,
                           d_table, ld_d);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
