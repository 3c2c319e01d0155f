// tokenizer_sample.hip — a step's Unigram seed vocabulary from the batch's texts, on the device (include/zett_hip.h, "tokenizer sampling";
// what rust_utils.TokenizerSampler.sample_tokenizer computes, restated in tests/sampler_ref.py).
//
//   words      text_words.hip.h's word stage (classify / walk / compact) with the plain split pattern and a U+0020 in front of EVERY
//              text; before the compaction the slot of a text is marked as the start of the text's first word (flag bit 4)
//   count      a lane per word (lanes of a wave with the same word first sum into one): the word's starts (every stride-th entry of the reference's start list) and from each start the keys
//              of 1 .. max_length - 1 bytes.  A key is 16 bytes, 15 key bytes and the length; a key of one byte goes into a 256-bin
//              histogram in LDS (one global add per bin and workgroup), every other key into the open-addressing table
//   table      slot = a 64-bit reference (24 bits of the key's hash, 40 bits of where the key's bytes are: position and length in the
//              call's text copy while counting, an index into the queue's lists while merging) and a 32-bit score.  A slot is claimed
//              with one atomicCAS on the reference; the loser compares its key with the bytes behind the reference it got back and
//              either adds to the score or probes on.  The bytes behind a reference were written by an earlier launch, the reference
//              arrives through the atomic: no lane waits for another lane's store.  Probing is linear, wraps at the capacity and stops
//              after `capacity` slots (ZETT_SAMPLE_TABLE_FULL)
//   compact    occupied slots and non-empty bins as flags, the flags to an index list with the compaction of scan.hip.h, the list
//              gathered into (key16, score) arrays the queue owns
//   merge      the table again, rebuilt per call from every list of the queue; sum (64 bits), min and the number of keys
//   candidates p = v / sum + noise_std * z for every kept key, as 24 ordered bytes: ~bits(p) (0 for p <= 0), length, key bytes; a workgroup
//              packs the candidates of its share of the slots into the same share of the candidate array (its counter is in LDS)
//   select     MSB-first radix select over those 24 bytes, one histogram and one pick per byte: the K smallest, i.e. the K best by
//              (higher p, shorter key, smaller bytes); the survivors gathered and sorted by a bitonic network
//   emit       the fixed pieces (256 bytes, the whitespace runs) and the survivors with log(p)
//
// Integer sums are order independent and z is a function of (seed, key), so the same calls give the same bits.  No loop waits on
// another lane; every probe loop is bounded by the capacity.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <deque>
#include <vector>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "text_words.hip.h"

using namespace zett;

struct zett_sampler {
    int device = 0;
    int max_depth = 0;
    int64_t list_cap = 0, table_cap = 0, max_pieces = 0, sort_cap = 0;
    int64_t np_occ = 0, nseg_occ = 0;
    // device
    ulonglong2* list_keys = nullptr;          // [(max_depth + 1) * list_cap]
    uint32_t* list_scores = nullptr;
    int32_t* list_n = nullptr;                // [max_depth + 1]
    unsigned long long* refs = nullptr;       // [table_cap]
    uint32_t* scores = nullptr;
    uint32_t* hist1 = nullptr;                // [256]
    uint8_t* occ = nullptr;                   // [table_cap + 256 + 16]
    int32_t *idx = nullptr, *segcnt = nullptr, *segoff = nullptr, *totals = nullptr;
    void* state = nullptr;                    // SelState
    void* cand = nullptr;                     // Comp [table_cap]
    void* surv = nullptr;                     // Comp [sort_cap]
    // host: the queue of ring slots, front first
    std::deque<int> queue;
    std::vector<int> free_slots;
    bool merged = false;
    uint64_t seed = 0;
};

namespace {

constexpr uint64_t kLocMask = (1ull << 40) - 1;
constexpr int kFixedBytes = 256;
constexpr int kGrid = 4096;                 // workgroups of the other grid-stride passes, at most
constexpr int kSelGrid = 1024;              // workgroups of the passes over the merged table: each owns a contiguous share of the slots

struct Comp { uint64_t a, b, c; };            // 24 ordered bytes, most significant first

struct SelState {
    unsigned long long sum;
    uint32_t min, n_entries, n_cand, n_surv;
    uint64_t prefix[3];
    long long krem;
    int32_t take_all, pad;
    uint32_t hist[256];
    uint32_t block_n[kSelGrid];          // candidates of each workgroup's share of the slots
};

__device__ __forceinline__ uint64_t mix64(uint64_t x) {          // the finalizer of splitmix64
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
__device__ __forceinline__ uint64_t key_hash(uint64_t lo, uint64_t hi) { return mix64(lo ^ mix64(hi + 0x9E3779B97F4A7C15ull)); }

// z ~ N(0, 1) as a function of (seed, key): two counter-based 53-bit uniforms through Box-Muller
__device__ inline double key_normal(uint64_t seed, uint64_t lo, uint64_t hi) {
    const uint64_t a = mix64(mix64(mix64(seed + 0x9E3779B97F4A7C15ull) ^ lo) ^ hi);
    const uint64_t b = mix64(a + 0xD1B54A32D192ED03ull);
    const double u1 = (double)((a >> 11) + 1) * 0x1.0p-53;           // (0, 1]
    const double u2 = (double)(b >> 11) * 0x1.0p-53;                 // [0, 1)
    return sqrt(-2.0 * log(u1)) * cospi(2.0 * u2);
}

// where the bytes of a key are: the call's text copy (position * 16 + length) ...
struct RawKeys {
    const uint8_t* raw;
    __device__ __forceinline__ void get(uint64_t loc, uint64_t& lo, uint64_t& hi) const {
        const int64_t pos = (int64_t)(loc >> 4);
        const int len = (int)(loc & 15);
        lo = 0; hi = 0;
        for (int i = 0; i < len; ++i) {
            const uint64_t b = raw[pos + i];
            if (i < 8) lo |= b << (8 * i); else hi |= b << (8 * (i - 8));
        }
        hi |= (uint64_t)len << 56;
    }
};
// ... or the lists of the queue (an index)
struct ListKeys {
    const ulonglong2* keys;
    __device__ __forceinline__ void get(uint64_t loc, uint64_t& lo, uint64_t& hi) const {
        const ulonglong2 v = keys[loc];
        lo = v.x; hi = v.y;
    }
};

template <class K>
__device__ inline void table_add(unsigned long long* __restrict__ refs, uint32_t* __restrict__ scores, uint32_t cap, const K keys, uint64_t lo, uint64_t hi,
                                 uint64_t loc, uint32_t inc, int* __restrict__ status) {
    const uint64_t h = key_hash(lo, hi);
    const uint64_t tag = h & 0xFFFFFF;
    uint32_t s = (uint32_t)(((h >> 32) * (uint64_t)cap) >> 32);
    const unsigned long long mine = (tag << 40) | (loc + 1);
    for (uint32_t probe = 0; probe < cap; ++probe) {
        unsigned long long cur = __hip_atomic_load(&refs[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(&refs[s], 0ull, mine);
            if (cur == 0) { atomicAdd(&scores[s], inc); return; }
        }
        if ((cur >> 40) == tag) {
            uint64_t klo, khi;
            keys.get((cur & kLocMask) - 1, klo, khi);
            if (klo == lo && khi == hi) { atomicAdd(&scores[s], inc); return; }
        }
        s = s + 1 == cap ? 0 : s + 1;
    }
    atomicOr(status, ZETT_SAMPLE_TABLE_FULL);
}

__global__ __launch_bounds__(64) void sample_init_state_kernel(SelState* __restrict__ st, long long k_pieces) {          // (behind a memset to 0)
    if (threadIdx.x == 0) { st->min = 0xFFFFFFFFu; st->krem = k_pieces; }
}

__global__ __launch_bounds__(256) void sample_count_kernel(const uint8_t* __restrict__ raw, const uint8_t* __restrict__ codes, const uint8_t* __restrict__ flags,
                                                           const int32_t* __restrict__ woff, const int32_t* __restrict__ totals, int64_t np, int max_length, int stride,
                                                           unsigned long long* __restrict__ refs, uint32_t* __restrict__ scores, uint32_t cap,
                                                           uint32_t* __restrict__ hist1, int* __restrict__ status) {
    __shared__ uint32_t s_hist[256];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t n_words = std::min<int64_t>(std::max(totals[0], 0), np);
    const RawKeys keys{raw};
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); base < n_words; base += (int64_t)gridDim.x * 256) {          // (wave-uniform)
        const int64_t w = base + lane;
        int o0 = 0, len = 0, first = 0;
        if (w < n_words) {
            o0 = (int)std::min<int64_t>(std::max(woff[w], 0), np);
            len = (int)(std::min<int64_t>(std::max<int64_t>(woff[w + 1], o0), np) - o0);
            first = len > 0 && (flags[o0] & 4);
        }
        // Lanes of the wave that hold the same word (" the") are summed before anything is added: the lowest of them counts the
        // word's keys `mult` times, the others rest.  Equal words are equal bytes: the hash only saves the comparison.
        uint64_t wh = (uint64_t)len * 2 + first;
        for (int i = 0; i < len; ++i) wh = mix64(wh ^ raw[o0 + i]);
        uint32_t mult = 0;
        bool leader = true;
        for (int j = 0; j < 64; ++j) {
            const uint64_t hj = __shfl(wh, j, 64);
            const int oj = __shfl(o0, j, 64), lj = __shfl(len, j, 64), fj = __shfl(first, j, 64);
            if (len == 0 || hj != wh || lj != len || fj != first) continue;
            bool same = true;
            for (int i = 0; i < len && same; ++i) same = raw[o0 + i] == raw[oj + i];
            if (same) { ++mult; leader = leader && j >= lane; }
        }
        if (len == 0 || !leader) continue;
        auto emit = [&](int start) {                                   // the keys of 1 .. max_length - 1 bytes from byte `start` of the word
            uint64_t lo = 0, hi = 0;
            uint32_t inc = 0;
            const int kmax = std::min(max_length - 1, len - start);
            for (int k = 1; k <= kmax; ++k) {
                const uint64_t c = raw[o0 + start + k - 1];
                if (k <= 8) lo |= c << (8 * (k - 1)); else hi |= c << (8 * (k - 9));
                inc += ((c >= 33 && c <= 126) ? 1 : 2) * mult;         // the UTF-8 length of the byte-level character, once per lane that holds the word
                if (k == 1) atomicAdd(&s_hist[c], inc);
                else table_add(refs, scores, cap, keys, lo, hi | ((uint64_t)k << 56), (uint64_t)(o0 + start) * 16 + k, inc, status);
            }
        };
        const int o1 = o0 + len;
        int li = 0;
        if (first) { emit(0); li = 1; }                                // the first word of a text: one more 0 in front of the list
        int p1 = o0 + 1;
        while (p1 < o1 && (codes[p1] & 7) == C_SKIP) ++p1;
        for (int p = o0; p < o1;) {
            int pn = p + 1;
            while (pn < o1 && (codes[pn] & 7) == C_SKIP) ++pn;
            if (li % stride == 0) emit(pn - p1);
            ++li;
            p = pn;
        }
    }
    __syncthreads();
    if (s_hist[threadIdx.x]) atomicAdd(&hist1[threadIdx.x], s_hist[threadIdx.x]);
}

__global__ __launch_bounds__(256) void sample_occupied_kernel(const unsigned long long* __restrict__ refs, const uint32_t* __restrict__ hist1, int64_t cap,
                                                              uint8_t* __restrict__ occ) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cap + kFixedBytes; i += (int64_t)gridDim.x * 256)
        occ[i] = i < cap ? refs[i] != 0 : hist1[i - cap] != 0;
}

__global__ __launch_bounds__(256) void sample_gather_kernel(const unsigned long long* __restrict__ refs, const uint32_t* __restrict__ scores,
                                                            const uint32_t* __restrict__ hist1, int64_t cap, const uint8_t* __restrict__ raw,
                                                            const int32_t* __restrict__ idx, const int32_t* __restrict__ totals, int64_t list_cap,
                                                            ulonglong2* __restrict__ out_keys, uint32_t* __restrict__ out_scores, int32_t* __restrict__ out_n,
                                                            int* __restrict__ status) {
    const int64_t found = std::min<int64_t>(std::max(totals[0], 0), cap + kFixedBytes);
    const int64_t n = std::min(found, list_cap);
    const RawKeys keys{raw};
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *out_n = (int32_t)n;
        if (found > list_cap) atomicOr(status, ZETT_SAMPLE_LIST_FULL);
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t src = std::min<int64_t>(std::max(idx[i], 0), cap + kFixedBytes - 1);
        uint64_t lo, hi;
        uint32_t v;
        if (src < cap) {
            const unsigned long long r = refs[src];
            if (r) keys.get((r & kLocMask) - 1, lo, hi); else { lo = 0; hi = 0; }
            v = scores[src];
        } else {
            lo = (uint64_t)(src - cap);
            hi = 1ull << 56;
            v = hist1[src - cap];
        }
        out_keys[i] = make_ulonglong2(lo, hi);
        out_scores[i] = v;
    }
}

__global__ __launch_bounds__(256) void sample_merge_kernel(const ulonglong2* __restrict__ all_keys, const uint32_t* __restrict__ all_scores,
                                                           const int32_t* __restrict__ list_n, int slot, int64_t list_cap, unsigned long long* __restrict__ refs,
                                                           uint32_t* __restrict__ scores, uint32_t cap, int* __restrict__ status) {
    const int64_t n = std::min<int64_t>(std::max(list_n[slot], 0), list_cap);
    const ListKeys keys{all_keys};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const uint64_t loc = (uint64_t)slot * list_cap + i;
        const ulonglong2 k = all_keys[loc];
        if ((k.y >> 56) == 0) continue;                                // (a key the gather could not read: never counted)
        table_add(refs, scores, cap, keys, k.x, k.y, loc, all_scores[loc], status);
    }
}

__device__ __forceinline__ int whitespace_bytes(uint64_t lo, uint64_t hi, int len) {
    int n = 0;
    for (int i = 0; i < len; ++i) {
        const int c = (int)(((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8)))) & 0xff);
        n += c == 0x20 || c == 0x0A || c == 0x09;
    }
    return n;
}

// sum, min and number of the merged keys: an empty slot is never looked at
__global__ __launch_bounds__(256) void sample_stats_kernel(const unsigned long long* __restrict__ refs, const uint32_t* __restrict__ scores, int64_t cap,
                                                           SelState* __restrict__ st) {
    unsigned long long sum = 0;
    uint32_t mn = 0xFFFFFFFFu, cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += (int64_t)gridDim.x * 256)
        if (refs[i]) {
            const uint32_t v = scores[i];
            sum += v; mn = std::min(mn, v); ++cnt;
        }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum += __shfl_xor(sum, o, 64);
        mn = std::min(mn, (uint32_t)__shfl_xor(mn, o, 64));
        cnt += __shfl_xor(cnt, o, 64);
    }
    __shared__ unsigned long long s_sum[4];
    __shared__ uint32_t s_min[4], s_cnt[4];
    if ((threadIdx.x & 63) == 0) { s_sum[threadIdx.x >> 6] = sum; s_min[threadIdx.x >> 6] = mn; s_cnt[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]) {          // one add per workgroup
        atomicAdd(&st->sum, s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3]);
        atomicMin(&st->min, std::min(std::min(s_min[0], s_min[1]), std::min(s_min[2], s_min[3])));
        atomicAdd(&st->n_entries, s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3]);
    }
}

__global__ __launch_bounds__(256) void sample_candidates_kernel(const unsigned long long* __restrict__ refs, const uint32_t* __restrict__ scores, int64_t cap,
                                                                const ulonglong2* __restrict__ all_keys, double noise_std, uint64_t seed, SelState* __restrict__ st,
                                                                Comp* __restrict__ cand, int* __restrict__ status) {
    const unsigned long long total = st->sum;
    if (blockIdx.x == 0 && threadIdx.x == 0 && total >= (1ull << 32)) atomicOr(status, ZETT_SAMPLE_SUM_OVERFLOW);
    const double dsum = (double)total;
    // The workgroup's share of the slots is also its share of `cand`: it packs its candidates to the front of it, counted in LDS
    __shared__ uint32_t s_n;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    const int64_t chunk = (cap + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * chunk, hi = std::min(cap, lo + chunk);
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        const unsigned long long r = refs[i];
        if (!r) continue;
        const ulonglong2 k = all_keys[(r & kLocMask) - 1];
        const int len = (int)(k.y >> 56);
        if (len < 2 || whitespace_bytes(k.x, k.y, len) >= 2) continue;          // a fixed piece already
        double p = __ddiv_rn((double)scores[i], dsum);                           // each operation rounded on its own: a host gets the same bits
        if (noise_std != 0.0) p = __dadd_rn(p, __dmul_rn(noise_std, key_normal(seed, k.x, k.y)));
        const uint64_t u = p > 0.0 ? (uint64_t)__double_as_longlong(p) : 0;
        Comp c;
        c.a = ~u;
        c.b = ((uint64_t)len << 56) | (__builtin_bswap64(k.x) >> 8);
        c.c = ((k.x >> 56) << 56) | (__builtin_bswap64(k.y) >> 8);
        const uint32_t at = atomicAdd(&s_n, 1u);
        if (lo + at < hi) cand[lo + at] = c;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        st->block_n[blockIdx.x] = s_n;
        if (s_n) atomicAdd(&st->n_cand, s_n);
    }
}

__device__ __forceinline__ uint64_t comp_word(const Comp& c, int w) { return w == 0 ? c.a : (w == 1 ? c.b : c.c); }
__device__ __forceinline__ bool comp_less(const Comp& x, const Comp& y) {
    return x.a != y.a ? x.a < y.a : (x.b != y.b ? x.b < y.b : x.c < y.c);
}

// byte d of the candidates whose bytes [0, d) are the prefix
__global__ __launch_bounds__(256) void sample_select_hist_kernel(const Comp* __restrict__ cand, int64_t cap, SelState* __restrict__ st, int d) {
    __shared__ uint32_t s_hist[256];
    s_hist[threadIdx.x] = 0;
    __syncthreads();
    const int64_t chunk = (cap + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * chunk;
    const int64_t n = std::min<int64_t>(st->block_n[blockIdx.x], std::max<int64_t>(0, std::min(cap, lo + chunk) - lo));
    const int w = d >> 3, r = d & 7;
    const uint64_t p0 = st->prefix[0], p1 = st->prefix[1], pw = st->prefix[w];
    if (!st->take_all)
        for (int64_t i = threadIdx.x; i < n; i += 256) {
            const Comp c = cand[lo + i];
            bool in = (w < 1 || c.a == p0) && (w < 2 || c.b == p1);
            const uint64_t x = comp_word(c, w);
            if (r) in = in && (x >> (64 - 8 * r)) == (pw >> (64 - 8 * r));
            if (in) atomicAdd(&s_hist[(x >> (56 - 8 * r)) & 0xff], 1u);
        }
    __syncthreads();
    if (s_hist[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], s_hist[threadIdx.x]);
}

// the bin that holds the krem-th smallest
__global__ __launch_bounds__(64) void sample_select_pick_kernel(SelState* __restrict__ st, int d) {
    if (threadIdx.x != 0) return;
    const int w = d >> 3, r = d & 7;
    if (d == 0 && (long long)st->n_cand <= st->krem) st->take_all = 1;
    if (!st->take_all) {
        long long acc = 0;
        for (int b = 0; b < 256; ++b) {
            const long long h = st->hist[b];
            if (acc + h >= st->krem) {
                st->prefix[w] |= (uint64_t)b << (56 - 8 * r);
                st->krem -= acc;
                break;
            }
            acc += h;
        }
    }
    for (int b = 0; b < 256; ++b) st->hist[b] = 0;
}

__global__ __launch_bounds__(256) void sample_survivors_kernel(const Comp* __restrict__ cand, int64_t cap, SelState* __restrict__ st, Comp* __restrict__ surv,
                                                               int64_t sort_n) {
    const int64_t chunk = (cap + gridDim.x - 1) / gridDim.x, lo = blockIdx.x * chunk;
    const int64_t n = std::min<int64_t>(st->block_n[blockIdx.x], std::max<int64_t>(0, std::min(cap, lo + chunk) - lo));
    const Comp t{st->prefix[0], st->prefix[1], st->prefix[2]};
    const bool all = st->take_all != 0;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const Comp c = cand[lo + i];
        if (all || !comp_less(t, c)) {
            const uint32_t at = atomicAdd(&st->n_surv, 1u);
            if (at < sort_n) surv[at] = c;
        }
    }
}

__global__ __launch_bounds__(256) void sample_bitonic_kernel(Comp* __restrict__ v, int64_t n, int64_t k, int64_t j) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t l = i ^ j;
    if (i >= n || l <= i || l >= n) return;
    const Comp x = v[i], y = v[l];
    const bool up = (i & k) == 0;
    if (up ? comp_less(y, x) : comp_less(x, y)) { v[i] = y; v[l] = x; }
}

__global__ __launch_bounds__(256) void sample_emit_kernel(const SelState* __restrict__ st, const Comp* __restrict__ surv, int64_t sort_n, int max_length,
                                                          uint8_t* __restrict__ pieces, uint8_t* __restrict__ lengths, double* __restrict__ scores,
                                                          int64_t out_cap, int32_t* __restrict__ n_out, int* __restrict__ status) {
    const int64_t fixed = kFixedBytes + 9 * (int64_t)(max_length - 1);
    const int64_t n_all = fixed + std::min<int64_t>(st->n_surv, sort_n);
    const int64_t n = std::min(n_all, out_cap);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *n_out = (int32_t)n;
        if (n_all > out_cap) atomicOr(status, ZETT_SAMPLE_OUT_FULL);
    }
    const double min_log = log(__ddiv_rn((double)st->min, (double)st->sum));
    const uint8_t ws[3] = {0x20, 0x0A, 0x09};
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        uint8_t key[16];
        for (int q = 0; q < 16; ++q) key[q] = 0;
        int len;
        double s;
        if (i < kFixedBytes) {
            key[0] = (uint8_t)i; len = 1; s = min_log;
        } else if (i < fixed) {
            const int r = (int)(i - kFixedBytes), per = 3 * (max_length - 1);
            const int c1 = r / per, run = (r % per) / 3 + 1, c2 = r % 3;
            key[0] = ws[c2];
            for (int q = 1; q <= run; ++q) key[q] = ws[c1];
            len = run + 1; s = 0.0;
        } else {
            const Comp c = surv[i - fixed];
            len = (int)(c.b >> 56);
            const uint64_t lo = __builtin_bswap64((c.b << 8) | (c.c >> 56)), hi = __builtin_bswap64(c.c << 8);
            for (int q = 0; q < 8; ++q) { key[q] = (uint8_t)(lo >> (8 * q)); if (q < 7) key[8 + q] = (uint8_t)(hi >> (8 * q)); }
            const uint64_t u = ~c.a;
            s = u ? log(__longlong_as_double((long long)u)) : -100000.0;
        }
        for (int q = 0; q < 16; ++q) pieces[i * 16 + q] = key[q];
        lengths[i] = (uint8_t)len;
        scores[i] = s;
    }
}

__global__ __launch_bounds__(256) void sample_table_kernel(const unsigned long long* __restrict__ refs, const uint32_t* __restrict__ scores, int64_t cap,
                                                           const ulonglong2* __restrict__ all_keys, uint64_t seed, uint8_t* __restrict__ keys,
                                                           uint8_t* __restrict__ lengths, uint32_t* __restrict__ counts, double* __restrict__ z, int64_t out_cap,
                                                           int32_t* __restrict__ n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += (int64_t)gridDim.x * 256) {
        const unsigned long long r = refs[i];
        if (!r) continue;
        const ulonglong2 k = all_keys[(r & kLocMask) - 1];
        const int64_t at = atomicAdd(n, 1);
        if (at >= out_cap) continue;
        for (int q = 0; q < 8; ++q) { keys[at * 16 + q] = (uint8_t)(k.x >> (8 * q)); keys[at * 16 + 8 + q] = q < 7 ? (uint8_t)(k.y >> (8 * q)) : 0; }
        lengths[at] = (uint8_t)(k.y >> 56);
        counts[at] = scores[i];
        z[at] = key_normal(seed, k.x, k.y);
    }
}

void release(zett_sampler* s) {
    void* all[] = {s->list_keys, s->list_scores, s->list_n, s->refs, s->scores, s->hist1, s->occ, s->idx, s->segcnt, s->segoff, s->totals, s->state, s->cand, s->surv};
    for (void* p : all)
        if (p) (void)hipFree(p);
    delete s;
}

}  // namespace

extern "C" {

int zett_sampler_create(int device, int32_t max_depth, int64_t list_capacity, int64_t table_capacity, int64_t max_pieces, zett_sampler** out) {
    if (!out) return fail(ZETT_E_INVALID, "null argument");
    *out = nullptr;
    if (max_depth < 1 || max_depth > 4096) return fail(ZETT_E_INVALID, "max_depth = %d must be in [1, 4096]", (int)max_depth);
    if (table_capacity < 1 || table_capacity >= (1ll << 31) - 1024) return fail(ZETT_E_INVALID, "table_capacity = %lld must be in [1, 2^31 - 1024)", (long long)table_capacity);
    if (list_capacity < 1 || list_capacity > table_capacity + kFixedBytes) return fail(ZETT_E_INVALID, "list_capacity = %lld must be in [1, table_capacity + 256]", (long long)list_capacity);
    if (list_capacity * (int64_t)(max_depth + 1) >= (1ll << 39)) return fail(ZETT_E_INVALID, "list_capacity * (max_depth + 1) must stay below 2^39");
    if (max_pieces < 1 || max_pieces > (1ll << 26)) return fail(ZETT_E_INVALID, "max_pieces = %lld must be in [1, 2^26]", (long long)max_pieces);
    ZETT_ON_DEVICE(device);
    zett_sampler* s = new zett_sampler();
    s->device = device; s->max_depth = max_depth; s->list_cap = list_capacity; s->table_cap = table_capacity; s->max_pieces = max_pieces;
    s->sort_cap = 1;
    while (s->sort_cap < max_pieces) s->sort_cap <<= 1;
    s->np_occ = table_capacity + kFixedBytes;
    s->nseg_occ = compact_segments(s->np_occ);
    const int64_t slots = max_depth + 1;
    hipError_t e = hipSuccess;
    auto get = [&](auto** p, int64_t bytes) { if (e == hipSuccess) e = hipMalloc((void**)p, (size_t)bytes); };
    get(&s->list_keys, slots * list_capacity * 16);
    get(&s->list_scores, slots * list_capacity * 4);
    get(&s->list_n, slots * 4);
    get(&s->refs, table_capacity * 8);
    get(&s->scores, table_capacity * 4);
    get(&s->hist1, 256 * 4);
    get(&s->occ, s->np_occ + 16);
    get(&s->idx, (s->np_occ + 1) * 4);
    get(&s->segcnt, s->nseg_occ * 4);
    get(&s->segoff, s->nseg_occ * 4);
    get(&s->totals, 16);
    get(&s->state, sizeof(SelState));
    get(&s->cand, table_capacity * (int64_t)sizeof(Comp));
    get(&s->surv, s->sort_cap * (int64_t)sizeof(Comp));
    if (e == hipSuccess) e = hipMemset(s->list_n, 0, slots * 4);
    if (e != hipSuccess) {
        release(s);
        return fail(ZETT_E_HIP, "zett_sampler_create: %s", hipGetErrorString(e));
    }
    for (int i = (int)slots - 1; i >= 0; --i) s->free_slots.push_back(i);
    *out = s;
    return 0;
}

int zett_sampler_destroy(zett_sampler* s) {
    if (!s) return 0;
    ZETT_ON_DEVICE(s->device);
    release(s);
    return 0;
}

int zett_sampler_depth(const zett_sampler* s, int32_t* depth) {
    if (!s || !depth) return fail(ZETT_E_INVALID, "null argument");
    *depth = (int32_t)s->queue.size();
    return 0;
}

int zett_sampler_workspace_bytes(int64_t n_text, int64_t n_texts, int64_t* bytes) {
    if (int rc = shape_args("tokenizer sampling", n_text, n_texts)) return rc;
    if (!bytes) return fail(ZETT_E_INVALID, "null argument");
    Carve w;                                       // the workspace of a call is the word stage alone
    word_layout(w, n_text, n_texts);
    *bytes = w.bytes;
    return 0;
}

int zett_sampler_sample(zett_sampler* s, const uint8_t* text, const int64_t* text_offsets, int64_t n_texts, int64_t n_text, const uint8_t* class_table,
                        int64_t n_code_points, int64_t seed_size, int32_t max_length, int32_t stride, double noise_std, uint64_t seed, int32_t pop_prev,
                        int32_t push_current, uint8_t* pieces, uint8_t* piece_lengths, double* scores, int64_t out_capacity, int32_t* n_out, void* workspace,
                        int64_t workspace_bytes, int32_t* status, void* stream) {
    if (!s) return fail(ZETT_E_INVALID, "null argument");
    if (int rc = shape_args("tokenizer sampling", n_text, n_texts)) return rc;
    if (max_length < 1 || max_length > 16) return fail(ZETT_E_INVALID, "max_length = %d must be in [1, 16]: a key is at most 15 bytes", (int)max_length);
    if (stride < 1) return fail(ZETT_E_INVALID, "stride = %d must be at least 1", (int)stride);
    if (seed_size < 0) return fail(ZETT_E_INVALID, "seed_size = %lld must not be negative", (long long)seed_size);
    if (!(noise_std >= 0.0) || !(noise_std < 1e300)) return fail(ZETT_E_INVALID, "noise_std must be a finite number >= 0");
    if (!n_out) return fail(ZETT_E_INVALID, "null argument");
    const int64_t fixed = kFixedBytes + 9 * (int64_t)(max_length - 1);
    const int64_t k_pieces = std::max<int64_t>(1, seed_size - fixed);              // the length is looked at after each push: one piece always goes through
    if (pop_prev) {
        if (!pieces || !piece_lengths || !scores || out_capacity < 0) return fail(ZETT_E_INVALID, "null output");
        if (k_pieces > s->max_pieces) return fail(ZETT_E_INVALID, "seed_size = %lld asks for %lld table pieces, the sampler was created for %lld", (long long)seed_size, (long long)k_pieces, (long long)s->max_pieces);
    }
    if (!pop_prev && push_current && (int)s->queue.size() >= s->max_depth) return fail(ZETT_E_STATE, "the queue holds %d batches, the sampler was created for %d", (int)s->queue.size(), s->max_depth);
    Carve carve;
    const WordLayout L = word_layout(carve, n_text, n_texts);
    if (int rc = word_stage_args(text, text_offsets, n_texts, n_text, class_table, n_code_points, workspace, workspace_bytes, carve.bytes, status)) return rc;
    ZETT_ON_DEVICE(s->device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(status, 0, 4, st));
    HIP_TRY(hipMemsetAsync(n_out, 0, 4, st));
    const uint32_t cap = (uint32_t)s->table_cap;
    const int cur = s->free_slots.back();
    s->free_slots.pop_back();
    s->merged = false;

    // ---- this call's table, compacted into ring slot `cur`
    if (n_texts == 0) {
        HIP_TRY(hipMemsetAsync(s->list_n + cur, 0, 4, st));
    } else {
        const WordArrays a(workspace, L);
        launch_word_stage(text, text_offsets, n_texts, n_text, class_table, n_code_points, kPrefixEvenEmpty, 0, 0, true, L, a, status, st);
        HIP_TRY(hipMemsetAsync(s->refs, 0, (size_t)cap * 8, st));
        HIP_TRY(hipMemsetAsync(s->scores, 0, (size_t)cap * 4, st));
        HIP_TRY(hipMemsetAsync(s->hist1, 0, 256 * 4, st));
        hipLaunchKernelGGL(sample_count_kernel, dim3(grid256((L.np + 3) / 4, 8192)), dim3(256), 0, st, (const uint8_t*)a.raw, (const uint8_t*)a.codes, (const uint8_t*)a.flags,
                           (const int32_t*)a.woff, (const int32_t*)a.totals, L.np, (int)max_length, (int)stride, s->refs, s->scores, cap, s->hist1, status);
        hipLaunchKernelGGL(sample_occupied_kernel, dim3(grid256(s->np_occ, kGrid)), dim3(256), 0, st, (const unsigned long long*)s->refs, (const uint32_t*)s->hist1, (int64_t)cap, s->occ);
        launch_compact(s->occ, s->np_occ, s->idx, s->segcnt, s->segoff, s->totals, st);
        hipLaunchKernelGGL(sample_gather_kernel, dim3(grid256(s->list_cap, kGrid)), dim3(256), 0, st, (const unsigned long long*)s->refs, (const uint32_t*)s->scores,
                           (const uint32_t*)s->hist1, (int64_t)cap, (const uint8_t*)a.raw, (const int32_t*)s->idx, (const int32_t*)s->totals, s->list_cap,
                           s->list_keys + (int64_t)cur * s->list_cap, s->list_scores + (int64_t)cur * s->list_cap, s->list_n + cur, status);
    }

    // ---- the queue: pop_back, push_front, (merge and select), and what push_current = 0 takes back
    int prev = -1;
    if (pop_prev && !s->queue.empty()) { prev = s->queue.back(); s->queue.pop_back(); }
    s->queue.push_front(cur);
    if (pop_prev) {
        SelState* state = (SelState*)s->state;
        Comp* cand = (Comp*)s->cand;
        Comp* surv = (Comp*)s->surv;
        int64_t sort_n = 1;
        while (sort_n < k_pieces) sort_n <<= 1;
        HIP_TRY(hipMemsetAsync(s->refs, 0, (size_t)cap * 8, st));
        HIP_TRY(hipMemsetAsync(s->scores, 0, (size_t)cap * 4, st));
        HIP_TRY(hipMemsetAsync(state, 0, sizeof(SelState), st));
        hipLaunchKernelGGL(sample_init_state_kernel, dim3(1), dim3(64), 0, st, state, (long long)k_pieces);
        HIP_TRY(hipMemsetAsync(surv, 0xFF, (size_t)sort_n * sizeof(Comp), st));
        for (int q : s->queue)
            hipLaunchKernelGGL(sample_merge_kernel, dim3(grid256(s->list_cap, kGrid)), dim3(256), 0, st, (const ulonglong2*)s->list_keys, (const uint32_t*)s->list_scores,
                               (const int32_t*)s->list_n, q, s->list_cap, s->refs, s->scores, cap, status);
        const int tgrid = grid256(cap, kSelGrid);          // (the same grid for every pass over `cand`: a workgroup reads what it wrote)
        hipLaunchKernelGGL(sample_stats_kernel, dim3(tgrid), dim3(256), 0, st, (const unsigned long long*)s->refs, (const uint32_t*)s->scores, (int64_t)cap, state);
        hipLaunchKernelGGL(sample_candidates_kernel, dim3(tgrid), dim3(256), 0, st, (const unsigned long long*)s->refs, (const uint32_t*)s->scores, (int64_t)cap,
                           (const ulonglong2*)s->list_keys, noise_std, seed, state, cand, status);
        for (int d = 0; d < 24; ++d) {
            hipLaunchKernelGGL(sample_select_hist_kernel, dim3(tgrid), dim3(256), 0, st, (const Comp*)cand, (int64_t)cap, state, d);
            hipLaunchKernelGGL(sample_select_pick_kernel, dim3(1), dim3(64), 0, st, state, d);
        }
        hipLaunchKernelGGL(sample_survivors_kernel, dim3(tgrid), dim3(256), 0, st, (const Comp*)cand, (int64_t)cap, state, surv, sort_n);
        for (int64_t k = 2; k <= sort_n; k <<= 1)
            for (int64_t j = k >> 1; j > 0; j >>= 1)
                hipLaunchKernelGGL(sample_bitonic_kernel, dim3((unsigned)((sort_n + 255) / 256)), dim3(256), 0, st, surv, sort_n, k, j);
        hipLaunchKernelGGL(sample_emit_kernel, dim3(grid256(fixed + sort_n, kGrid)), dim3(256), 0, st, (const SelState*)state, (const Comp*)surv, sort_n, (int)max_length, pieces,
                           piece_lengths, scores, out_capacity, n_out, status);
        s->merged = true;
        s->seed = seed;
    }
    if (!push_current) {
        s->queue.pop_front();
        s->free_slots.push_back(cur);
        if (prev >= 0) s->queue.push_back(prev);
    } else if (prev >= 0) {
        s->free_slots.push_back(prev);
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_sampler_table(zett_sampler* s, uint8_t* keys, uint8_t* key_lengths, uint32_t* counts, double* z, int64_t capacity, int32_t* n, void* stream) {
    if (!s || !n || capacity < 0 || (capacity && (!keys || !key_lengths || !counts || !z))) return fail(ZETT_E_INVALID, "null argument");
    if (!s->merged) return fail(ZETT_E_STATE, "the merged table is there after a call with pop_prev alone");
    ZETT_ON_DEVICE(s->device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(n, 0, 4, st));
    hipLaunchKernelGGL(sample_table_kernel, dim3(grid256(s->table_cap, kGrid)), dim3(256), 0, st, (const unsigned long long*)s->refs, (const uint32_t*)s->scores, s->table_cap,
                       (const ulonglong2*)s->list_keys, s->seed, keys, key_lengths, counts, z, capacity, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
