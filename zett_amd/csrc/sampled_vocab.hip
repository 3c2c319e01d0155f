// sampled_vocab.hip — the vocabulary and the encoder tables of a sampled tokenizer, built on the device from the sampler's piece list
// (include/zett_hip.h, "sampled vocabulary"; the list surgery of the reference's Collator.sample_tokenizer, zett/collator.py:371-400, as
// the closed form of zett_amd/sampled_vocab.py).
//
// The reference's special tokens (string_k, s_k), sorted by s_k, k = 0 .. S - 1; m pieces are left after the removal.
//
//   flag       a thread per piece: keep = 0 for a piece whose bytes are a special's raw bytes
//   compact    scan.hip.h's count / scan / place: the flags into the list of the kept pieces' indices, and m
//   rows       a thread per final id v.  Special k sits at pos_k = min(s_k, m + k) (strictly increasing in k), everything else is kept
//              piece v - #{k : pos_k < v}.  The id's raw bytes into the blob (piece v at 16 * v, the specials behind the pieces), its
//              score and byte length into the outputs, the length of its byte-level text into the workspace; the minimum of the scores
//              through one atomicMin per wave on their order-preserving 64-bit keys
//   offsets    one workgroup: the scan of the text lengths into text_offsets, clamped to the capacity; the record
//   text       a thread per id: the UTF-8 of its byte-level characters into its own range of the text
//   table      a thread per id with bytes: FNV hash, then one atomicCAS on the slot's aligned {off, len} word claims the slot.  The
//              bytes behind `off` were written by `rows`, an earlier launch, and the reference to them arrives through the atomic: a
//              loser compares lengths and bytes (never the fields the winner writes after its claim) and either reports a duplicate or
//              probes on, linearly, wrapping, at most `capacity` slots.  The bitmap with atomicOr.  With ZETT_VOCAB_SCORES_THROUGH_JSON
//              the slot's score is what the library's JSON round trip makes of the sampler's (score_json.hip.h)
//
// Integers and bit copies only (the JSON round trip: 128-bit integers, one conversion and one correctly rounded division).  No lane waits for another lane; every loop is bounded by a capacity.  Whatever the status, every
// offset is clamped before it is used and every write stays inside the outputs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/zett_hip.h"
#include "retok.hip.h"
#include "scan.hip.h"
#include "score_json.hip.h"

using namespace zett;

namespace {

constexpr int kMaxSpecials = ZETT_SPLICE_MAX_ROWS;
constexpr int kMaxSpecialBytes = ZETT_SAMPLED_VOCAB_KEY_BYTES;      // raw bytes of one special token in the table
constexpr int64_t kMaxVocab = 1 << 22;
constexpr int kPieceBytes = 16;
constexpr int64_t kAnyGrid = INT32_MAX;      // the kernels below take one item per thread: no cap on their grids

struct Record {                              // zett_sampled_vocab_record
    int32_t n_vocab, n_removed, n_text, status;
    double min_score;
    double table_min_score;
};
static_assert(sizeof(Record) == 32 && sizeof(zett_sampled_vocab_record) == 32, "the record is 32 bytes");
static_assert(sizeof(PieceEntry) == 32 && offsetof(PieceEntry, off) == 8 && offsetof(PieceEntry, len) == 12, "the slot's {off, len} word is its second 8 bytes");

struct Specials {                            // device arrays, sorted by id
    const int32_t* ids;
    const int32_t* raw_off;                  // [n + 1]
    const uint8_t* raw;
    const int32_t* chars;
    const int32_t* hn;
    int32_t n, raw_bytes;
};

struct Layout {
    int64_t flags, kidx, segcnt, segoff, totals, tlen, minkey, bytes;
    int64_t np, nseg;
};
Layout layout(int64_t n_pieces, int64_t n_special) {
    Layout L{};
    L.np = n_pieces;
    L.nseg = compact_segments(L.np);
    Carve w;
    L.flags = w.take(L.np + 16);
    L.kidx = w.take((L.np + 1) * 4);
    L.segcnt = w.take(L.nseg * 4);
    L.segoff = w.take(L.nseg * 4);
    L.totals = w.take(16);
    L.tlen = w.take((L.np + n_special) * 4);
    L.minkey = w.take(16);
    L.bytes = w.bytes;
    return L;
}

__device__ __forceinline__ int clampi(int64_t v, int64_t lo, int64_t hi) { return (int)(v < lo ? lo : (v > hi ? hi : v)); }
__device__ __forceinline__ int sp_off(const Specials& s, int k) { return clampi(s.raw_off[k], 0, s.raw_bytes); }
__device__ __forceinline__ int sp_len(const Specials& s, int k) {
    const int o0 = sp_off(s, k);
    return std::min(clampi(s.raw_off[k + 1], o0, s.raw_bytes) - o0, kMaxSpecialBytes);
}
__device__ __forceinline__ int64_t sp_pos(const Specials& s, int k, int64_t m) { return std::min<int64_t>(std::max(s.ids[k], 0), m + k); }
__device__ __forceinline__ int key_byte(uint64_t lo, uint64_t hi, int b) { return (int)(((b < 8) ? (lo >> (8 * b)) : (hi >> (8 * (b - 8)))) & 0xff); }
// bytes of the UTF-8 of the byte-level character of raw byte b (byte_char_utf8 of retok.hip.h gives the bytes themselves)
__device__ __forceinline__ int char_bytes(int b) { return (b >= 33 && b <= 126) ? 1 : 2; }
// double bits <-> a 64-bit key with the order of the doubles
__device__ __forceinline__ unsigned long long order_key(unsigned long long bits) { return (bits >> 63) ? ~bits : (bits | (1ull << 63)); }
__device__ __forceinline__ unsigned long long order_bits(unsigned long long key) { return (key >> 63) ? (key & ~(1ull << 63)) : ~key; }

// the pieces of the call: n clamped to what the host sized everything for
__device__ __forceinline__ int64_t pieces_in(const int32_t* __restrict__ n, int64_t np) { return std::min<int64_t>(std::max(*n, 0), np); }

__global__ __launch_bounds__(256) void vocab_flag_kernel(const ulonglong2* __restrict__ pieces, const uint8_t* __restrict__ lengths, const int32_t* __restrict__ n,
                                                         int64_t np, const Specials sp, uint8_t* __restrict__ flags, Record* __restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    const int64_t n_in = pieces_in(n, np);
    if (i == 0) {
        if (*n < 256) atomicOr(&rec->status, ZETT_VOCAB_NOT_A_SAMPLE);
        if (*n > np) atomicOr(&rec->status, ZETT_VOCAB_OUT_FULL);
    }
    if (i >= n_in) { flags[i] = 0; return; }
    const int len = std::min<int>(lengths[i], kPieceBytes);
    const ulonglong2 key = pieces[i];
    bool keep = true;
    for (int k = 0; k < sp.n && keep; ++k) {
        if (len == 0 || sp_len(sp, k) != len) continue;
        const uint8_t* s = sp.raw + sp_off(sp, k);
        bool same = true;
        for (int b = 0; b < len && same; ++b) same = s[b] == key_byte(key.x, key.y, b);
        keep = !same;
    }
    flags[i] = keep;
}

// what final id v is: special k (>= 0), or the index of a kept piece in the sampler's list
struct Source { int special; int64_t piece; };
__device__ __forceinline__ Source source_of(int64_t v, int64_t m, const Specials& sp, const int32_t* __restrict__ kidx, int64_t np) {
    int before = 0, is = -1;
    for (int k = 0; k < sp.n; ++k) {
        const int64_t p = sp_pos(sp, k, m);
        before += p < v;
        if (p == v) is = k;
    }
    if (is >= 0) return Source{is, 0};
    const int64_t q = std::min<int64_t>(std::max<int64_t>(v - before, 0), np - 1);
    return Source{-1, (int64_t)clampi(kidx[q], 0, np - 1)};
}
// where the bytes of id v are in the blob: piece v at 16 * v, special k behind the np + n_special pieces
__device__ __forceinline__ int64_t blob_off(int64_t v, const Source& src, const Specials& sp, int64_t np) {
    return src.special >= 0 ? kPieceBytes * (np + sp.n) + sp_off(sp, src.special) : kPieceBytes * v;
}

__global__ __launch_bounds__(256) void vocab_rows_kernel(const ulonglong2* __restrict__ pieces, const uint8_t* __restrict__ lengths, const unsigned long long* __restrict__ scores,
                                                         int64_t np, const Specials sp, const int32_t* __restrict__ kidx, const int32_t* __restrict__ totals,
                                                         uint8_t* __restrict__ blob, unsigned long long* __restrict__ priors, int64_t* __restrict__ byte_lengths,
                                                         int64_t vocab_cap, int32_t* __restrict__ tlen, unsigned long long* __restrict__ minkey, int through_json) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t m = std::min<int64_t>(std::max(totals[0], 0), np);
    const int64_t nv = m + sp.n;
    unsigned long long key = ~0ull, tkey = ~0ull;                      // of the score as the outputs hold it, and as the table does
    if (v < nv) {
        const Source src = source_of(v, m, sp, kidx, np);
        unsigned long long bits = 0;                                   // 0.0
        int64_t blen;
        int tl = 0;
        if (src.special >= 0) {
            const int len = sp_len(sp, src.special);
            const uint8_t* s = sp.raw + sp_off(sp, src.special);
            uint8_t* d = blob + blob_off(v, src, sp, np);
            const bool text = sp.hn[src.special] < 0;                  // an hn special: no text, its row is patched
            for (int b = 0; b < len; ++b) { d[b] = s[b]; if (text) tl += char_bytes(s[b]); }
            blen = sp.chars[src.special];
        } else {
            const int len = std::min<int>(lengths[src.piece], kPieceBytes);
            ulonglong2 k = pieces[src.piece];
            if (len < 8) { k.x &= (1ull << (8 * len)) - 1; k.y = 0; }
            else if (len < 16) k.y &= (1ull << (8 * (len - 8))) - 1;
            *(ulonglong2*)(blob + kPieceBytes * v) = k;
            for (int b = 0; b < len; ++b) tl += char_bytes(key_byte(k.x, k.y, b));
            bits = scores[src.piece];
            blen = len;
        }
        tlen[v] = tl;
        if (v < vocab_cap) { priors[v] = bits; byte_lengths[v] = blen; }
        key = order_key(bits);
        tkey = order_key(through_json ? json_round_trip_bits(bits) : bits);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(key, o, 64), tother = __shfl_xor(tkey, o, 64);
        key = other < key ? other : key;
        tkey = tother < tkey ? tother : tkey;
    }
    if ((threadIdx.x & 63) == 0 && key != ~0ull) { atomicMin(minkey, key); atomicMin(minkey + 1, tkey); }
}

// One workgroup: thread t scans ids [t * per, (t + 1) * per); the record.
__global__ __launch_bounds__(1024) void vocab_offsets_kernel(const int32_t* __restrict__ n, int64_t np, int32_t n_special, const int32_t* __restrict__ totals,
                                                             const int32_t* __restrict__ tlen, int64_t vocab_cap, int64_t text_cap, int32_t* __restrict__ text_offsets,
                                                             const unsigned long long* __restrict__ minkey, Record* __restrict__ rec) {
    __shared__ long long s_waves[16];
    const int tid = threadIdx.x;
    const int64_t m = std::min<int64_t>(std::max(totals[0], 0), np);
    const int64_t nv = m + n_special, nout = std::min(nv, vocab_cap);
    const int64_t per = (nout + 1023) / 1024, lo = std::min(tid * per, nout), hi = std::min(lo + per, nout);
    long long mine = 0;
    for (int64_t v = lo; v < hi; ++v) mine += std::max(tlen[v], 0);
    long long total;
    long long at = block_exclusive_scan<1024>(mine, s_waves, &total);
    for (int64_t v = lo; v < hi; ++v) {
        text_offsets[v] = (int32_t)std::min<long long>(at, text_cap);
        at += std::max(tlen[v], 0);
    }
    if (tid == 0) {
        text_offsets[nout] = (int32_t)std::min<long long>(total, text_cap);
        rec->n_vocab = (int32_t)nv;
        rec->n_removed = (int32_t)(pieces_in(n, np) - m);
        rec->n_text = (int32_t)std::min<long long>(total, text_cap);
        const unsigned long long key = *minkey;
        const unsigned long long bits = key == ~0ull ? 0ull : order_bits(key);
        memcpy(&rec->min_score, &bits, 8);
        const unsigned long long tbits = minkey[1] == ~0ull ? 0ull : order_bits(minkey[1]);
        memcpy(&rec->table_min_score, &tbits, 8);
        if (nv > vocab_cap || total > text_cap) atomicOr(&rec->status, ZETT_VOCAB_OUT_FULL);
    }
}

__global__ __launch_bounds__(256) void vocab_text_kernel(int64_t np, const Specials sp, const int32_t* __restrict__ kidx, const int32_t* __restrict__ totals,
                                                         const uint8_t* __restrict__ blob, const uint8_t* __restrict__ lengths, int64_t vocab_cap, int64_t text_cap,
                                                         const int32_t* __restrict__ text_offsets, uint8_t* __restrict__ text) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t m = std::min<int64_t>(std::max(totals[0], 0), np);
    if (v >= std::min(m + sp.n, vocab_cap)) return;
    const Source src = source_of(v, m, sp, kidx, np);
    if (src.special >= 0 && sp.hn[src.special] >= 0) return;
    const int len = src.special >= 0 ? sp_len(sp, src.special) : std::min<int>(lengths[src.piece], kPieceBytes);
    const uint8_t* s = blob + blob_off(v, src, sp, np);
    int64_t at = clampi(text_offsets[v], 0, text_cap);
    const int64_t end = clampi(text_offsets[v + 1], at, text_cap);
    for (int b = 0; b < len; ++b) {
        uint8_t u[2];
        const int nu = byte_char_utf8(s[b], u);
        if (at < end) text[at++] = u[0];
        if (nu == 2 && at < end) text[at++] = u[1];
    }
}

__global__ __launch_bounds__(256) void vocab_table_kernel(int64_t np, const Specials sp, const int32_t* __restrict__ kidx, const int32_t* __restrict__ totals,
                                                          const uint8_t* __restrict__ blob, const uint8_t* __restrict__ lengths, const unsigned long long* __restrict__ scores,
                                                          PieceEntry* __restrict__ slots, uint32_t cap, uint32_t* __restrict__ bits, int32_t* __restrict__ single_id,
                                                          int64_t blob_bytes, int through_json, Record* __restrict__ rec) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t m = std::min<int64_t>(std::max(totals[0], 0), np);
    if (v >= m + sp.n) return;
    const Source src = source_of(v, m, sp, kidx, np);
    const int len = src.special >= 0 ? sp_len(sp, src.special) : std::min<int>(lengths[src.piece], kPieceBytes);
    if (len == 0) return;                                              // a string that is not byte-level: not a piece of the model's table
    const int64_t off = blob_off(v, src, sp, np);
    const uint8_t* s = blob + off;
    uint64_t h = FNV_OFFSET;
    for (int b = 0; b < len; ++b) h = fnv_step(h, s[b]);
    const uint32_t mask = cap - 1;
    const unsigned long long mine = (unsigned long long)(uint32_t)off | ((unsigned long long)(uint32_t)len << 32);
    uint32_t slot = piece_slot(h, mask);
    for (uint32_t probe = 0; probe < cap; ++probe, slot = (slot + 1) & mask) {
        PieceEntry* e = slots + slot;
        unsigned long long* word = (unsigned long long*)&e->off;
        unsigned long long cur = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0) {
            cur = atomicCAS(word, 0ull, mine);
            if (cur == 0) {                                            // the slot is this id's: nobody else writes its other fields
                e->hash = h;
                e->id = (int32_t)v;
                e->where = 0;
                unsigned long long sb = src.special >= 0 ? 0ull : scores[src.piece];
                if (through_json) sb = json_round_trip_bits(sb);          // the score as the library's own model holds it
                memcpy(&e->score, &sb, 8);
                const uint32_t b = piece_bit(h, cap * 4 - 1);
                atomicOr(&bits[b >> 5], 1u << (b & 31));
                if (len == 1) single_id[s[0]] = (int32_t)v;
                return;
            }
        }
        if ((int)(cur >> 32) != len) continue;
        const int64_t other = std::min<int64_t>((uint32_t)cur, blob_bytes - kMaxSpecialBytes);
        bool same = true;
        for (int b = 0; b < len && same; ++b) same = blob[other + b] == s[b];
        if (same) { atomicOr(&rec->status, ZETT_VOCAB_DUPLICATE); return; }
    }
    atomicOr(&rec->status, ZETT_VOCAB_TABLE_FULL);
}

__global__ __launch_bounds__(256) void vocab_readout_kernel(const PieceEntry* __restrict__ slots, uint32_t cap, const uint8_t* __restrict__ blob, int64_t blob_bytes,
                                                            uint8_t* __restrict__ keys, int32_t* __restrict__ key_lengths, int32_t* __restrict__ ids,
                                                            unsigned long long* __restrict__ scores, int64_t out_cap, int32_t* __restrict__ n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < cap; i += (int64_t)gridDim.x * 256) {
        const PieceEntry e = slots[i];
        if (e.len == 0) continue;
        const int64_t at = atomicAdd(n, 1);
        if (at >= out_cap) continue;
        const int len = clampi(e.len, 0, kMaxSpecialBytes);
        const int64_t off = clampi(e.off, 0, blob_bytes - kMaxSpecialBytes);
        for (int b = 0; b < kMaxSpecialBytes; ++b) keys[at * kMaxSpecialBytes + b] = b < len ? blob[off + b] : 0;
        key_lengths[at] = e.len;
        ids[at] = e.id;
        unsigned long long sb;
        memcpy(&sb, &e.score, 8);
        scores[at] = sb;
    }
}

// zett/utils.py:671-673: the row of a special token that is a special token of the hn tokenizer too is its hn id, then pads
__global__ __launch_bounds__(256) void vocab_patch_kernel(const Record* __restrict__ rec, const Specials sp, int32_t* __restrict__ sf, int64_t n_rows, int32_t maxlen,
                                                          int32_t pad_id) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)sp.n * maxlen) return;
    const int k = (int)(i / maxlen), col = (int)(i % maxlen);
    const int64_t m = std::max(rec->n_vocab - sp.n, 0);
    const int64_t row = sp_pos(sp, k, m);
    if (sp.hn[k] >= 0 && row < n_rows) sf[row * maxlen + col] = col == 0 ? sp.hn[k] : pad_id;
}

int specials_args(const int32_t* ids, const int32_t* raw_offsets, const uint8_t* raw, const int32_t* char_lengths, const int32_t* hn_ids, int32_t n_special,
                  int32_t raw_bytes) {
    if (n_special < 0 || n_special > kMaxSpecials) return fail(ZETT_E_INVALID, "%d special tokens, at most %d are carried", (int)n_special, kMaxSpecials);
    if (raw_bytes < 0 || raw_bytes > kMaxSpecials * kMaxSpecialBytes) return fail(ZETT_E_INVALID, "%d raw bytes of special tokens, at most %d", (int)raw_bytes, kMaxSpecials * kMaxSpecialBytes);
    if (n_special && (!ids || !raw_offsets || !char_lengths || !hn_ids || (raw_bytes && !raw))) return fail(ZETT_E_INVALID, "null special-token array");
    return 0;
}

}  // namespace

extern "C" {

int zett_retok_create_unigram_device(int device, int64_t max_vocab, zett_retok** out) {
    if (!out) return fail(ZETT_E_INVALID, "null argument");
    *out = nullptr;
    if (max_vocab < 1 || max_vocab > kMaxVocab) return fail(ZETT_E_INVALID, "max_vocab = %lld must be in [1, %lld]", (long long)max_vocab, (long long)kMaxVocab);
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(ZETT_E_INVALID, "device %d out of range", device);
    ZETT_ON_DEVICE(device);
    auto* r = new zett_retok();
    r->device = device;
    auto& sv = r->sv;
    sv.max_vocab = max_vocab;
    sv.slot_capacity = pow2_capacity((size_t)max_vocab);
    sv.blob_bytes = kPieceBytes * max_vocab + kMaxSpecials * kMaxSpecialBytes + kMaxSpecialBytes + 16;
    int32_t* bf = nullptr;
    int16_t* cp = nullptr;
    hipError_t e = hipSuccess;
    auto get = [&](auto** p, size_t bytes) {
        if (e != hipSuccess) return;
        e = hipMalloc((void**)p, bytes);
        if (e == hipSuccess) r->owned.push_back((void*)*p);
    };
    get(&sv.slots, (size_t)sv.slot_capacity * sizeof(PieceEntry));
    get(&sv.bits, (size_t)sv.slot_capacity * 4 / 8);
    get(&sv.blob, (size_t)sv.blob_bytes);
    get(&sv.single_id, 256 * 4);
    get(&bf, 256 * 4);
    get(&cp, 324 * 2);
    int16_t cp_host[324];                       // GPT-2 bytes_to_unicode, inverted (zett_retok_create)
    for (int i = 0; i < 324; ++i) cp_host[i] = -1;
    for (int b = 0, extra = 0; b < 256; ++b) {
        const bool keep = (b >= 33 && b <= 126) || (b >= 161 && b <= 172) || (b >= 174);
        cp_host[keep ? b : 256 + extra++] = (int16_t)b;
    }
    if (e == hipSuccess) e = hipMemset(sv.slots, 0, (size_t)sv.slot_capacity * sizeof(PieceEntry));
    if (e == hipSuccess) e = hipMemset(sv.bits, 0, (size_t)sv.slot_capacity * 4 / 8);
    if (e == hipSuccess) e = hipMemset(sv.blob, 0, (size_t)sv.blob_bytes);
    if (e == hipSuccess) e = hipMemset(sv.single_id, 0xFF, 256 * 4);
    if (e == hipSuccess) e = hipMemset(bf, 0xFF, 256 * 4);
    if (e == hipSuccess) e = hipMemcpy(cp, cp_host, sizeof(cp_host), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipHostMalloc((void**)&r->host_pinned, 128, hipHostMallocDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&r->done, hipEventDisableTiming);
    if (e != hipSuccess) {
        for (void* p : r->owned) (void)hipFree(p);
        if (r->host_pinned) (void)hipHostFree(r->host_pinned);
        if (r->done) (void)hipEventDestroy(r->done);
        delete r;
        return fail(ZETT_E_HIP, "zett_retok_create_unigram_device: %s", hipGetErrorString(e));
    }
    RetokTables& t = r->t;
    t.pieces = sv.slots; t.piece_mask = 15; t.piece_blob = sv.blob;
    t.piece_bits = sv.bits; t.piece_bits_mask = 16 * 4 - 1;
    t.specials = nullptr; t.special_mask = 0xffffffffu; t.special_blob = nullptr;
    t.merges = nullptr; t.merge_mask = 0xffffffffu;
    t.single_id = sv.single_id; t.bf_ids = bf; t.cp_to_byte = cp;
    t.kind = ZETT_RETOK_UNIGRAM; t.unk_id = -1; t.fuse_unk = 1; t.byte_fallback = 0; t.ignore_merges = 0;
    t.max_piece_len = kPieceBytes; t.max_word_chars = 100;
    t.unk_score = -10.0;
    sv.state = 1;
    *out = r;
    return 0;
}

int zett_sampled_vocab_workspace_bytes(int64_t max_vocab, int32_t n_special, int64_t* bytes) {
    if (max_vocab < 1 || max_vocab > kMaxVocab) return fail(ZETT_E_INVALID, "max_vocab = %lld must be in [1, %lld]", (long long)max_vocab, (long long)kMaxVocab);
    if (n_special < 0 || n_special > kMaxSpecials) return fail(ZETT_E_INVALID, "%d special tokens, at most %d are carried", (int)n_special, kMaxSpecials);
    if (!bytes) return fail(ZETT_E_INVALID, "null argument");
    *bytes = layout(max_vocab, n_special).bytes;
    return 0;
}

int zett_sampled_vocab_build(zett_retok* r, const uint8_t* pieces, const uint8_t* piece_lengths, const double* scores, const int32_t* n, int64_t piece_capacity,
                             int64_t seed_size, const int32_t* special_ids, const int32_t* special_raw_offsets, const uint8_t* special_raw,
                             const int32_t* special_char_lengths, const int32_t* special_hn_ids, int32_t n_special, int32_t special_raw_bytes, int32_t max_special_raw,
                             double* priors, int64_t* byte_lengths, int32_t* text_offsets, int64_t vocab_capacity, uint8_t* token_text, int64_t text_capacity,
                             void* record, int32_t flags, void* workspace, int64_t workspace_bytes, void* stream) {
    if (!r) return fail(ZETT_E_INVALID, "null argument");
    if (flags & ~ZETT_VOCAB_SCORES_THROUGH_JSON) return fail(ZETT_E_INVALID, "unknown flags 0x%x", (unsigned)flags);
    if (r->sv.state == 0) return fail(ZETT_E_INVALID, "the handle was not made by zett_retok_create_unigram_device");
    if (int rc = specials_args(special_ids, special_raw_offsets, special_raw, special_char_lengths, special_hn_ids, n_special, special_raw_bytes)) return rc;
    if (max_special_raw < 0 || max_special_raw > kMaxSpecialBytes) return fail(ZETT_E_INVALID, "a special token of %d raw bytes, at most %d are carried", (int)max_special_raw, kMaxSpecialBytes);
    if (!pieces || !piece_lengths || !scores || !n || !record) return fail(ZETT_E_INVALID, "null argument");
    if (!aligned(pieces, 16) || !aligned(scores, 8) || !aligned(record, 8)) return fail(ZETT_E_INVALID, "misaligned pieces (16 bytes), scores or record (8 bytes)");
    if (piece_capacity < 1 || seed_size < 1) return fail(ZETT_E_INVALID, "piece_capacity = %lld and seed_size = %lld must be at least 1", (long long)piece_capacity, (long long)seed_size);
    if (seed_size + n_special > r->sv.max_vocab)
        return fail(ZETT_E_INVALID, "seed_size + n_special = %lld is more than the handle's max_vocab = %lld", (long long)(seed_size + n_special), (long long)r->sv.max_vocab);
    if (vocab_capacity < 0 || text_capacity < 0 || text_capacity >= 0x7fffffff) return fail(ZETT_E_INVALID, "negative or too large an output capacity");
    if (!text_offsets || (vocab_capacity && (!priors || !byte_lengths)) || (text_capacity && !token_text)) return fail(ZETT_E_INVALID, "null output");
    if (!aligned(priors, 8) || !aligned(byte_lengths, 8) || !aligned(text_offsets, 4)) return fail(ZETT_E_INVALID, "misaligned output");
    const int64_t np = std::min(piece_capacity, seed_size);            // the pieces looked at: *n beyond it sets ZETT_VOCAB_OUT_FULL
    const Layout L = layout(np, n_special);
    if (!workspace || !aligned(workspace, 16)) return fail(ZETT_E_INVALID, "null or misaligned workspace (16 bytes)");
    if (workspace_bytes < L.bytes) return fail(ZETT_E_INVALID, "the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes, (long long)L.bytes);
    ZETT_ON_DEVICE(r->device);
    hipStream_t st = (hipStream_t)stream;
    auto& sv = r->sv;
    const uint32_t cap = pow2_capacity((size_t)(seed_size + n_special));          // <= slot_capacity: seed_size + n_special <= max_vocab
    sv.state = 2;
    sv.capacity = cap;
    sv.bound = np + n_special;
    sv.max_piece_len = std::max<int>(kPieceBytes, max_special_raw);

    char* w = (char*)workspace;
    uint8_t* keep = (uint8_t*)(w + L.flags);
    int32_t* kidx = (int32_t*)(w + L.kidx);
    int32_t* segcnt = (int32_t*)(w + L.segcnt);
    int32_t* segoff = (int32_t*)(w + L.segoff);
    int32_t* totals = (int32_t*)(w + L.totals);
    int32_t* tlen = (int32_t*)(w + L.tlen);
    unsigned long long* minkey = (unsigned long long*)(w + L.minkey);
    Record* rec = (Record*)record;
    const Specials sp{special_ids, special_raw_offsets, special_raw, special_char_lengths, special_hn_ids, n_special, special_raw_bytes};
    HIP_TRY(hipMemsetAsync(rec, 0, sizeof(Record), st));
    HIP_TRY(hipMemsetAsync(minkey, 0xFF, 16, st));
    HIP_TRY(hipMemsetAsync(sv.slots, 0, (size_t)cap * sizeof(PieceEntry), st));
    HIP_TRY(hipMemsetAsync(sv.bits, 0, (size_t)cap * 4 / 8, st));
    HIP_TRY(hipMemsetAsync(sv.single_id, 0xFF, 256 * 4, st));
    hipLaunchKernelGGL(vocab_flag_kernel, dim3(grid256(np, kAnyGrid)), dim3(256), 0, st, (const ulonglong2*)pieces, piece_lengths, n, np, sp, keep, rec);
    launch_compact(keep, L.np, kidx, segcnt, segoff, totals, st);
    const int vgrid = grid256(np + n_special, kAnyGrid);
    hipLaunchKernelGGL(vocab_rows_kernel, dim3(vgrid), dim3(256), 0, st, (const ulonglong2*)pieces, piece_lengths, (const unsigned long long*)scores, np, sp,
                       (const int32_t*)kidx, (const int32_t*)totals, sv.blob, (unsigned long long*)priors, byte_lengths, vocab_capacity, tlen, minkey, (int)(flags & ZETT_VOCAB_SCORES_THROUGH_JSON));
    hipLaunchKernelGGL(vocab_offsets_kernel, dim3(1), dim3(1024), 0, st, n, np, n_special, (const int32_t*)totals, (const int32_t*)tlen, vocab_capacity, text_capacity,
                       text_offsets, (const unsigned long long*)minkey, rec);
    hipLaunchKernelGGL(vocab_text_kernel, dim3(vgrid), dim3(256), 0, st, np, sp, (const int32_t*)kidx, (const int32_t*)totals, (const uint8_t*)sv.blob, piece_lengths,
                       vocab_capacity, text_capacity, (const int32_t*)text_offsets, token_text);
    hipLaunchKernelGGL(vocab_table_kernel, dim3(vgrid), dim3(256), 0, st, np, sp, (const int32_t*)kidx, (const int32_t*)totals, (const uint8_t*)sv.blob, piece_lengths,
                       (const unsigned long long*)scores, sv.slots, cap, sv.bits, sv.single_id, sv.blob_bytes, (int)(flags & ZETT_VOCAB_SCORES_THROUGH_JSON), rec);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_sampled_vocab_commit(zett_retok* r, const void* host_record) {
    if (!r || !host_record) return fail(ZETT_E_INVALID, "null argument");
    if (r->sv.state < 2) return fail(ZETT_E_STATE, "zett_sampled_vocab_build comes first");
    Record rec;
    memcpy(&rec, host_record, sizeof(rec));
    if (rec.n_vocab < 0 || rec.n_vocab > r->sv.bound) return fail(ZETT_E_INVALID, "the record's n_vocab = %d is outside [0, %lld], the bound of the build", (int)rec.n_vocab, (long long)r->sv.bound);
    RetokTables& t = r->t;
    t.piece_mask = r->sv.capacity - 1;
    t.piece_bits_mask = r->sv.capacity * 4 - 1;
    t.max_piece_len = r->sv.max_piece_len;
    t.unk_score = rec.table_min_score - 10.0;    // tokenizers kUnkPenalty, below the lowest score of the model's listing
    r->sv.state = 3;
    return 0;
}

int zett_sampled_vocab_table(zett_retok* r, uint8_t* keys, int32_t* key_lengths, int32_t* ids, double* scores, int32_t* single_id, int64_t capacity, int32_t* n,
                             void* stream) {
    if (!r || !n || capacity < 0 || (capacity && (!keys || !key_lengths || !ids || !scores))) return fail(ZETT_E_INVALID, "null argument");
    if (r->sv.state < 2) return fail(ZETT_E_STATE, "the table is there after zett_sampled_vocab_build alone");
    ZETT_ON_DEVICE(r->device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(n, 0, 4, st));
    if (single_id) HIP_TRY(hipMemcpyAsync(single_id, r->sv.single_id, 256 * 4, hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(vocab_readout_kernel, dim3(grid256(r->sv.capacity, 4096)), dim3(256), 0, st, (const PieceEntry*)r->sv.slots, r->sv.capacity,
                       (const uint8_t*)r->sv.blob, r->sv.blob_bytes, keys, key_lengths, ids, (unsigned long long*)scores, capacity, n);
    HIP_TRY(hipGetLastError());
    return 0;
}

int zett_sampled_vocab_patch_rows(zett_retok* r, const void* record, const int32_t* special_ids, const int32_t* special_hn_ids, int32_t n_special,
                                  int32_t* surface_forms, int64_t n_rows, int32_t maxlen, int32_t pad_id, void* stream) {
    if (!r || !record) return fail(ZETT_E_INVALID, "null argument");
    if (n_special < 0 || n_special > kMaxSpecials) return fail(ZETT_E_INVALID, "%d special tokens, at most %d are carried", (int)n_special, kMaxSpecials);
    if (n_rows < 0 || maxlen < 1) return fail(ZETT_E_INVALID, "bad shape");
    if (n_special == 0 || n_rows == 0) return 0;
    if (!special_ids || !special_hn_ids || !surface_forms) return fail(ZETT_E_INVALID, "null argument");
    ZETT_ON_DEVICE(r->device);
    const Specials sp{special_ids, nullptr, nullptr, nullptr, special_hn_ids, n_special, 0};
    hipLaunchKernelGGL(vocab_patch_kernel, dim3(grid256((int64_t)n_special * maxlen, kAnyGrid)), dim3(256), 0, (hipStream_t)stream, (const Record*)record, sp, surface_forms, n_rows,
                       maxlen, pad_id);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
