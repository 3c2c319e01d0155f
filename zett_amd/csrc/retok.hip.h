// retok.hip.h — get_surface_form_matrix on the device (reference zett/utils.py:651-689).
//
// Two stages, both HBM/latency-bound integer work (no MFMA here):
//
//  1. chars -> bytes.  The target tokens arrive as UTF-8 text of byte-level characters
//     (the GPT-2 printable-character alphabet, zett/utils.py:351-609).  A workgroup
//     takes 4 KiB of text with coalesced 16-byte loads, marks character starts, looks
//     every character up in the byte table staged in LDS, and compacts the bytes with a
//     wavefront scan (scan.hip.h: shuffles inside a wave, LDS across the 4 waves); block
//     totals are chained by one tiny scan launch.  A character outside the table is the
//     reference's KeyError (zett/utils.py:675).
//
//  2. bytes -> source-subtoken ids, one lane per token: special-token lookup
//     (zett/utils.py:671-673) or the hn tokenizer's bare model (zett/utils.py:681):
//       BPE      tokenizers `BPE::tokenize`: merge_word (byte fallback / unk / drop) then
//                Word::merge_all with its (rank, position) priority order and its
//                expired-entry rule, on open-addressing pair tables;
//       Unigram  tokenizers `Unigram::tokenize`: Viterbi over an FNV-hashed piece table
//                (strictly-greater updates, start positions ascending => earliest start
//                wins ties), unknown runs fused, optional byte fallback;
//       WordPiece tokenizers `WordPiece::tokenize` (zett/tokenizer_converters.py:370-373 carries
//                WordPiece hn tokenizers through): greedy longest match from every start,
//                continuing pieces in their own key space of the same hash table, the whole
//                word [UNK] on a miss or beyond max_input_chars_per_word;
//     then truncation to maxlen with the n_truncated count (zett/utils.py:683-685).
//
// Results are integers: bit-exact against the oracle and the reference by construction.
//
// This header is what more than one translation unit needs of that: the tables, their hashing and lookups, the stage-1 kernel
// template, the per-token segmentation of stage 2 and the zett_retok handle with its host-side table builders.  retok.hip holds
// the stage-2 kernels and the zett_retok_* entry points; lexical.hip, text_encode.hip and sampled_vocab.hip build on the rest.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

#include "common.hip.h"
#include "scan.hip.h"

namespace zett {

struct PieceEntry {
    uint64_t hash;
    int32_t off;
    int32_t len;      // 0 = empty slot
    int32_t id;
    int32_t where;    // WordPiece: 0 = matches at the start of a word, 1 = continuing piece (prefix stripped); else 0
    double score;
};

struct MergeEntry {
    int32_t a, b;     // a == -1: empty slot
    int32_t rank, new_id;
};

struct RetokTables {
    const PieceEntry* pieces; uint32_t piece_mask; const uint8_t* piece_blob;
    const uint32_t* piece_bits; uint32_t piece_bits_mask;      // (r6) one bit per piece hash, 32 bits of table per piece: see piece_maybe

    const PieceEntry* specials; uint32_t special_mask; const uint8_t* special_blob;
    const MergeEntry* merges; uint32_t merge_mask;
    const int32_t* single_id;     // [256] id of the one-byte piece or -1
    const int32_t* bf_ids;        // [256] id of "<0xXX>" or -1
    const int16_t* cp_to_byte;    // [324] code point -> byte or -1
    int kind, unk_id, fuse_unk, byte_fallback, ignore_merges, max_piece_len, max_word_chars;
    double unk_score;             // min_score - kUnkPenalty
#ifdef ZETT_RETOK_DEBUG
    int debug_stop;               // tools/retok_phases.sh only (-DZETT_RETOK_DEBUG): the stage-2 kernels return after phase <n>; the library never defines it
#endif
};
#ifdef ZETT_RETOK_DEBUG
#define RETOK_STOP(n) do { if (t.debug_stop == (n)) return; } while (0)
#else
#define RETOK_STOP(n) do { } while (0)
#endif

constexpr uint64_t FNV_OFFSET = 14695981039346656037ull;
constexpr uint64_t FNV_PRIME = 1099511628211ull;
constexpr uint64_t FNV_OFFSET_CONT = FNV_OFFSET ^ 0x5bd1e9955bd1e995ull;      // key space of WordPiece continuing pieces

__host__ __device__ inline uint64_t fnv_step(uint64_t h, uint8_t b) { return (h ^ b) * FNV_PRIME; }
__host__ __device__ inline uint32_t piece_slot(uint64_t h, uint32_t mask) { return (uint32_t)(h ^ (h >> 32)) & mask; }
// Pre-filter of the Unigram lookups: most (start, end) substrings of a token are not pieces, and each of those misses was a round
// trip to a 16-64 MB table.  A bitmap with 32 bits per piece (XLM-R: 1 MB — L2-resident) answers ~97 % of them from L2: bit
// piece_bit(h) is set for every piece's hash; a clear bit is a certain miss, a set bit goes to the table as before.  Same ids.
__host__ __device__ inline uint32_t piece_bit(uint64_t h, uint32_t mask) { return (uint32_t)((h * 0xD6E8FEB86659FD93ull) >> 37) & mask; }
__device__ inline bool piece_maybe(const uint32_t* bits, uint32_t mask, uint64_t h) {
    if (!bits) return true;
    const uint32_t b = piece_bit(h, mask);
    return (bits[b >> 5] >> (b & 31)) & 1u;
}
__host__ __device__ inline uint32_t merge_slot(int32_t a, int32_t b, uint32_t mask) {
    const uint64_t k = (((uint64_t)(uint32_t)a) << 32 | (uint32_t)b) * 0x9E3779B97F4A7C15ull;
    return (uint32_t)(k >> 32) & mask;
}

// bytes [0, len) of a piece in the global blob against the candidate substring.  The blob side is fetched as WHOLE 8-byte words,
// all of them before the first comparison (r6): the byte loop this replaces left after the first mismatch — so every byte was a
// load the previous one's comparison had to wait for, up to len dependent L2 round trips behind a hash hit.  The blob carries 16
// bytes of slack behind its last piece (build_piece_table), its base is 256-byte aligned (hipMalloc).
constexpr int PIECE_CMP_WORDS = 4;          // pieces of up to 32 bytes take the word path
template <typename BP>
__device__ inline bool piece_bytes_equal(const uint8_t* p, BP s, int len) {
    if (len > 8 * PIECE_CMP_WORDS) {
        int i = 0;
        while (i < len && p[i] == s[i]) ++i;
        return i == len;
    }
    const uint64_t* base = (const uint64_t*)((uintptr_t)p & ~(uintptr_t)7);
    const int sh = (int)((uintptr_t)p & 7) * 8;
    const int nw = (len + 7) >> 3;
    uint64_t w[PIECE_CMP_WORDS + 1];
#pragma unroll
    for (int j = 0; j <= PIECE_CMP_WORDS; ++j) w[j] = j <= nw ? base[j] : 0ull;
    bool eq = true;
#pragma unroll
    for (int j = 0; j < PIECE_CMP_WORDS; ++j) {
        if (j < nw) {
            const uint64_t have = sh ? ((w[j] >> sh) | (w[j + 1] << (64 - sh))) : w[j];
            uint64_t want = 0;
            const int nb = len - 8 * j < 8 ? len - 8 * j : 8;
            for (int b = 0; b < nb; ++b) want |= (uint64_t)s[8 * j + b] << (8 * b);
            const uint64_t mask = nb == 8 ? ~0ull : ((1ull << (8 * nb)) - 1ull);
            eq = eq && ((have ^ want) & mask) == 0;
        }
    }
    return eq;
}

// BP: pointer to the token's bytes — global memory, or the wave's staged text in LDS (stage 2 below)
template <typename BP>
__device__ inline const PieceEntry* piece_find(const PieceEntry* tab, uint32_t mask, const uint8_t* blob, uint64_t h, BP s, int len) {
    for (uint32_t slot = piece_slot(h, mask);; slot = (slot + 1) & mask) {
        const PieceEntry* e = tab + slot;
        if (e->len == 0) return nullptr;
        if (e->hash == h && e->len == len) {
            if (piece_bytes_equal(blob + e->off, s, len)) return e;
        }
    }
}

// the same lookup when the entry of the FIRST slot has already been fetched (unigram_token fetches several at once)
template <typename BP>
__device__ inline const PieceEntry* piece_find_from(const PieceEntry* tab, uint32_t mask, const uint8_t* blob, uint64_t h, BP s, int len,
                                                    uint32_t slot, const PieceEntry& first) {
    if (first.len == 0) return nullptr;
    if (first.hash == h && first.len == len) {
        if (piece_bytes_equal(blob + first.off, s, len)) return tab + slot;
    }
    for (slot = (slot + 1) & mask;; slot = (slot + 1) & mask) {
        const PieceEntry* e = tab + slot;
        if (e->len == 0) return nullptr;
        if (e->hash == h && e->len == len) {
            if (piece_bytes_equal(blob + e->off, s, len)) return e;
        }
    }
}

// WordPiece: the same table holds word-initial pieces (where 0, hashed from FNV_OFFSET) and continuing pieces (where 1,
// hashed from FNV_OFFSET_CONT): `where` is part of the key
template <typename BP>
__device__ inline const PieceEntry* piece_find_where(const PieceEntry* tab, uint32_t mask, const uint8_t* blob, uint64_t h, BP s, int len, int where) {
    for (uint32_t slot = piece_slot(h, mask);; slot = (slot + 1) & mask) {
        const PieceEntry* e = tab + slot;
        if (e->len == 0) return nullptr;
        if (e->hash == h && e->len == len && e->where == where) {
            if (piece_bytes_equal(blob + e->off, s, len)) return e;
        }
    }
}

__device__ inline const MergeEntry* merge_find(const RetokTables& t, int32_t a, int32_t b) {
    if (t.merge_mask == 0xffffffffu) return nullptr;   // no merges at all
    for (uint32_t slot = merge_slot(a, b, t.merge_mask);; slot = (slot + 1) & t.merge_mask) {
        const MergeEntry* e = t.merges + slot;
        if (e->a == -1) return nullptr;
        if (e->a == a && e->b == b) return e;
    }
}

// ---------------------------------------------------------------------------------------
// stage 1: UTF-8 byte-level characters -> raw bytes
// ---------------------------------------------------------------------------------------
constexpr int CH_PER_THREAD = 16;
constexpr int CH_PER_BLOCK = 256 * CH_PER_THREAD;

// MODE 0: count character starts per block.  MODE 1: decode + compact.
// SEP (r5): the text holds the tokens NUL-SEPARATED instead of coming with an offsets array (zett_retokenize_async with
// offsets == nullptr: what one "\0".join(tokens).encode() on the host produces — no per-token work there at all).  A NUL is
// then not a character: it emits no byte, and the k-th one marks the start of token k + 1 — the same block scan that numbers the
// characters numbers the separators, and raw_off[] (first raw byte of every token, what stage 2 consumes) is written HERE
// instead of by token_raw_offsets_kernel.  blk_count then holds two arrays of n_blocks + 1 ints ... see the launcher.  A bad
// character is reported with its TOKEN index (the separators before it) instead of its text position.
template <int MODE, bool SEP>
__global__ __launch_bounds__(256) void chars_to_bytes_kernel(const uint8_t* __restrict__ text, int64_t n_text,
                                                             const int16_t* __restrict__ cp_to_byte,
                                                             int32_t* __restrict__ blk_count,      // MODE 0 out / MODE 1 in (scanned)
                                                             uint8_t* __restrict__ raw, uint32_t* __restrict__ raw_pos,
                                                             unsigned long long* __restrict__ err_pos, uint32_t call,
                                                             int32_t* __restrict__ sep_count = nullptr,   // SEP: MODE 0 out / MODE 1 in (scanned)
                                                             int32_t* __restrict__ raw_off = nullptr, int64_t n_tokens = 0) {
    __shared__ int16_t s_tab[324];
    __shared__ int s_red[4];
    __shared__ int s_red2[4];
    __shared__ uint8_t s_next[256];        // first byte of the following thread's span
    if (MODE == 1)
        for (int i = threadIdx.x; i < 324; i += 256) s_tab[i] = cp_to_byte[i];
    const int64_t base = (int64_t)blockIdx.x * CH_PER_BLOCK + (int64_t)threadIdx.x * CH_PER_THREAD;
    uint8_t b[CH_PER_THREAD + 1];
    if (base + CH_PER_THREAD <= n_text && ((uintptr_t)(text + base) & 15) == 0) {
        const uint4 v = *(const uint4*)(text + base);
        memcpy(b, &v, 16);
    } else {
#pragma unroll
        for (int i = 0; i < CH_PER_THREAD; ++i) b[i] = (base + i < n_text) ? text[base + i] : 0x80;   // 0x80: never a start
    }
    if (MODE == 1) {
        s_next[threadIdx.x] = b[0];
        __syncthreads();
        if (threadIdx.x < 255) b[CH_PER_THREAD] = s_next[threadIdx.x + 1];
        else b[CH_PER_THREAD] = (base + CH_PER_THREAD < n_text) ? text[base + CH_PER_THREAD] : 0;
    }
    int cnt = 0, nsep = 0;
#pragma unroll
    for (int i = 0; i < CH_PER_THREAD; ++i) {
        const bool in = base + i < n_text;
        cnt += in && ((b[i] & 0xC0) != 0x80) && !(SEP && b[i] == 0);
        if (SEP) nsep += in && b[i] == 0;
    }
    int total = 0, total_sep = 0;
    const int excl = block_exclusive_scan<256>(cnt, s_red, &total);
    int tok = 0;
    if (SEP) tok = block_exclusive_scan<256>(nsep, s_red2, &total_sep);
    if (MODE == 0) {
        if (threadIdx.x == 0) { blk_count[blockIdx.x] = total; if (SEP) sep_count[blockIdx.x] = total_sep; }
        return;
    }
    uint32_t pos = (uint32_t)blk_count[blockIdx.x] + (uint32_t)excl;
    bool sep_ok = true;
    if (SEP) {
        tok += sep_count[blockIdx.x];                              // separators before this thread's span = index of the token it starts in
        // n_tokens tokens are n_tokens - 1 separators: a text that holds another number is refused (raw_off stays all zero — the
        // launcher cleared it — so stage 2 sees empty tokens, and the result query reports ZETT_E_INVALID)
        sep_ok = sep_count[gridDim.x] == (int32_t)(n_tokens - 1);
        if (!sep_ok && base == 0) atomicMin(err_pos, ((unsigned long long)call << 32) | 0xfffffffeull);
    }
#pragma unroll
    for (int i = 0; i < CH_PER_THREAD; ++i) {
        if (base + i >= n_text) break;
        if (!SEP) raw_pos[base + i] = pos;                         // characters before text[base+i]
        const uint8_t c = b[i];
        if (SEP) {
            if (c == 0) {                                              // token `tok` starts behind this separator
                ++tok;
                if (sep_ok) { raw_off[tok] = (int32_t)pos; if (base + i == n_text - 1) raw_off[n_tokens] = (int32_t)pos; }      // (a last, empty token)
                continue;
            }
            if (sep_ok && base + i == n_text - 1 && (c & 0xC0) == 0x80) raw_off[n_tokens] = (int32_t)pos;      // (text ends in a continuation byte)
        }
        if ((c & 0xC0) == 0x80) continue;                          // continuation byte
        int cp = -1;
        if (c < 0x80) cp = c;
        else if (c >= 0xC2 && c <= 0xDF && (b[i + 1] & 0xC0) == 0x80 && base + i + 1 < n_text) cp = ((c & 0x1F) << 6) | (b[i + 1] & 0x3F);
        const int byte = (cp >= 0 && cp < 324) ? s_tab[cp] : -1;
        if (byte < 0) atomicMin(err_pos, ((unsigned long long)call << 32) | (SEP ? (uint32_t)tok : (uint32_t)(base + i < 0x7fffffff ? base + i : 0x7ffffffe)));      // earliest call, then earliest position (SEP: token)
        raw[pos] = (uint8_t)(byte < 0 ? 0 : byte);
        ++pos;
        if (SEP && sep_ok && base + i == n_text - 1) raw_off[n_tokens] = (int32_t)pos;      // end of the last token
    }
}

// ---------------------------------------------------------------------------------------
// stage 2: a wave per 64 tokens, one lane per token; the tokens' bytes and their working state live in LDS
// ---------------------------------------------------------------------------------------
// The 64 tokens of a wave are one contiguous range of `raw`: the wave stages it in LDS with coalesced 16-byte loads.
// Every lane then sizes the working state of its token (BPE: symbol list, links and merge queue; Unigram: the Viterbi
// lattice), a wavefront scan over the 64 sizes carves one LDS arena into per-token regions, and the segmentation runs
// on LDS state — the hash tables of the model (2-4 MB: pieces, merges) are probed through L2.  A token whose bytes or
// state do not fit (a wave with > 4 KiB of text, a lane beyond the 24 KiB arena) takes the same code on global memory:
// its region of the `scratch` buffer, sized for the worst case by the host.
struct RetokLds {
    int32_t single_id[256];
    int32_t bf_ids[256];
};

constexpr int RT_TEXT_BYTES = 4096;        // staged text per wave
constexpr int RT_ARENA_WORDS = 6144;       // 24 KiB of per-token state per wave

typedef __attribute__((address_space(3))) uint8_t lds_u8;
typedef __attribute__((address_space(3))) int32_t lds_i32;
typedef __attribute__((address_space(3))) double lds_f64;
struct GlobalMem { typedef const uint8_t* bytes; typedef int32_t* words; typedef double* doubles; };
struct LdsMem { typedef const lds_u8* bytes; typedef lds_i32* words; typedef lds_f64* doubles; };

// UTF-8 bytes of the printable character standing for raw byte b
__device__ inline int byte_char_utf8(int b, uint8_t out[2]) {
    int cp;
    if ((b >= 33 && b <= 126) || (b >= 161 && b <= 172) || (b >= 174)) cp = b;
    else if (b <= 32) cp = 256 + b;
    else if (b <= 160) cp = 256 + 33 + (b - 127);
    else cp = 256 + 33 + 34;                                        // b == 173
    if (cp < 0x80) { out[0] = (uint8_t)cp; return 1; }
    out[0] = (uint8_t)(0xC0 | (cp >> 6));
    out[1] = (uint8_t)(0x80 | (cp & 0x3F));
    return 2;
}

__device__ inline bool fallback_pair(const RetokLds& L, int b, int32_t out[2], int* n) {
    uint8_t u[2];
    const int nu = byte_char_utf8(b, u);
    for (int k = 0; k < nu; ++k) {
        const int32_t id = L.bf_ids[u[k]];
        if (id < 0) return false;
        out[k] = id;
    }
    *n = nu;
    return true;
}

struct RowWriter {
    int32_t* row;
    int maxlen;
    int n;
    int32_t drop_from = 0x7fffffff;      // the lexical plan (lexical.hip): ids from here on have no source row — counted, not written
    int dropped = 0;
    __device__ void push(int32_t id) {
        if (id >= drop_from) { ++dropped; return; }
        if (n < maxlen) row[n] = id;
        ++n;
    }
};

// What zett_lexical_plan asks of stage 2 on top of the id rows (counts == nullptr: the plain retokenizer).  The handle's "special"
// table then holds the source tokenizer's whole dictionary: a whole-token hit with an id below n_rows is an exact match (count 1);
// every other token is segmented by the bare model (mode 0: not at all) with the ids >= n_rows filtered — mode 1 (fvt): one such
// id makes the count 0, mode 2 (bfvt): they are dropped and the others close up.  counts[token] is the TRUE number of ids kept,
// also beyond maxlen.
struct LexPlan {
    int32_t* counts;
    int32_t n_rows;
    int32_t mode;
    __device__ int count_of(const RowWriter& w) const { return (mode == 1 && w.dropped) ? 0 : w.n; }
};

// worst-case words of a token's region of the global scratch buffer (the fallback of the LDS arena)
constexpr int SCR_PER_BYTE = 24;
constexpr int SCR_FIXED = 16;

// tokenizers `BPE::merge_word`: the symbols the merges start from (byte fallback / unk / drop).  WRITE = false only counts.
template <bool WRITE, typename M>
__device__ inline int bpe_symbols(const RetokTables& t, const RetokLds& L, typename M::bytes raw, int len, typename M::words c) {
    int n = 0;
    bool unk_pending = false;
    for (int i = 0; i < len; ++i) {
        const int b = raw[i];
        const int32_t id = L.single_id[b];
        if (id >= 0) {
            if (unk_pending) { if (WRITE) c[n] = t.unk_id; ++n; unk_pending = false; }
            if (WRITE) c[n] = id;
            ++n;
            continue;
        }
        if (t.byte_fallback) {
            int32_t fb[2]; int nfb = 0;
            if (fallback_pair(L, b, fb, &nfb)) {            // a pending unk is not flushed first (library behaviour)
                for (int k = 0; k < nfb; ++k) { if (WRITE) c[n] = fb[k]; ++n; }
                continue;
            }
        }
        if (t.unk_id >= 0) {
            if (unk_pending && !t.fuse_unk) { if (WRITE) c[n] = t.unk_id; ++n; }
            unk_pending = true;
        }
    }
    if (unk_pending) { if (WRITE) c[n] = t.unk_id; ++n; }
    return n;
}

// state of a BPE token with n start symbols, in words: c[n] prev[n] next[n] + a queue of (rank, position, new id)
// triples with room for 2n entries — at most n - 1 pairs at the start, one more per merge, at most n - 1 merges
__device__ inline int bpe_state_words(int n) { return 9 * n + 1; }

// A merge-table lookup in two halves, so that several can be in flight at once (r6): merge_probe computes the slot and FETCHES its
// entry, merge_resolve compares and walks on only on a collision.  A lane's lookups used to wait for one another — three dependent
// L2 round trips per merge step (validate the popped pair, then the two new neighbours), one per start pair: the BPE kernel was a
// chain of ~3n round trips per token of n symbols, ~150 us whatever the vocabulary size.
struct MergeHit { bool found; int32_t rank, new_id; };
__device__ inline void merge_probe(const RetokTables& t, int32_t a, int32_t b, uint32_t& slot, MergeEntry& first) {
    slot = merge_slot(a, b, t.merge_mask);
    first = t.merges[slot];
}
__device__ inline MergeHit merge_resolve(const RetokTables& t, int32_t a, int32_t b, uint32_t slot, const MergeEntry& first) {
    if (first.a == -1) return {false, 0, 0};
    if (first.a == a && first.b == b) return {true, first.rank, first.new_id};
    for (slot = (slot + 1) & t.merge_mask;; slot = (slot + 1) & t.merge_mask) {
        const MergeEntry* e = t.merges + slot;
        if (e->a == -1) return {false, 0, 0};
        if (e->a == a && e->b == b) return {true, e->rank, e->new_id};
    }
}

template <typename M>
__device__ inline void bpe_merge(const RetokTables& t, const RetokLds& L, typename M::bytes raw, int len, int n, typename M::words scr, RowWriter& w) {
    typename M::words c = scr;        // symbol ids, -1 = removed
    typename M::words prev = c + n;
    typename M::words next = prev + n;
    typename M::words q = next + n;   // queue triples (rank, pos, new_id)
    bpe_symbols<true, M>(t, L, raw, len, c);
    for (int i = 0; i < n; ++i) { prev[i] = i - 1; next[i] = (i + 1 < n) ? i + 1 : -1; }
    int nq = 0;
    const bool have_merges = t.merge_mask != 0xffffffffu;
    if (have_merges) {
        for (int i0 = 0; i0 + 1 < n; i0 += 4) {          // the start pairs, four lookups in flight
            uint32_t slot[4];
            MergeEntry first[4];
            int32_t a[4], b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i0 + k + 1 < n) { a[k] = c[i0 + k]; b[k] = c[i0 + k + 1]; merge_probe(t, a[k], b[k], slot[k], first[k]); }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (i0 + k + 1 >= n) break;
                const MergeHit e = merge_resolve(t, a[k], b[k], slot[k], first[k]);
                if (e.found) { q[3 * nq] = e.rank; q[3 * nq + 1] = i0 + k; q[3 * nq + 2] = e.new_id; ++nq; }
            }
        }
    }
    RETOK_STOP(4);
    while (nq > 0) {                  // Word::merge_all
        int best = 0;
        for (int i = 1; i < nq; ++i)
            if (q[3 * i] < q[3 * best] || (q[3 * i] == q[3 * best] && q[3 * i + 1] < q[3 * best + 1])) best = i;
        const int pos = q[3 * best + 1], new_id = q[3 * best + 2];
        --nq;
        q[3 * best] = q[3 * nq]; q[3 * best + 1] = q[3 * nq + 1]; q[3 * best + 2] = q[3 * nq + 2];
        if (c[pos] < 0 || next[pos] == -1) continue;
        const int r = next[pos], pl = prev[pos], nr = next[r];
        // the popped pair as it stands NOW (an expired entry is one whose pair no longer merges to the same id), and — speculatively,
        // they only count if it is still valid — the two pairs the merged symbol will form with its neighbours: one round trip
        const int32_t ca = c[pos], cb = c[r];
        const int32_t la = pl >= 0 ? c[pl] : 0, rb = nr != -1 ? c[nr] : 0;
        uint32_t s0, s1 = 0, s2 = 0;
        MergeEntry f0, f1{}, f2{};
        merge_probe(t, ca, cb, s0, f0);
        if (pl >= 0) merge_probe(t, la, new_id, s1, f1);
        if (nr != -1) merge_probe(t, new_id, rb, s2, f2);
        const MergeHit e0 = merge_resolve(t, ca, cb, s0, f0);
        if (!e0.found || e0.new_id != new_id) continue;      // expired entry: compared by new id only
        c[pos] = new_id;
        c[r] = -1;
        next[pos] = nr;
        if (nr != -1) prev[nr] = pos;
        if (pl >= 0) {
            const MergeHit e = merge_resolve(t, la, new_id, s1, f1);
            if (e.found) { q[3 * nq] = e.rank; q[3 * nq + 1] = pl; q[3 * nq + 2] = e.new_id; ++nq; }
        }
        if (nr != -1) {
            const MergeHit e = merge_resolve(t, new_id, rb, s2, f2);
            if (e.found) { q[3 * nq] = e.rank; q[3 * nq + 1] = pos; q[3 * nq + 2] = e.new_id; ++nq; }
        }
    }
    RETOK_STOP(5);
    for (int i = 0; i < n; ++i)
        if (c[i] >= 0) w.push(c[i]);
}

// Viterbi lattice of a Unigram token of len bytes: best[len + 1] (double) + bstart / bid / fwd [len + 1]
__device__ inline int unigram_state_words(int len) { return 5 * (len + 1) + 1; }

// the best path of a finished lattice -> ids: backward links reversed, runs of unknown pieces fused, optional byte fallback
template <typename M>
__device__ inline void unigram_emit(const RetokTables& t, const RetokLds& L, typename M::bytes raw, int len, typename M::words bstart,
                                    typename M::words bid, typename M::words fwd, RowWriter& w) {
    for (int e = len; e > 0; e = bstart[e]) fwd[bstart[e]] = e;
    for (int s = 0; s < len;) {
        int e = fwd[s];
        if (bid[e] != -2) { w.push(bid[e]); s = e; continue; }
        int fe = e;                                 // fuse the run of unknown pieces
        while (fe < len && bid[fwd[fe]] == -2) fe = fwd[fe];
        bool ok = t.byte_fallback != 0;
        if (ok) {
            for (int i = s; i < fe && ok; ++i) { int32_t fb[2]; int nfb; ok = fallback_pair(L, raw[i], fb, &nfb); }
        }
        if (ok) {
            for (int i = s; i < fe; ++i) { int32_t fb[2]; int nfb = 0; fallback_pair(L, raw[i], fb, &nfb); for (int k = 0; k < nfb; ++k) w.push(fb[k]); }
        } else {
            w.push(t.unk_id);
        }
        s = fe;
    }
}

// returns false on "unknown token but unk_id is missing"
template <typename M>
__device__ inline bool unigram_token(const RetokTables& t, const RetokLds& L, typename M::bytes raw, int len, typename M::words scr, RowWriter& w) {
    typename M::doubles best = (typename M::doubles)scr;      // [len+1]   (regions start on 8-byte boundaries)
    typename M::words bstart = scr + 2 * (len + 1);           // [len+1]
    typename M::words bid = bstart + len + 1;                 // [len+1]  piece id, -2 = unknown
    typename M::words fwd = bid + len + 1;                    // [len+1]  forward links of the best path
    for (int i = 0; i <= len; ++i) { best[i] = 0.0; bstart[i] = -1; bid[i] = -1; }
    for (int s = 0; s < len; ++s) {
        const double base = best[s];
        bool has_single = false;
        const int emax = (s + t.max_piece_len < len) ? s + t.max_piece_len : len;
        uint64_t h = FNV_OFFSET;
        // The lookups of one start are independent of each other and of the lattice: the first slots of up to four ends are
        // fetched TOGETHER (r5: a lane's probes used to wait for one another — a 32-byte entry of a 16 MiB table is an L2 / MALL
        // miss, ~1-2 us each, and the 250 k-piece XLM-R vocabulary made this kernel 0.26 ms), then resolved in order.
        for (int e0 = s + 1; e0 <= emax; e0 += 4) {
            uint64_t hh[4];
            uint32_t slot[4];
            PieceEntry first[4];
            bool may[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                may[k] = false;
                if (e0 + k <= emax) {
                    h = fnv_step(h, raw[e0 + k - 1]);
                    hh[k] = h;
                    may[k] = piece_maybe(t.piece_bits, t.piece_bits_mask, h);
                    if (may[k]) { slot[k] = piece_slot(h, t.piece_mask); first[k] = t.pieces[slot[k]]; }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int e = e0 + k;
                if (e > emax) break;
                if (!may[k]) continue;
                const PieceEntry* p = piece_find_from(t.pieces, t.piece_mask, t.piece_blob, hh[k], raw + s, e - s, slot[k], first[k]);
                if (!p) continue;
                const double cand = p->score + base;
                if (bstart[e] == -1 || cand > best[e]) { best[e] = cand; bstart[e] = s; bid[e] = p->id; }
                if (e == s + 1) has_single = true;
            }
        }
        if (!has_single) {
            if (t.unk_id < 0) return false;
            const double cand = t.unk_score + base;
            const int e = s + 1;
            if (bstart[e] == -1 || cand > best[e]) { best[e] = cand; bstart[e] = s; bid[e] = -2; }
        }
    }
    unigram_emit<M>(t, L, raw, len, bstart, bid, fwd, w);
    return true;
}

// tokenizers `WordPiece::tokenize`.  Returns false on "the word is [UNK] but [UNK] is not in the vocabulary".  From each
// start the library tries the longest substring first and shortens it a character at a time; walking the ends upwards
// with a running hash and keeping the LAST hit finds the same piece.  One byte-level character is one raw byte.
template <typename M>
__device__ inline bool wordpiece_token(const RetokTables& t, typename M::bytes raw, int len, RowWriter& w, int32_t pad_id) {
    if (len > t.max_word_chars) {
        if (t.unk_id < 0) return false;
        w.push(t.unk_id);
        return true;
    }
    const int n0 = w.n;
    for (int s = 0; s < len;) {
        const int where = s == 0 ? 0 : 1;
        uint64_t h = where ? FNV_OFFSET_CONT : FNV_OFFSET;
        const int emax = (s + t.max_piece_len < len) ? s + t.max_piece_len : len;
        int best_e = -1, best_id = -1;
        for (int e = s + 1; e <= emax; ++e) {
            h = fnv_step(h, raw[e - 1]);
            const PieceEntry* p = piece_find_where(t.pieces, t.piece_mask, t.piece_blob, h, raw + s, e - s, where);
            if (p) { best_e = e; best_id = p->id; }
        }
        if (best_e < 0) {                                   // is_bad: the pieces found so far are dropped, the word is [UNK]
            if (t.unk_id < 0) return false;
            for (int i = n0; i < w.n && i < w.maxlen; ++i) w.row[i] = pad_id;
            w.n = n0;
            w.dropped = 0;
            w.push(t.unk_id);
            return true;
        }
        w.push(best_id);
        s = best_e;
    }
    return true;
}

// special-token lookup (zett/utils.py:671-673) and, with ignore_merges, the whole-token lookup of BPE::tokenize: -1 = no hit
template <typename M>
__device__ inline int whole_token_id(const PieceEntry* tab, uint32_t mask, const uint8_t* blob, typename M::bytes s, int len) {
    uint64_t h = FNV_OFFSET;
    for (int i = 0; i < len; ++i) h = fnv_step(h, s[i]);
    const PieceEntry* e = piece_find(tab, mask, blob, h, s, len);
    return e ? e->id : -1;
}

// one token: `n_sym` = its BPE start symbols (0 for the other kinds), `scr` = its state region
template <typename M>
__device__ inline bool segment_token(const RetokTables& t, const RetokLds& L, typename M::bytes s, int len, int n_sym, typename M::words scr,
                                     RowWriter& w, int32_t pad_id) {
    if (t.kind == ZETT_RETOK_BPE) { bpe_merge<M>(t, L, s, len, n_sym, scr, w); return true; }
    if (t.kind == ZETT_RETOK_UNIGRAM) return unigram_token<M>(t, L, s, len, scr, w);
    return wordpiece_token<M>(t, s, len, w, pad_id);
}

}  // namespace zett

// =========================================================================================
// host side
// =========================================================================================
struct zett_retok {
    int device = 0;
    zett::RetokTables t{};
    std::vector<void*> owned;
    zett::DevBuf raw, raw_pos, raw_off, blk, scratch, misc;
    int32_t* host_pinned = nullptr;      // [0..1] text length (sync entry point); [4..9] the three 64-bit result words; [12..17] their initial values
    hipEvent_t done = nullptr;           // behind the last enqueued call's result copy
    uint32_t calls = 0;                  // calls enqueued since the last result query (ordinal of the next call)
    struct Call { const int32_t* offsets; int64_t n_tokens; };
    std::vector<Call> recent;            // the calls since the last result query (for the token of a KeyError)
    bool words_ready = false;            // the device result words hold their initial values
    int unigram_wg = 1;                  // Unigram models: 1 = the workgroup-per-64-tokens kernel for calls of up to 32 768 tokens, 2 = always, 0 = never (the lane-per-token kernel)
    // A handle of zett_retok_create_unigram_device (sampled_vocab.hip): its piece table is filled on the device, per step.
    // state 0: not such a handle; 1: created, empty; 2: built, the record not committed yet; 3: committed — only then does it tokenize.
    struct SampledVocab {
        int state = 0;
        int64_t max_vocab = 0;
        zett::PieceEntry* slots = nullptr; uint32_t slot_capacity = 0;      // (the allocation: pow2_capacity(max_vocab) slots)
        uint32_t* bits = nullptr;
        uint8_t* blob = nullptr; int64_t blob_bytes = 0;
        int32_t* single_id = nullptr;
        uint32_t capacity = 0;           // slots of the last build: pow2_capacity(its bound)
        int64_t bound = 0;               // the last build's upper bound of n_vocab
        int max_piece_len = 0;
    } sv;
    bool tokenizes() const { return sv.state == 0 || sv.state == 3; }
};

namespace zett {

// Open addressing with linear probing, load factor 1/16 .. 1/8 (r6; was 1/4 .. 1/2).  A wave waits for the LONGEST probe chain among
// its 64 lanes' lookups, every probe a dependent L2 / MALL round trip, and the clusters of linear probing at half load have a heavy
// tail: the phase timing of round 6 (tools/retok_ab.py on a -DZETT_RETOK_DEBUG build) put 48 of a Unigram workgroup's 87 us into
// its lookups and 70 of the BPE kernel's 135 into the merge loop.  Memory is not the constraint on a 288 GB part (XLM-R's 250 k
// pieces: 64 MB; Llama-3's 128 k merges: 16 MB).
inline uint32_t pow2_capacity(size_t n) {
    uint32_t c = 16;
    while (c < 8 * n + 2) c <<= 1;
    return c;
}

struct HostPieceTable {
    std::vector<PieceEntry> slots;
    std::vector<uint8_t> blob;
    std::vector<uint32_t> bits;          // piece_maybe's bitmap (word-initial WordPiece / all other pieces alike: keyed by the hash)
    uint32_t bits_mask = 0;
    uint32_t mask = 0xffffffffu;
    int max_len = 0;
};

inline void build_piece_table(const uint8_t* bytes, const int32_t* offsets, const int32_t* ids, const double* scores, int n,
                              HostPieceTable& out, int32_t* single_id /* nullable */, const uint8_t* where = nullptr /* WordPiece: 1 = continuing piece */) {
    // duplicates: the LAST listed piece wins (tokenizers inserts into a HashMap in listing order)
    std::unordered_map<std::string, int> last;
    last.reserve((size_t)n * 2);
    for (int i = 0; i < n; ++i) {
        const int len = offsets[i + 1] - offsets[i];
        if (len <= 0) continue;
        std::string key((const char*)bytes + offsets[i], (size_t)len);
        if (where) key.push_back(where[i] ? '\1' : '\0');        // the key space is part of the key
        last[key] = i;
    }
    if (last.empty()) return;
    const uint32_t cap = pow2_capacity(last.size());
    out.mask = cap - 1;
    out.slots.assign(cap, PieceEntry{0, 0, 0, 0, 0, 0.0});
    out.bits_mask = cap * 4 - 1;         // 32 .. 64 bits per piece
    out.bits.assign((size_t)cap * 4 / 32, 0u);
    for (auto& kv : last) {
        const int i = kv.second;
        const int len = (int)kv.first.size() - (where ? 1 : 0);
        const int wh = where ? (where[i] ? 1 : 0) : 0;
        uint64_t h = wh ? FNV_OFFSET_CONT : FNV_OFFSET;
        for (int k = 0; k < len; ++k) h = fnv_step(h, (uint8_t)kv.first[k]);
        PieceEntry e{h, (int32_t)out.blob.size(), len, ids[i], wh, scores ? scores[i] : 0.0};
        out.blob.insert(out.blob.end(), kv.first.begin(), kv.first.begin() + len);
        uint32_t slot = piece_slot(h, out.mask);
        while (out.slots[slot].len != 0) slot = (slot + 1) & out.mask;
        out.slots[slot] = e;
        { const uint32_t b = piece_bit(h, out.bits_mask); out.bits[b >> 5] |= 1u << (b & 31); }
        if (len > out.max_len) out.max_len = len;
        if (single_id && len == 1 && !wh) single_id[(uint8_t)kv.first[0]] = ids[i];
    }
    out.blob.resize(out.blob.size() + 16, 0);          // slack for piece_bytes_equal's whole-word reads
}

template <typename U>
inline int upload(zett_retok* r, const std::vector<U>& v, const U** dev) {
    *dev = nullptr;
    if (v.empty()) return 0;
    void* p = nullptr;
    HIP_TRY(hipMalloc(&p, v.size() * sizeof(U)));
    r->owned.push_back(p);
    HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(U), hipMemcpyHostToDevice));
    *dev = (const U*)p;
    return 0;
}

// zett_retokenize_async, and with lex.counts set the same call as stages 1 and 2 of zett_lexical_plan (lexical.hip).  Defined in
// retok.hip; not part of the ABI.
__attribute__((visibility("hidden"))) int retok_enqueue_call(zett_retok* r, const uint8_t* token_chars, const int32_t* offsets, int64_t n_tokens,
                                                             int64_t n_text, int32_t maxlen, int32_t pad_id, int32_t* out, void* stream, LexPlan lex);

}  // namespace zett
