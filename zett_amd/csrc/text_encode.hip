// text_encode.hip — a batch of texts to padded input_ids on the device (include/zett_hip.h, "text encoding"; the tokenizer call of the
// reference's Collator.encode, zett/collator.py:166-178).
//
// Positions.  Text t occupies bytes [off[t], off[t + 1]) of `text`; on the device every text gets one SLOT in front of it, so byte i of
// text t sits at position p = i + t + 1 of a space of nP = n_text + B positions and the slot of text t at off[t] + t.  The slot holds
// the prefix space (U+0020) when the prefix mode gives text t one, and is a dead word otherwise: either way it is a word boundary, so
// no word ever crosses from one text into the next, and a word's bytes (prefix included) are one contiguous range of `raw`.
//
//   classify   a thread per byte / slot: the byte into `raw`, and for a character start its class (the 4-bit class table) and what the
//              contractions and ` ?` need to know about it (apostrophe, U+0020, s t m d r v l e) into one code byte; flags zeroed
//   walk       a lane per text: the leftmost-first matches of the split pattern as a state machine over the code bytes; a flag at
//              every match start (ZETT_ENCODE_RESPLIT: every match is matched again, on its own, with the plain pattern).  Sequential by
//              definition: where a match starts depends on where the previous one ended
//   (cut)      zett_encode_texts_added with a table of added tokens, between classify and walk: a thread per byte finds the longest
//              token that matches there inside the byte's own text (the sorted table narrowed byte by byte), and the walk takes the
//              candidates leftmost-first, walks every section between two matches as a text of its own and flags the match as a word
//              of one id.  The match's last position is the slot of the section behind it, so no position is added
//   compact    the flags into the word list woff[] — scan.hip.h's count / scan / place: a wave owns 1024 positions, one workgroup
//              scans the segment counts
//              (these three are the word stage of text_words.hip.h — kernels, workspace layout and launches: tokenizer_sample.hip
//              begins with the same stage)
//   words      a lane per word: retok.hip.h's stage 2 (BPE merge / Unigram Viterbi) on the word's raw bytes, state in LDS or — a wave
//              with more than 4 KiB of text, a lane beyond the arena — in the global scratch.  A word of b bytes gives at most 2b ids
//              (a byte is at least one symbol, byte fallback makes at most two ids of it), so word w writes at ids[2 * woff[w]]: no
//              second pass, no compaction, and the count per word is all the pack needs
//   pack       a wave per text: scan of the word counts, the row staged in LDS (prefix, ids up to the cut, suffix, pads), the id map,
//              then the row and its mask written with 16-byte stores where the output allows
//
// Integers only; the only atomic is the OR into the status word.  Every index derived from text_offsets is clamped before it is used.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/zett_hip.h"
#include "retok.hip.h"
#include "text_words.hip.h"

using namespace zett;

namespace {

constexpr int kMaxBlock = 8192;             // block_size: the row is staged in LDS
constexpr int kMaxTemplate = ZETT_ENCODE_MAX_TEMPLATE;
constexpr int kMaxMap = ZETT_SPLICE_MAX_ROWS;
constexpr int kScrPerByte = SCR_PER_BYTE + SCR_FIXED;      // a word starts at or behind its index: one factor covers both terms of the retokenizer's bound

struct Lists {
    int32_t n_prefix, n_suffix, n_map, pad_id;
    int32_t prefix[kMaxTemplate], suffix[kMaxTemplate];
    int32_t map_from[kMaxMap], map_to[kMaxMap];
};
static_assert(sizeof(Lists) < 4096 - 512, "the lists must fit the kernel-argument limit");

// workspace, in bytes: the word stage, then what the words and pack kernels add (every array starts on a 16-byte boundary)
struct Layout {
    WordLayout words;
    int64_t counts, ids, scratch, first, cand, bytes;
};
// added: the cut step's two arrays behind everything else (what comes before them does not move)
Layout layout(int64_t n_text, int64_t b, bool added = false) {
    Layout L{};
    Carve w;
    L.words = word_layout(w, n_text, b);
    const int64_t np = L.words.np;
    L.counts = w.take(np * 4);
    L.ids = w.take(np * 8);                         // 2 ids per position
    L.scratch = w.take((np * kScrPerByte + 64) * 4);
    if (added) {
        L.first = w.take(257 * 4);
        L.cand = w.take(np * 2);
    }
    L.bytes = w.bytes;
    return L;
}

// Stage 2 of the retokenizer, a lane per word (retok_tokens_kernel's shape): no special-token lookup, no byte table — the word's bytes
// are the text's bytes.  ids of word w at ids[2 * woff[w] ...), its count in counts[w].  ADDED: a word with kFlagAdded is a split-out
// token and gives its one id from the table.
template <bool ADDED>
__global__ __launch_bounds__(64) void encode_words_kernel(RetokTables t, const uint8_t* __restrict__ raw, const uint8_t* __restrict__ flags,
                                                          const int32_t* __restrict__ woff, const int32_t* __restrict__ totals, int32_t* __restrict__ ids,
                                                          int32_t* __restrict__ counts, int32_t* __restrict__ scratch, int* __restrict__ status,
                                                          const uint16_t* __restrict__ cand, const int32_t* __restrict__ added_ids, int n_added) {
    __shared__ RetokLds L;
    __shared__ __attribute__((aligned(16))) uint8_t s_text[RT_TEXT_BYTES + 16];
    __shared__ __attribute__((aligned(8))) int32_t s_arena[RT_ARENA_WORDS];
    const int64_t n_words = totals[0];
    const int64_t tok0 = (int64_t)blockIdx.x * 64;
    if (tok0 >= n_words) return;                                       // (uniform) the grid is sized for a word per position
    const int lane = threadIdx.x;
    for (int i = lane; i < 256; i += 64) { L.single_id[i] = t.single_id[i]; L.bf_ids[i] = t.bf_ids[i]; }
    const int64_t tok = tok0 + lane;
    const bool live = tok < n_words;
    const int o0 = live ? woff[tok] : 0;
    const int len = live ? woff[tok + 1] - o0 : 0;
    const int w_lo = woff[tok0];
    const int w_hi = woff[tok0 + 64 < n_words ? tok0 + 64 : n_words];
    const int mis = w_lo & 15;
    const bool text_lds = (w_hi - w_lo) + mis <= RT_TEXT_BYTES;
    if (text_lds)
        for (int i = lane * 16; i < (w_hi - w_lo) + mis; i += 64 * 16) *(uint4*)(s_text + i) = *(const uint4*)(raw + (w_lo - mis) + i);
    __syncthreads();
    const lds_u8* sl = (const lds_u8*)s_text + mis + (o0 - w_lo);
    const uint8_t* sg = raw + o0;
    RowWriter w{ids + 2 * (int64_t)o0, 2 * len, 0};
    bool todo = live && len > 0 && !(flags[o0] & 2);
    if (ADDED && todo && (flags[o0] & kFlagAdded)) {
        const int k = cand[o0];
        w.push(added_ids[(k < 1 ? 1 : (k > n_added ? n_added : k)) - 1]);
        todo = false;
    }
    if (todo && t.kind == ZETT_RETOK_BPE && t.ignore_merges) {
        const int id = text_lds ? whole_token_id<LdsMem>(t.pieces, t.piece_mask, t.piece_blob, sl, len)
                                : whole_token_id<GlobalMem>(t.pieces, t.piece_mask, t.piece_blob, sg, len);
        if (id >= 0) { w.push(id); todo = false; }
    }
    int n_sym = 0, need = 0;
    if (todo) {
        if (t.kind == ZETT_RETOK_BPE) {
            n_sym = text_lds ? bpe_symbols<false, LdsMem>(t, L, sl, len, (lds_i32*)nullptr) : bpe_symbols<false, GlobalMem>(t, L, sg, len, (int32_t*)nullptr);
            need = bpe_state_words(n_sym);
        } else {
            need = unigram_state_words(len);
        }
        need = (need + 1) & ~1;                                        // regions start on 8-byte boundaries
    }
    const int a0 = wave_inclusive_scan(need) - need;
    if (todo) {
        bool ok;
        if (text_lds && a0 + need <= RT_ARENA_WORDS) {
            ok = segment_token<LdsMem>(t, L, sl, len, n_sym, (lds_i32*)s_arena + a0, w, 0);
        } else {
            int32_t* scr = scratch + (int64_t)o0 * kScrPerByte;
            ok = segment_token<GlobalMem>(t, L, sg, len, n_sym, scr, w, 0);
        }
        if (!ok) {                                                     // the library raises: an unknown piece and no unk id
            atomicOr(status, ZETT_ENCODE_NO_UNK);
            w.n = 0;
        }
    }
    if (live) counts[tok] = w.n < 2 * len ? w.n : 2 * len;
}

// the first word that starts at or behind position p
__device__ __forceinline__ int64_t first_word_at(const int32_t* __restrict__ woff, int64_t n_words, int64_t p) {
    int64_t lo = 0, hi = n_words;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (woff[mid] < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ int32_t map_id(const Lists& ls, int32_t v) {
    for (int m = 0; m < ls.n_map; ++m)                                 // in order, as the reference's loop of assignments
        if (v == ls.map_from[m]) v = ls.map_to[m];
    return v;
}

// A wave per text.  WIDE: int64 outputs.  VEC: 16-byte stores (the launcher checked the row length, the row stride and the pointers).
template <bool WIDE, bool VEC>
__global__ __launch_bounds__(64) void encode_pack_kernel(const int64_t* __restrict__ off, int64_t b, int64_t n_text, const int32_t* __restrict__ woff,
                                                         const int32_t* __restrict__ totals, const int32_t* __restrict__ counts, const int32_t* __restrict__ ids,
                                                         int block, const Lists ls, void* __restrict__ out_ids, void* __restrict__ out_mask, int64_t ld_out) {
    extern __shared__ int32_t s_row[];
    const int lane = threadIdx.x;
    const int64_t n_words = totals[0];
    const int cap = block - ls.n_prefix - ls.n_suffix;
    for (int64_t t = blockIdx.x; t < b; t += gridDim.x) {
        const int64_t p0 = clamp_off(off[t], n_text) + t;
        const int64_t p1 = t + 1 < b ? clamp_off(off[t + 1], n_text) + t + 1 : n_text + b;
        const int64_t w0 = first_word_at(woff, n_words, p0), w1 = first_word_at(woff, n_words, p1);
        for (int j = lane; j < block; j += 64) s_row[j] = ls.pad_id;
        __syncthreads();
        int64_t base = 0;                                              // ids of the words before this round
        for (int64_t wb = w0; wb < w1 && base < cap; wb += 64) {
            const int64_t w = wb + lane;
            int k = 0, at = 0;
            if (w < w1) {
                at = woff[w];
                k = std::max(0, std::min(counts[w], 2 * (woff[w + 1] - at)));
            }
            const int inc = wave_inclusive_scan(k);
            const int64_t e = base + inc - k;
            const int32_t* src = ids + 2 * (int64_t)at;
            for (int q = 0; q < k && e + q < cap; ++q) s_row[ls.n_prefix + e + q] = src[q];      // (a word may be cut in the middle)
            base += __shfl(inc, 63, 64);
        }
        const int total = (int)std::min<int64_t>(base, cap);
        __syncthreads();
        if (lane == 0) {
            for (int i = 0; i < ls.n_prefix; ++i) s_row[i] = ls.prefix[i];
            for (int i = 0; i < ls.n_suffix; ++i) s_row[ls.n_prefix + total + i] = ls.suffix[i];
        }
        __syncthreads();
        const int n_real = ls.n_prefix + total + ls.n_suffix;
        if (VEC) {
            constexpr int per = WIDE ? 2 : 4;
            uint4* oi = (uint4*)((char*)out_ids + t * ld_out * (WIDE ? 8 : 4));
            uint4* om = (uint4*)((char*)out_mask + t * ld_out * (WIDE ? 8 : 4));
            for (int u = lane; u < block / per; u += 64) {
                int32_t v[per], m[per];
#pragma unroll
                for (int k = 0; k < per; ++k) { v[k] = map_id(ls, s_row[u * per + k]); m[k] = u * per + k < n_real; }
                if (WIDE) {
                    oi[u] = make_uint4((uint32_t)v[0], (uint32_t)(v[0] >> 31), (uint32_t)v[per - 1], (uint32_t)(v[per - 1] >> 31));
                    om[u] = make_uint4((uint32_t)m[0], 0u, (uint32_t)m[per - 1], 0u);
                } else {
                    oi[u] = make_uint4((uint32_t)v[0], (uint32_t)v[1 % per], (uint32_t)v[2 % per], (uint32_t)v[3 % per]);
                    om[u] = make_uint4((uint32_t)m[0], (uint32_t)m[1 % per], (uint32_t)m[2 % per], (uint32_t)m[3 % per]);
                }
            }
        } else {
            for (int j = lane; j < block; j += 64) {
                const int32_t v = map_id(ls, s_row[j]);
                if (WIDE) {
                    ((int64_t*)out_ids)[t * ld_out + j] = v;
                    ((int64_t*)out_mask)[t * ld_out + j] = j < n_real;
                } else {
                    ((int32_t*)out_ids)[t * ld_out + j] = v;
                    ((int32_t*)out_mask)[t * ld_out + j] = j < n_real;
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" {

int zett_encode_workspace_bytes(int64_t n_text, int64_t n_texts, int64_t* bytes) {
    if (int rc = shape_args("text encoding", n_text, n_texts)) return rc;
    if (!bytes) return fail(ZETT_E_INVALID, "null argument");
    *bytes = layout(n_text, n_texts).bytes;
    return 0;
}

int zett_encode_added_workspace_bytes(int64_t n_text, int64_t n_texts, int32_t n_added, int64_t* bytes) {
    if (int rc = shape_args("text encoding", n_text, n_texts)) return rc;
    if (!bytes) return fail(ZETT_E_INVALID, "null argument");
    if (n_added < 0 || n_added > kMaxAdded) return fail(ZETT_E_INVALID, "%d added tokens: a table holds at most %d", (int)n_added, kMaxAdded);
    *bytes = layout(n_text, n_texts, n_added > 0).bytes;
    return 0;
}

int zett_encode_texts(zett_retok* r, const uint8_t* text, const int64_t* text_offsets, int64_t n_texts, int64_t n_text, const uint8_t* class_table,
                      int64_t n_code_points, int32_t flags, int32_t prefix_mode, int32_t block_size, const int32_t* prefix_ids, int32_t n_prefix,
                      const int32_t* suffix_ids, int32_t n_suffix, const int32_t* map_from, const int32_t* map_to, int32_t n_map, int32_t pad_id, void* input_ids,
                      void* attention_mask, int32_t out_bytes, int64_t ld_out, void* workspace, int64_t workspace_bytes, int32_t* status, void* stream) {
    return zett_encode_texts_added(r, text, text_offsets, n_texts, n_text, class_table, n_code_points, flags, prefix_mode, block_size, prefix_ids, n_prefix, suffix_ids,
                                   n_suffix, map_from, map_to, n_map, pad_id, input_ids, attention_mask, out_bytes, ld_out, nullptr, nullptr, nullptr, 0, 0, workspace,
                                   workspace_bytes, status, stream);
}

int zett_encode_texts_added(zett_retok* r, const uint8_t* text, const int64_t* text_offsets, int64_t n_texts, int64_t n_text, const uint8_t* class_table,
                      int64_t n_code_points, int32_t flags, int32_t prefix_mode, int32_t block_size, const int32_t* prefix_ids, int32_t n_prefix,
                      const int32_t* suffix_ids, int32_t n_suffix, const int32_t* map_from, const int32_t* map_to, int32_t n_map, int32_t pad_id, void* input_ids,
                      void* attention_mask, int32_t out_bytes, int64_t ld_out, const uint8_t* added_bytes, const int32_t* added_offsets, const int32_t* added_ids,
                      int32_t n_added, int32_t n_added_bytes, void* workspace, int64_t workspace_bytes, int32_t* status, void* stream) {
    if (!r) return fail(ZETT_E_INVALID, "null argument");
    if (!r->tokenizes()) return fail(ZETT_E_STATE, "the handle's tables are built on the device: zett_sampled_vocab_build and zett_sampled_vocab_commit come first");
    if (r->t.kind != ZETT_RETOK_BPE && r->t.kind != ZETT_RETOK_UNIGRAM)
        return fail(ZETT_E_NOT_IMPLEMENTED, "text encoding segments with a BPE or a Unigram model (WordPiece targets need another pre-tokenizer)");
    if (int rc = shape_args("text encoding", n_text, n_texts)) return rc;
    if (flags & ~(ZETT_ENCODE_MARKS_ARE_LETTERS | ZETT_ENCODE_RESPLIT)) return fail(ZETT_E_INVALID, "unknown flags 0x%x", (unsigned)flags);
    if (prefix_mode != ZETT_ENCODE_PREFIX_NONE && prefix_mode != ZETT_ENCODE_PREFIX_ALWAYS && prefix_mode != ZETT_ENCODE_PREFIX_UNLESS_SPACE)
        return fail(ZETT_E_INVALID, "unknown prefix mode %d", (int)prefix_mode);
    if (block_size < 1 || block_size > kMaxBlock) return fail(ZETT_E_INVALID, "block_size = %d must be in [1, %d]", (int)block_size, kMaxBlock);
    if (n_prefix < 0 || n_prefix > kMaxTemplate || n_suffix < 0 || n_suffix > kMaxTemplate)
        return fail(ZETT_E_INVALID, "%d prefix and %d suffix ids: at most %d each travel with a launch", (int)n_prefix, (int)n_suffix, kMaxTemplate);
    if (block_size <= n_prefix + n_suffix)
        return fail(ZETT_E_INVALID, "block_size = %d leaves no room for the text behind %d template ids", (int)block_size, (int)(n_prefix + n_suffix));
    if (n_map < 0 || n_map > kMaxMap) return fail(ZETT_E_INVALID, "%d id pairs are listed, at most %d travel with a launch", (int)n_map, kMaxMap);
    if ((n_prefix && !prefix_ids) || (n_suffix && !suffix_ids) || (n_map && (!map_from || !map_to))) return fail(ZETT_E_INVALID, "null argument");
    if (out_bytes != 4 && out_bytes != 8) return fail(ZETT_E_INVALID, "input_ids and attention_mask must be int32 or int64");
    if (ld_out < block_size) return fail(ZETT_E_INVALID, "ld_out = %lld must be at least block_size = %d", (long long)ld_out, (int)block_size);
    if (n_texts && (!input_ids || !attention_mask)) return fail(ZETT_E_INVALID, "null argument");
    if (n_texts && (!aligned(input_ids, out_bytes) || !aligned(attention_mask, out_bytes))) return fail(ZETT_E_INVALID, "misaligned output");
    if (n_added < 0 || n_added > kMaxAdded) return fail(ZETT_E_INVALID, "%d added tokens: a table holds at most %d", (int)n_added, kMaxAdded);
    if (n_added && (!added_bytes || !added_offsets || !added_ids)) return fail(ZETT_E_INVALID, "null argument");
    if (n_added && (n_added_bytes < 2 * n_added || n_added_bytes > kMaxAddedBytes * n_added))
        return fail(ZETT_E_INVALID, "%d bytes for %d added tokens: a token has 2 to %d bytes", (int)n_added_bytes, (int)n_added, kMaxAddedBytes);
    if (n_added && !aligned(added_offsets, 4)) return fail(ZETT_E_INVALID, "misaligned added_offsets");
    if (n_added && !aligned(added_ids, 4)) return fail(ZETT_E_INVALID, "misaligned added_ids");
    Lists ls{};
    ls.n_prefix = n_prefix; ls.n_suffix = n_suffix; ls.n_map = n_map; ls.pad_id = pad_id;
    for (int i = 0; i < n_prefix; ++i) ls.prefix[i] = prefix_ids[i];
    for (int i = 0; i < n_suffix; ++i) ls.suffix[i] = suffix_ids[i];
    for (int i = 0; i < n_map; ++i) { ls.map_from[i] = map_from[i]; ls.map_to[i] = map_to[i]; }
    const Layout L = layout(n_text, n_texts, n_added > 0);
    if (int rc = word_stage_args(text, text_offsets, n_texts, n_text, class_table, n_code_points, workspace, workspace_bytes, L.bytes, status)) return rc;
    ZETT_ON_DEVICE(r->device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(status, 0, 4, st));
    if (n_texts == 0) return 0;

    const WordArrays a(workspace, L.words);
    int32_t* counts = (int32_t*)((char*)workspace + L.counts);
    int32_t* ids = (int32_t*)((char*)workspace + L.ids);
    int32_t* scratch = (int32_t*)((char*)workspace + L.scratch);
    const AddedCut cut{AddedTable{added_bytes, added_offsets, added_ids, n_added, n_added_bytes}, (int32_t*)((char*)workspace + L.first), (uint16_t*)((char*)workspace + L.cand)};
    launch_word_stage(text, text_offsets, n_texts, n_text, class_table, n_code_points, (int)prefix_mode, (flags & ZETT_ENCODE_MARKS_ARE_LETTERS) != 0,
                      (flags & ZETT_ENCODE_RESPLIT) != 0, false, L.words, a, status, st, n_added ? &cut : nullptr);
#define ZETT_WORDS(ADDED)                                                                                                                                          \
    hipLaunchKernelGGL(encode_words_kernel<ADDED>, dim3((unsigned)((L.words.np + 63) / 64)), dim3(64), 0, st, r->t, (const uint8_t*)a.raw, (const uint8_t*)a.flags, \
                       (const int32_t*)a.woff, (const int32_t*)a.totals, ids, counts, scratch, status, (const uint16_t*)cut.cand, added_ids, (int)n_added)
    if (n_added) ZETT_WORDS(true); else ZETT_WORDS(false);
#undef ZETT_WORDS
    const int per = out_bytes == 8 ? 2 : 4;
    const bool vec = block_size % per == 0 && ld_out % per == 0 && aligned(input_ids, 16) && aligned(attention_mask, 16);
    const size_t lds = (size_t)block_size * 4;
#define ZETT_PACK(WIDE, VEC)                                                                                                                                       \
    hipLaunchKernelGGL((encode_pack_kernel<WIDE, VEC>), dim3(grid_for(n_texts, 1 << 16)), dim3(64), lds, st, text_offsets, n_texts, n_text, (const int32_t*)a.woff, \
                       (const int32_t*)a.totals, (const int32_t*)counts, (const int32_t*)ids, (int)block_size, ls, input_ids, attention_mask, ld_out)
    if (out_bytes == 8) { if (vec) ZETT_PACK(true, true); else ZETT_PACK(true, false); }
    else { if (vec) ZETT_PACK(false, true); else ZETT_PACK(false, false); }
#undef ZETT_PACK
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
