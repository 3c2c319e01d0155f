// text_words.hip.h — the word stage: the split of a batch of texts into words, shared by text_encode.hip (zett_encode_texts) and
// tokenizer_sample.hip (zett_sampler_sample).  The kernels (classify / walk, from the text bytes to a flag at every word start) and
// their host half: the layout of the stage's seven workspace arrays, the checks both entry points make, and the one launch sequence
// (with the cut step of zett_encode_texts_added between classify and walk: added tokens split out of the texts) that ends in scan.hip.h's compaction of the flags into the word list woff[].  The stages are described at the head of
// text_encode.hip.  Everything here has internal linkage: a translation unit that includes the header gets its own copy (of
// sample_mark_first_kernel too, whether it launches it or not).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/zett_hip.h"
#include "scan.hip.h"

namespace {

constexpr int64_t kMaxPositions = 1 << 30;
// a prefix mode of the sampler alone (zett_encode_texts refuses it): a U+0020 in front of EVERY text, the empty one included
constexpr int kPrefixEvenEmpty = 3;

// code byte of a position: class in bits 0-2, what the pattern asks about the character itself in bits 3-7
enum : int { C_O = 0, C_L = 1, C_M = 2, C_N = 3, C_S = 4, C_SKIP = 7 };
enum : int { A_NONE = 0, A_SPACE, A_APOS, A_s, A_t, A_m, A_d, A_r, A_v, A_l, A_e };

__device__ __forceinline__ int64_t clamp_off(int64_t o, int64_t n_text) { return o < 0 ? 0 : (o > n_text ? n_text : o); }

__global__ __launch_bounds__(256) void encode_classify_kernel(const uint8_t* __restrict__ text, const int64_t* __restrict__ off, int64_t b, int64_t n_text,
                                                              const uint8_t* __restrict__ table, int64_t n_cp, int prefix_mode, uint8_t* __restrict__ codes,
                                                              uint8_t* __restrict__ flags, uint8_t* __restrict__ raw, int* __restrict__ status) {
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (item >= n_text + b) return;
    if (item >= n_text) {                                             // the slot of text t
        const int64_t t = item - n_text;
        const int64_t lo = clamp_off(off[t], n_text), hi = clamp_off(off[t + 1], n_text);
        if (off[t] < 0 || off[t] > n_text || off[t + 1] < off[t] || (t == 0 && off[0] != 0) || (t == b - 1 && off[b] != n_text)) atomicOr(status, ZETT_ENCODE_BAD_OFFSETS);
        const bool prefixed = prefix_mode == kPrefixEvenEmpty || (hi > lo && (prefix_mode == ZETT_ENCODE_PREFIX_ALWAYS || (prefix_mode == ZETT_ENCODE_PREFIX_UNLESS_SPACE && text[lo] != 0x20)));
        const int64_t p = lo + t;
        raw[p] = 0x20;
        codes[p] = prefixed ? (uint8_t)(C_S | (A_SPACE << 3)) : (uint8_t)C_SKIP;
        flags[p] = prefixed ? 0 : 2;                                   // 2: a dead word (the walk marks the live slot itself)
        return;
    }
    int64_t lo = 0, hi = b - 1;                                       // the last text whose offset is <= item
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if (off[mid] <= item) lo = mid; else hi = mid - 1;
    }
    const int64_t p = item + lo + 1;
    const int c = text[item];
    raw[p] = (uint8_t)c;
    flags[p] = 0;
    if ((c & 0xC0) == 0x80) { codes[p] = C_SKIP; return; }          // continuation byte
    int need = c < 0x80 ? 0 : (c >= 0xF0 ? 3 : (c >= 0xE0 ? 2 : 1));
    int64_t cp = c < 0x80 ? c : (c >= 0xF0 ? (c & 0x07) : (c >= 0xE0 ? (c & 0x0F) : (c & 0x1F)));
    for (int k = 1; k <= need; ++k) {
        const int nb = item + k < n_text ? text[item + k] : 0;
        if ((nb & 0xC0) != 0x80) { cp = -1; break; }                  // not UTF-8: class O
        cp = (cp << 6) | (nb & 0x3F);
    }
    int cls = C_O;
    if (cp >= 0 && cp < n_cp) cls = (table[cp >> 1] >> ((cp & 1) * 4)) & 7;
    if (cls > C_S) cls = C_O;
    int a = A_NONE;
    switch (c) {
        case ' ': a = A_SPACE; break;
        case '\'': a = A_APOS; break;
        case 's': a = A_s; break;
        case 't': a = A_t; break;
        case 'm': a = A_m; break;
        case 'd': a = A_d; break;
        case 'r': a = A_r; break;
        case 'v': a = A_v; break;
        case 'l': a = A_l; break;
        case 'e': a = A_e; break;
        default: break;
    }
    codes[p] = (uint8_t)(cls | (a << 3));
}

// the next character start behind position i (hi: none)
__device__ __forceinline__ int64_t next_char(const uint8_t* __restrict__ codes, int64_t i, int64_t hi) {
    ++i;
    while (i < hi && (codes[i] & 7) == C_SKIP) ++i;
    return i;
}

// The end of the match that starts at i < hi (always > i).  The alternatives of the pattern in their order: a contraction; ` ?` and a
// run of letters (marks too if `marks`), of digits, or of anything that is not whitespace, letter or digit (marks always); whitespace
// not followed by non-whitespace (a run gives up its last character to the next match unless it ends the text); whitespace.
__device__ inline int64_t match_end(const uint8_t* __restrict__ codes, int64_t i, int64_t hi, int marks) {
    const int c = codes[i];
    if ((c >> 3) == A_APOS) {
        const int64_t j = next_char(codes, i, hi);
        if (j < hi) {
            const int a1 = codes[j] >> 3;
            if (a1 == A_s || a1 == A_t || a1 == A_m || a1 == A_d) return next_char(codes, j, hi);
            if (a1 == A_r || a1 == A_v || a1 == A_l) {
                const int64_t k = next_char(codes, j, hi);
                if (k < hi) {
                    const int a2 = codes[k] >> 3;
                    if (a2 == (a1 == A_l ? A_l : A_e)) return next_char(codes, k, hi);
                }
            }
        }
    }
    int64_t s = i;                                                   // where the run starts: behind an optional U+0020
    int cls = c & 7;
    if ((c >> 3) == A_SPACE) {
        const int64_t j = next_char(codes, i, hi);
        if (j < hi && (codes[j] & 7) != C_S) { s = j; cls = codes[j] & 7; }
    }
    if (cls == C_S) {
        int64_t last = s, j = next_char(codes, s, hi);
        while (j < hi && (codes[j] & 7) == C_S) { last = j; j = next_char(codes, j, hi); }
        if (j >= hi || last == s) return j;                            // the run ends the text, or is one character
        return last;
    }
    const int run = (cls == C_L || (cls == C_M && marks)) ? 0 : (cls == C_N ? 1 : 2);
    int64_t j = next_char(codes, s, hi);
    while (j < hi) {
        const int k = codes[j] & 7;
        const bool in = run == 0 ? (k == C_L || (k == C_M && marks)) : (run == 1 ? k == C_N : (k == C_O || k == C_M));
        if (!in) break;
        j = next_char(codes, j, hi);
    }
    return j;
}

__global__ __launch_bounds__(64) void encode_walk_kernel(const int64_t* __restrict__ off, int64_t b, int64_t n_text, const uint8_t* __restrict__ codes,
                                                         uint8_t* __restrict__ flags, int marks, int resplit) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= b) return;
    const int64_t lo = clamp_off(off[t], n_text), end = std::max(lo, clamp_off(off[t + 1], n_text));
    int64_t i = lo + t;
    const int64_t hi = end + t + 1;
    if (codes[i] == C_SKIP) ++i;                                      // no prefix: the slot is a dead word
    while (i < hi) {
        const int64_t e = match_end(codes, i, hi, marks);
        if (resplit) {                                                 // the word once more, on its own, with the plain pattern
            for (int64_t j = i; j < e; j = match_end(codes, j, e, 0)) flags[j] = 1;
        } else {
            flags[i] = 1;
        }
        i = e;
    }
}

// ---- the cut step: added tokens split out of the texts (zett_encode_texts_added alone) ------------------------------------------------
// The table: n tokens in strictly ascending byte order (a token before every longer one it starts), token k at
// bytes[offsets[k] .. offsets[k + 1]), each of 2 .. kMaxAddedBytes bytes.  A match [m, m + len) becomes one word of one id on its first
// len - 1 positions (flag 8); its LAST position is the slot of the section behind it — prefix space or dead word, as a text's slot.
constexpr int kMaxAdded = 512;              // tokens of a table
constexpr int kMaxAddedBytes = 64;          // bytes of a token
constexpr int kFlagAdded = 8;               // flags[]: the word is a split-out token, its table index + 1 in cand[]

struct AddedTable {
    const uint8_t* bytes;
    const int32_t* offsets;      // n + 1
    const int32_t* ids;          // n
    int32_t n, n_bytes;
};

__device__ __forceinline__ int added_off(const AddedTable& tb, int k) {
    const int o = tb.offsets[k];
    return o < 0 ? 0 : (o > tb.n_bytes ? tb.n_bytes : o);
}
__device__ __forceinline__ int added_len(const AddedTable& tb, int k) {
    const int n = added_off(tb, k + 1) - added_off(tb, k);
    return n < 0 ? 0 : (n > kMaxAddedBytes ? kMaxAddedBytes : n);
}
// byte d of token k; 0 behind its end
__device__ __forceinline__ int added_byte(const AddedTable& tb, int k, int d) { return d < added_len(tb, k) ? tb.bytes[added_off(tb, k) + d] : 0; }

// One workgroup: the table's checks (offsets from 0 to n_bytes, lengths, the order) and first[c] = the first token whose first byte is
// >= c (first[256] = n), which is where every search of the candidates kernel starts.
__global__ __launch_bounds__(256) void encode_added_prepare_kernel(AddedTable tb, int32_t* __restrict__ first, int* __restrict__ status) {
    const int tid = threadIdx.x;
    bool bad = tid == 0 && (tb.offsets[0] != 0 || tb.offsets[tb.n] != tb.n_bytes);
    for (int k = tid; k < tb.n; k += 256) {
        const int o0 = tb.offsets[k], n = tb.offsets[k + 1] - o0;
        if (o0 < 0 || o0 > tb.n_bytes || n < 2 || n > kMaxAddedBytes) bad = true;
        if (k + 1 < tb.n) {                                            // strictly below its successor
            const int la = added_len(tb, k), lb = added_len(tb, k + 1);
            int d = 0;
            while (d < la && d < lb && added_byte(tb, k, d) == added_byte(tb, k + 1, d)) ++d;
            if (d == lb || (d < la && added_byte(tb, k, d) > added_byte(tb, k + 1, d))) bad = true;
        }
    }
    if (bad) atomicOr(status, ZETT_ENCODE_BAD_TABLE);
    int lo = 0, hi = tb.n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (added_byte(tb, mid, 0) < tid) lo = mid + 1; else hi = mid;
    }
    first[tid] = lo;
    if (tid == 0) first[256] = tb.n;
}

// A thread per byte / slot: cand[p] = 1 + the longest token that matches at the byte and ends inside the byte's own text, 0: none.
// The tokens that share the d bytes read so far are a range of the sorted table; one of d bytes can only be its first.
__global__ __launch_bounds__(256) void encode_candidates_kernel(const uint8_t* __restrict__ text, const int64_t* __restrict__ off, int64_t b, int64_t n_text,
                                                                AddedTable tb, const int32_t* __restrict__ first, uint16_t* __restrict__ cand) {
    const int64_t item = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (item >= n_text + b) return;
    if (item >= n_text) { cand[clamp_off(off[item - n_text], n_text) + (item - n_text)] = 0; return; }
    int64_t tl = 0, th = b - 1;                                       // the last text whose offset is <= item
    while (tl < th) {
        const int64_t mid = (tl + th + 1) >> 1;
        if (off[mid] <= item) tl = mid; else th = mid - 1;
    }
    const int c = text[item];
    int lo = std::min(std::max(first[c], 0), (int)tb.n), hi = std::min(std::max(first[c + 1], lo), (int)tb.n);
    int best = 0;
    if (lo < hi) {
        const int64_t avail = clamp_off(off[tl + 1], n_text) - item;     // bytes up to the text's end
        for (int d = 1; lo < hi && d <= kMaxAddedBytes; ++d) {
            if (added_len(tb, lo) <= d) {
                best = lo + 1;
                if (++lo >= hi) break;
            }
            if (d >= avail) break;
            const int ch = text[item + d];
            int a = lo, z = hi;                                        // the first token whose byte d is >= ch
            while (a < z) {
                const int mid = (a + z) >> 1;
                if (added_byte(tb, mid, d) < ch) a = mid + 1; else z = mid;
            }
            lo = a;
            z = hi;                                                    // the first whose byte d is > ch
            while (a < z) {
                const int mid = (a + z) >> 1;
                if (added_byte(tb, mid, d) <= ch) a = mid + 1; else z = mid;
            }
            hi = a;
        }
    }
    cand[item + tl + 1] = (uint16_t)best;
}

// The walk with cuts, a lane per text: the leftmost candidate at or behind i is taken (the longest at its byte), what lies in front of
// it is walked as a text of its own behind slot s, and i moves behind the match — candidates inside it are never looked at.
__global__ __launch_bounds__(64) void encode_walk_cut_kernel(const int64_t* __restrict__ off, int64_t b, int64_t n_text, uint8_t* codes, uint8_t* flags, uint8_t* raw,
                                                             const uint16_t* __restrict__ cand, AddedTable tb, int prefix_mode, int marks, int resplit) {
    const int64_t t = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= b) return;
    const int64_t lo = clamp_off(off[t], n_text), end = std::max(lo, clamp_off(off[t + 1], n_text));
    const int64_t hi = end + t + 1;
    int64_t s = lo + t, q = s + 1;                                    // the section's slot and its first byte
    for (;;) {
        int64_t m = q;
        int k = 0;
        while (m < hi && (k = cand[m]) == 0) ++m;
        int len = 0;
        if (m < hi) {
            len = added_len(tb, std::min(k, (int)tb.n) - 1);
            if (len > hi - m) len = (int)(hi - m);
            if (len < 2) { m = hi; len = 0; }                          // (a table that failed its checks: nothing is cut)
        }
        const bool prefixed = m > q && (prefix_mode == ZETT_ENCODE_PREFIX_ALWAYS || (prefix_mode == ZETT_ENCODE_PREFIX_UNLESS_SPACE && raw[q] != 0x20));
        raw[s] = 0x20;
        codes[s] = prefixed ? (uint8_t)(C_S | (A_SPACE << 3)) : (uint8_t)C_SKIP;
        flags[s] = prefixed ? 0 : 2;
        int64_t i = prefixed ? s : q;
        while (i < m) {
            const int64_t e = match_end(codes, i, m, marks);
            if (resplit) {
                for (int64_t j = i; j < e; j = match_end(codes, j, e, 0)) flags[j] = 1;
            } else {
                flags[i] = 1;
            }
            i = e;
        }
        if (m >= hi) break;
        flags[m] = 1 | kFlagAdded;
        s = m + len - 1;
        q = m + len;
    }
}

// the sampler's extra step: the slot of every text starts the text's first word
__global__ __launch_bounds__(256) void sample_mark_first_kernel(const int64_t* __restrict__ off, int64_t b, int64_t n_text, uint8_t* __restrict__ flags) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t < b) flags[clamp_off(off[t], n_text) + t] = 5;
}

// ---- the host half ------------------------------------------------------------------------------------------------------------
// Bytes behind the np = n_text + n_texts positions of an array, for the kernels that read it 16 bytes at a time:
constexpr int64_t kCodeSlack = 16;          // codes, flags (the compaction's loads are 16 flags wide)
constexpr int64_t kRawSlack = 32;           // raw: 16 bytes of slack for the staging loads of the last wave (text_encode.hip's words kernel)

// the seven arrays of the stage as offsets into the caller's workspace (every array starts on a 16-byte boundary); the caller
// goes on taking its own arrays from the same Carve
struct WordLayout {
    int64_t codes, flags, raw, woff, segcnt, segoff, totals;
    int64_t np, nseg;          // positions, and their scan segments
};
inline WordLayout word_layout(zett::Carve& w, int64_t n_text, int64_t n_texts) {
    WordLayout L{};
    L.np = n_text + n_texts;
    L.nseg = zett::compact_segments(L.np);
    L.codes = w.take(L.np + kCodeSlack);
    L.flags = w.take(L.np + kCodeSlack);
    L.raw = w.take(L.np + kRawSlack);
    L.woff = w.take((L.np + 1) * 4);
    L.segcnt = w.take(L.nseg * 4);
    L.segoff = w.take(L.nseg * 4);
    L.totals = w.take(16);
    return L;
}

struct WordArrays {
    uint8_t *codes, *flags, *raw;
    int32_t *woff, *segcnt, *segoff, *totals;
    WordArrays(void* workspace, const WordLayout& L)
        : codes((uint8_t*)workspace + L.codes), flags((uint8_t*)workspace + L.flags), raw((uint8_t*)workspace + L.raw),
          woff((int32_t*)((char*)workspace + L.woff)), segcnt((int32_t*)((char*)workspace + L.segcnt)), segoff((int32_t*)((char*)workspace + L.segoff)),
          totals((int32_t*)((char*)workspace + L.totals)) {}
};

// `what`: the entry point's name for its call ("text encoding")
inline int shape_args(const char* what, int64_t n_text, int64_t n_texts) {
    if (n_text < 0 || n_texts < 0) return zett::fail(ZETT_E_INVALID, "%s needs n_text >= 0 bytes and n_texts >= 0 texts (n_text = %lld, n_texts = %lld)", what, (long long)n_text, (long long)n_texts);
    if (n_text + n_texts >= kMaxPositions) return zett::fail(ZETT_E_INVALID, "n_text + n_texts = %lld: a call takes fewer than 2^30 positions", (long long)(n_text + n_texts));
    return 0;
}

// the arguments both entry points pass on to the word stage; need_bytes: the entry point's whole workspace (shape_args came first)
inline int word_stage_args(const uint8_t* text, const int64_t* text_offsets, int64_t n_texts, int64_t n_text, const uint8_t* class_table, int64_t n_code_points,
                           const void* workspace, int64_t workspace_bytes, int64_t need_bytes, const int32_t* status) {
    if (!status || !class_table || n_code_points <= 0 || n_code_points > 0x110000) return zett::fail(ZETT_E_INVALID, "null status or class table, or a table of more than 0x110000 code points");
    if (n_texts == 0) return 0;
    if (!text_offsets || (n_text && !text)) return zett::fail(ZETT_E_INVALID, "null argument");
    if (!workspace || !zett::aligned(workspace, 16)) return zett::fail(ZETT_E_INVALID, "null or misaligned workspace (16 bytes)");
    if (workspace_bytes < need_bytes) return zett::fail(ZETT_E_INVALID, "the workspace holds %lld bytes, %lld are needed", (long long)workspace_bytes, (long long)need_bytes);
    return 0;
}

// the cut step's table and its two arrays in the caller's workspace: first int32 [257], cand uint16 [np]
struct AddedCut {
    AddedTable table;
    int32_t* first;
    uint16_t* cand;
};

// classify, (cut: the candidates of the added tokens,) walk, (mark_first: the sampler's flag on the first word of every text,) compact:
// a.woff[0 .. a.totals[0]] is the word list
inline void launch_word_stage(const uint8_t* text, const int64_t* text_offsets, int64_t n_texts, int64_t n_text, const uint8_t* class_table, int64_t n_code_points,
                              int prefix_mode, int marks, int resplit, bool mark_first, const WordLayout& L, const WordArrays& a, int32_t* status, hipStream_t st,
                              const AddedCut* cut = nullptr) {
    hipLaunchKernelGGL(encode_classify_kernel, dim3((unsigned)((L.np + 255) / 256)), dim3(256), 0, st, text, text_offsets, n_texts, n_text, class_table, n_code_points,
                       prefix_mode, a.codes, a.flags, a.raw, status);
    if (cut) {
        hipLaunchKernelGGL(encode_added_prepare_kernel, dim3(1), dim3(256), 0, st, cut->table, cut->first, status);
        hipLaunchKernelGGL(encode_candidates_kernel, dim3((unsigned)((L.np + 255) / 256)), dim3(256), 0, st, text, text_offsets, n_texts, n_text, cut->table,
                           (const int32_t*)cut->first, cut->cand);
        hipLaunchKernelGGL(encode_walk_cut_kernel, dim3((unsigned)((n_texts + 63) / 64)), dim3(64), 0, st, text_offsets, n_texts, n_text, a.codes, a.flags, a.raw,
                           (const uint16_t*)cut->cand, cut->table, prefix_mode, marks, resplit);
    } else {
        hipLaunchKernelGGL(encode_walk_kernel, dim3((unsigned)((n_texts + 63) / 64)), dim3(64), 0, st, text_offsets, n_texts, n_text, (const uint8_t*)a.codes, a.flags, marks, resplit);
    }
    if (mark_first) hipLaunchKernelGGL(sample_mark_first_kernel, dim3((unsigned)((n_texts + 255) / 256)), dim3(256), 0, st, text_offsets, n_texts, n_text, a.flags);
    zett::launch_compact(a.flags, L.np, a.woff, a.segcnt, a.segoff, a.totals, st);
}

}  // namespace
