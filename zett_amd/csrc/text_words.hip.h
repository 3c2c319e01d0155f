// text_words.hip.h — the split of a batch of texts into words, shared by text_encode.hip (zett_encode_texts) and tokenizer_sample.hip
// (zett_sampler_sample): classify / walk, from the text bytes to a flag at every word start (scan.hip.h's compaction makes the word
// list woff[] of them).  Both entry points launch these kernels; the stages are described at the head of text_encode.hip.  Everything
// here has internal linkage: a translation unit that includes the header gets its own copy.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "../../include/zett_hip.h"

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

}  // namespace
