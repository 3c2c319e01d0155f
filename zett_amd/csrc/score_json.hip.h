// score_json.hip.h — what a float64 score becomes when the tokenizers library writes it to JSON and reads it back.
//
// The library writes the shortest decimal that reads back as the double (digits D, value D * 10^-s) and its reader computes
// (double)D / 10^s: two roundings where a correctly rounded reader has one, so about one score in nine comes back one ulp away.
// transformers' PreTrainedTokenizerFast rebuilds its backend through that JSON, so the model the host-built tokenizer segments with
// holds the re-read scores.  sampled_vocab.hip puts the same values into its table when the installed library behaves this way
// (zett_amd/sampled_vocab.py probes it; json_round_trip there is this function in Python, checked against the library).
//
// Exact integer arithmetic in 128 bits: for the first s = 0, 1, ... the nearest integer D to |x| * 10^s is tested for lying inside the
// interval of reals that round to x (half an ulp either way, a quarter below a power of two; the bounds count when the mantissa is
// even).  Values the 128 bits do not hold (|x| >= 2^53, more than 22 decimal places) and integers come back as they are.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#ifndef __host__
#define __host__
#define __device__
#endif
#endif

namespace zett {

__host__ __device__ inline uint64_t json_round_trip_bits(uint64_t bits) {
    typedef unsigned __int128 u128;
    const uint64_t mag = bits & ~(1ull << 63);
    const int be = (int)(mag >> 52);
    if (be == 0 || be == 0x7ff) return bits;                          // zero, subnormal, infinity, NaN
    const uint64_t m = (mag & ((1ull << 52) - 1)) | (1ull << 52);     // |x| = m * 2^-sh
    const int sh = 1075 - be;
    if (sh <= 0 || sh > 116) return bits;
    const bool even = (m & 1) == 0, pow2 = m == (1ull << 52);
    const u128 one = (u128)1 << sh;
    u128 p10 = 1;                                                     // 10^s
    for (int s = 0; s <= 22; ++s, p10 *= 10) {
        const u128 n = (u128)m * p10;                                 // |x| * 10^s * 2^sh  (< 2^53 * 2^74)
        const u128 fl = n >> sh, r = n & (one - 1);
        const u128 half = one >> 1;
        const bool up = r > half || (r == half && (fl & 1));
        const u128 d = fl + (up ? 1 : 0);
        if (d == 0) continue;
        const u128 err = up ? one - r : r;                            // |d * 2^sh - n|
        const u128 lim = p10;                                         // an ulp of x in these units
        const u128 e2 = (!up && pow2) ? err * 4 : err * 2;            // (err < 2^116: no overflow)
        if (!(e2 < lim || (even && e2 == lim))) continue;
        uint64_t dd = (uint64_t)d;
        int ss = s;
        while (ss > 0 && dd % 10 == 0) { dd /= 10; --ss; }
        if (ss == 0) return bits;                                     // an integer: read back exactly
        double p = 1.0;
        for (int i = 0; i < ss; ++i) p *= 10.0;
#ifdef __HIP_DEVICE_COMPILE__
        const double f = __ddiv_rn((double)dd, p);
#else
        const double f = (double)dd / p;
#endif
        uint64_t out;
        __builtin_memcpy(&out, &f, 8);
        return out | (bits & (1ull << 63));
    }
    return bits;
}

}  // namespace zett
