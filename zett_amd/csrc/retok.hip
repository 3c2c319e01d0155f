// retok.hip — the retokenizer's own translation unit: get_surface_form_matrix on the device behind the zett_retok_* entry points
// (include/zett_hip.h).  retok.hip.h has the design, the tables and the per-token segmentation, which text_encode.hip,
// sampled_vocab.hip and lexical.hip share; here are the kernels only these entry points launch — the raw offsets of the tokens,
// the pad fill and the two stage-2 kernels (a lane per token; for Unigram models a workgroup per 64 tokens) — and the host side:
// create / destroy, the enqueue of one call (retok_enqueue_call, which zett_lexical_plan calls too) and the result query.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "common.hip.h"
#include "retok.hip.h"
#include "scan.hip.h"

namespace zett {

__global__ void token_raw_offsets_kernel(const int32_t* __restrict__ offsets, int64_t n_tokens, int64_t n_text,
                                         const uint32_t* __restrict__ raw_pos, const int32_t* __restrict__ blk_scan,
                                         int n_blocks, int32_t* __restrict__ raw_off) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tokens) return;
    const int64_t o = offsets[t];
    raw_off[t] = (o >= n_text) ? blk_scan[n_blocks] : (int32_t)raw_pos[o];
}

__global__ void fill_i32_kernel(int32_t* __restrict__ p, int64_t n, int32_t v) {
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) p[i] = v;
}

__global__ __launch_bounds__(64) void retok_tokens_kernel(RetokTables t, const uint8_t* __restrict__ raw,
                                                          const int32_t* __restrict__ raw_off, int64_t n_tokens,
                                                          int maxlen, int32_t pad_id, int32_t* __restrict__ out, int32_t* __restrict__ scratch,
                                                          unsigned long long* __restrict__ n_truncated,
                                                          unsigned long long* __restrict__ err_unk, uint32_t call, LexPlan lex) {
    __shared__ RetokLds L;
    __shared__ __attribute__((aligned(16))) uint8_t s_text[RT_TEXT_BYTES + 16];
    __shared__ __attribute__((aligned(8))) int32_t s_arena[RT_ARENA_WORDS];
    const int lane = threadIdx.x;
    for (int i = lane; i < 256; i += 64) { L.single_id[i] = t.single_id[i]; L.bf_ids[i] = t.bf_ids[i]; }
    const int64_t tok0 = (int64_t)blockIdx.x * 64;
    const int64_t tok = tok0 + lane;
    const bool live = tok < n_tokens;
    const int o0 = live ? raw_off[tok] : 0;
    const int len = live ? raw_off[tok + 1] - o0 : 0;
    // the wave's text: bytes [w_lo, w_hi) of `raw`, staged from the 16-byte boundary below w_lo (the buffer has 16 bytes of slack)
    const int w_lo = raw_off[tok0];
    const int w_hi = raw_off[tok0 + 64 < n_tokens ? tok0 + 64 : n_tokens];
    const int mis = w_lo & 15;
    const bool text_lds = (w_hi - w_lo) + mis <= RT_TEXT_BYTES;
    if (text_lds)
        for (int i = lane * 16; i < (w_hi - w_lo) + mis; i += 64 * 16) *(uint4*)(s_text + i) = *(const uint4*)(raw + (w_lo - mis) + i);
    __syncthreads();
    RETOK_STOP(1);
    const lds_u8* sl = (const lds_u8*)s_text + mis + (o0 - w_lo);
    const uint8_t* sg = raw + o0;
    RowWriter w{out + tok * maxlen, maxlen, 0};
    if (lex.counts && lex.mode) w.drop_from = lex.n_rows;
    bool todo = live && len > 0, exact = false;
    if (todo && t.special_mask != 0xffffffffu) {              // zett/utils.py:671-673
        const int id = text_lds ? whole_token_id<LdsMem>(t.specials, t.special_mask, t.special_blob, sl, len)
                                : whole_token_id<GlobalMem>(t.specials, t.special_mask, t.special_blob, sg, len);
        if (id >= 0 && (!lex.counts || id < lex.n_rows)) { w.row[0] = id; todo = false; exact = true; }
    }
    if (lex.counts && lex.mode == 0) todo = false;
    if (todo && t.kind == ZETT_RETOK_BPE && t.ignore_merges) {
        const int id = text_lds ? whole_token_id<LdsMem>(t.pieces, t.piece_mask, t.piece_blob, sl, len)
                                : whole_token_id<GlobalMem>(t.pieces, t.piece_mask, t.piece_blob, sg, len);
        if (id >= 0) { w.push(id); todo = false; }
    }
    RETOK_STOP(2);
    // state of the token, and its place in the wave's arena: an exclusive wavefront scan over the 64 sizes
    int n_sym = 0, need = 0;
    if (todo) {
        if (t.kind == ZETT_RETOK_BPE) {
            n_sym = text_lds ? bpe_symbols<false, LdsMem>(t, L, sl, len, (lds_i32*)nullptr) : bpe_symbols<false, GlobalMem>(t, L, sg, len, (int32_t*)nullptr);
            need = bpe_state_words(n_sym);
        } else if (t.kind == ZETT_RETOK_UNIGRAM) {
            need = unigram_state_words(len);
        }
        need = (need + 1) & ~1;                                // regions start on 8-byte boundaries
    }
    const int a0 = wave_inclusive_scan(need) - need;
    RETOK_STOP(3);
    if (todo) {
        bool ok;
        if (text_lds && a0 + need <= RT_ARENA_WORDS) {
            ok = segment_token<LdsMem>(t, L, sl, len, n_sym, (lds_i32*)s_arena + a0, w, pad_id);
        } else {
            int32_t* scr = scratch + ((int64_t)o0 * SCR_PER_BYTE + tok * SCR_FIXED);
            ok = segment_token<GlobalMem>(t, L, sg, len, n_sym, scr, w, pad_id);
        }
        if (!ok) {
            atomicMin(err_unk, ((unsigned long long)call << 32) | (uint32_t)(tok < 0x7ffffffe ? tok : 0x7ffffffe));      // earliest call, then earliest token
            return;
        }
        if (w.n > maxlen) atomicAdd(n_truncated, 1ull);      // zett/utils.py:683-685
    }
    if (lex.counts && live) lex.counts[tok] = exact ? 1 : lex.count_of(w);
}

// ---------------------------------------------------------------------------------------
// stage 2 for Unigram models (r6): a WORKGROUP per 64 tokens — the piece lookups by all four waves, the Viterbi walk by lane
// ---------------------------------------------------------------------------------------
// The one-lane-per-token kernel above runs a Unigram token as len starts x up to max_piece_len ends of DEPENDENT table probes
// (a 32-byte entry of a 16 MiB table: an L2 / MALL miss, ~1-2 us), and a wave's 64 lanes walk tokens of different lengths in
// lockstep: 0.25 ms for the 50 k tokens of XLM-R -> GPT-2 whatever the occupancy (NOTEBOOK R5.5).  But the lookups do not depend
// on the lattice at all — only the score accumulation does.  So:
//   phase 0  (wave 0, a lane per token) special-token lookup, sizes: the token's (start, end) table has len x W slots,
//            W = min(len, max_piece_len); a wavefront scan places the tables of the 64 tokens in one LDS array
//   phase 1  (256 threads) the slots of all tokens as ONE flat work list: thread -> (token, start, end) by a binary search over
//            the 65 prefix sums, FNV hash of the substring from the staged text, first table entries of four slots fetched
//            together, then resolved; (id, score) or a miss into the slot.  Every probe of the workgroup is in flight at once:
//            ~9 slots per thread instead of ~150 dependent round trips per lane
//   phase 2  (wave 0, a lane per token) unigram_token_table: the same walk on LDS reads, then the same emission
// Tokens whose tables do not fit the 4 096 slots together are processed in rounds; a token that alone exceeds them, and a
// workgroup whose text does not fit its LDS stage, take the per-lane code.  Integer results, same visiting order: identical ids.
constexpr int UG_THREADS = 256;
constexpr int UG_TOKENS = 64;
constexpr int UG_PCAP = 4096;

// (r6) the same Viterbi walk when every (start, end) lookup of the token has already been made by the workgroup
// (retok_unigram_kernel, phase 1): slot s * W + k of the token's table holds the piece of bytes [s, s + 1 + k) — its id (UG_MISS:
// no such piece) and score.  Same visiting order, same strictly-greater updates, same double additions as unigram_token.
constexpr int32_t UG_MISS = -0x7fffffff - 1;
template <typename M>
__device__ inline bool unigram_token_table(const RetokTables& t, const RetokLds& L, typename M::bytes raw, int len, typename M::words scr, RowWriter& w,
                                           const lds_i32* pid, const lds_f64* pscore, int W) {
    typename M::doubles best = (typename M::doubles)scr;
    typename M::words bstart = scr + 2 * (len + 1);
    typename M::words bid = bstart + len + 1;
    typename M::words fwd = bid + len + 1;
    for (int i = 0; i <= len; ++i) { best[i] = 0.0; bstart[i] = -1; bid[i] = -1; }
    for (int s = 0; s < len; ++s) {
        const double base = best[s];
        bool has_single = false;
        const int kmax = (len - s < W) ? len - s : W;
        // four ends of the start at a time: their table slots and lattice cells are read TOGETHER (distinct ends: no two of the
        // four updates touch the same cell), then compared and written — the walk is a chain of LDS latencies otherwise
        for (int k0 = 0; k0 < kmax; k0 += 4) {
            int32_t id[4];
            double sc[4], be[4];
            int bs[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = k0 + k < kmax;
                const int slot = s * W + (in ? k0 + k : k0), e = s + 1 + (in ? k0 + k : k0);
                id[k] = in ? pid[slot] : UG_MISS;
                sc[k] = pscore[slot];
                be[k] = best[e];
                bs[k] = bstart[e];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (id[k] == UG_MISS) continue;
                const int e = s + 1 + k0 + k;
                const double cand = sc[k] + base;
                if (bs[k] == -1 || cand > be[k]) { best[e] = cand; bstart[e] = s; bid[e] = id[k]; }
                if (k0 + k == 0) has_single = true;
            }
        }
        if (!has_single) {
            if (t.unk_id < 0) return false;
            const double cand = t.unk_score + base;
            const int e = s + 1;
            if (bstart[e] == -1 || cand > best[e]) { best[e] = cand; bstart[e] = s; bid[e] = -2; }
        }
    }
#ifdef ZETT_RETOK_DEBUG
    if (t.debug_stop == 4) return true;
#endif
    unigram_emit<M>(t, L, raw, len, bstart, bid, fwd, w);
    return true;
}

__global__ __launch_bounds__(UG_THREADS) void retok_unigram_kernel(RetokTables t, const uint8_t* __restrict__ raw,
                                                                   const int32_t* __restrict__ raw_off, int64_t n_tokens,
                                                                   int maxlen, int32_t pad_id, int32_t* __restrict__ out, int32_t* __restrict__ scratch,
                                                                   unsigned long long* __restrict__ n_truncated,
                                                                   unsigned long long* __restrict__ err_unk, uint32_t call, LexPlan lex) {
    __shared__ RetokLds L;
    __shared__ __attribute__((aligned(16))) uint8_t s_text[RT_TEXT_BYTES + 16];
    __shared__ __attribute__((aligned(8))) int32_t s_arena[RT_ARENA_WORDS];
    __shared__ __attribute__((aligned(8))) double s_pscore[UG_PCAP];
    __shared__ int32_t s_pid[UG_PCAP];
    __shared__ int s_base[UG_TOKENS + 1];          // first slot of every token's table (0 slots: nothing to segment)
    __shared__ int s_len[UG_TOKENS], s_toff[UG_TOKENS];
    const int tid = threadIdx.x, lane = tid & 63;
    const bool wave0 = tid < 64;
    for (int i = tid; i < 256; i += UG_THREADS) { L.single_id[i] = t.single_id[i]; L.bf_ids[i] = t.bf_ids[i]; }
    const int64_t tok0 = (int64_t)blockIdx.x * UG_TOKENS;
    const int64_t tok = tok0 + lane;
    const bool live = wave0 && tok < n_tokens;
    const int o0 = live ? raw_off[tok] : 0;
    const int len = live ? raw_off[tok + 1] - o0 : 0;
    const int w_lo = raw_off[tok0];
    const int w_hi = raw_off[tok0 + UG_TOKENS < n_tokens ? tok0 + UG_TOKENS : n_tokens];
    const int mis = w_lo & 15;
    const bool text_lds = (w_hi - w_lo) + mis <= RT_TEXT_BYTES;          // (uniform)
    if (text_lds)
        for (int i = tid * 16; i < (w_hi - w_lo) + mis; i += UG_THREADS * 16) *(uint4*)(s_text + i) = *(const uint4*)(raw + (w_lo - mis) + i);
    __syncthreads();
    RETOK_STOP(1);
    const lds_u8* sl = (const lds_u8*)s_text + mis + (o0 - w_lo);
    const uint8_t* sg = raw + o0;
    RowWriter w{out + (live ? tok : 0) * maxlen, maxlen, 0};
    if (lex.counts && lex.mode) w.drop_from = lex.n_rows;
    bool todo = live && len > 0, exact = false;
    if (todo && t.special_mask != 0xffffffffu) {              // zett/utils.py:671-673
        const int id = text_lds ? whole_token_id<LdsMem>(t.specials, t.special_mask, t.special_blob, sl, len)
                                : whole_token_id<GlobalMem>(t.specials, t.special_mask, t.special_blob, sg, len);
        if (id >= 0 && (!lex.counts || id < lex.n_rows)) { w.row[0] = id; todo = false; exact = true; }
    }
    if (lex.counts && lex.mode == 0) todo = false;
    if (lex.counts && live && !todo) lex.counts[tok] = exact ? 1 : 0;      // (a segmented token's count: finish())
    int need = todo ? ((unigram_state_words(len) + 1) & ~1) : 0;
    const int W_mine = len < t.max_piece_len ? len : t.max_piece_len;
    int slots = (todo && text_lds) ? len * W_mine : 0;
    int a0 = 0;
    if (wave0) {
        a0 = wave_inclusive_scan(need) - need;
        s_base[lane + 1] = wave_inclusive_scan(slots);
        if (lane == 0) s_base[0] = 0;
        s_len[lane] = todo ? len : 0;
        s_toff[lane] = mis + (o0 - w_lo);
    }
    __syncthreads();
    RETOK_STOP(2);
    bool ok = true;
    auto finish = [&]() {
        if (!todo) return;
        if (!ok) { atomicMin(err_unk, ((unsigned long long)call << 32) | (uint32_t)(tok < 0x7ffffffe ? tok : 0x7ffffffe)); return; }
        if (w.n > maxlen) atomicAdd(n_truncated, 1ull);       // zett/utils.py:683-685
        if (lex.counts) lex.counts[tok] = lex.count_of(w);
    };
    if (!text_lds) {          // (uniform) more than 4 KiB of text in 64 tokens: the per-lane code on global memory
        if (todo) {
            int32_t* scr = scratch + ((int64_t)o0 * SCR_PER_BYTE + tok * SCR_FIXED);
            ok = unigram_token<GlobalMem>(t, L, sg, len, scr, w);
        }
        finish();
        return;
    }
    for (int tb = 0; tb < UG_TOKENS;) {          // rounds of tokens [tb, te) whose tables fit together (all of it uniform: LDS values only)
        int te = tb;
        while (te < UG_TOKENS && s_base[te + 1] - s_base[tb] <= UG_PCAP) ++te;
        const bool solo = te == tb;               // token tb alone exceeds the table: the per-lane code
        if (solo) te = tb + 1;
        const int b0 = s_base[tb], total = solo ? 0 : s_base[te] - b0;
        // ---- phase 1: every (token, start, end) slot of the round, four per thread at a time
        for (int i = tid; i < total; i += UG_THREADS * 4) {
            uint64_t hh[4];
            uint32_t slot[4];
            PieceEntry first[4];
            int sub_off[4], sub_len[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int idx = i + k * UG_THREADS;
                sub_len[k] = 0;
                if (idx >= total) continue;
                int lo = tb, hi = te - 1;              // the last token whose table starts at or before b0 + idx
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (s_base[mid] - b0 <= idx) lo = mid; else hi = mid - 1;
                }
                const int tl = s_len[lo];
                const int Wt = tl < t.max_piece_len ? tl : t.max_piece_len;
                const int local = idx - (s_base[lo] - b0);
                const int st = local / Wt, e = st + 1 + local % Wt;
                if (e > tl) { s_pid[idx] = UG_MISS; continue; }          // (the tail of the table's last rows: no such substring)
                sub_off[k] = s_toff[lo] + st;
                sub_len[k] = e - st;
                uint64_t h = FNV_OFFSET;
                for (int b = 0; b < sub_len[k]; ++b) h = fnv_step(h, s_text[sub_off[k] + b]);
                hh[k] = h;
                if (!piece_maybe(t.piece_bits, t.piece_bits_mask, h)) { s_pid[idx] = UG_MISS; sub_len[k] = 0; continue; }      // a certain miss, answered from L2
                slot[k] = piece_slot(h, t.piece_mask);
                first[k] = t.pieces[slot[k]];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (sub_len[k] == 0) continue;
                const int idx = i + k * UG_THREADS;
                const PieceEntry* pe = piece_find_from(t.pieces, t.piece_mask, t.piece_blob, hh[k], (const lds_u8*)s_text + sub_off[k], sub_len[k], slot[k], first[k]);
                if (pe) { s_pid[idx] = pe->id; s_pscore[idx] = pe->score; }
                else s_pid[idx] = UG_MISS;
            }
        }
        __syncthreads();
        RETOK_STOP(3);
        // ---- phase 2: the walk, a lane per token
        if (wave0 && todo && lane >= tb && lane < te) {
            const bool arena = a0 + need <= RT_ARENA_WORDS;
            int32_t* scr = scratch + ((int64_t)o0 * SCR_PER_BYTE + tok * SCR_FIXED);
            if (solo) {
                ok = arena ? unigram_token<LdsMem>(t, L, sl, len, (lds_i32*)s_arena + a0, w) : unigram_token<GlobalMem>(t, L, sg, len, scr, w);
            } else {
                const lds_i32* pid = (const lds_i32*)s_pid + (s_base[lane] - b0);
                const lds_f64* psc = (const lds_f64*)s_pscore + (s_base[lane] - b0);
                ok = arena ? unigram_token_table<LdsMem>(t, L, sl, len, (lds_i32*)s_arena + a0, w, pid, psc, W_mine)
                           : unigram_token_table<GlobalMem>(t, L, sg, len, scr, w, pid, psc, W_mine);
            }
            finish();
        }
        __syncthreads();
        tb = te;
    }
}

}  // namespace zett

extern "C" {

int zett_retok_create(const zett_retok_model* m, int device, zett_retok** out) {
    using namespace zett;
    if (!m || !out) return fail(ZETT_E_INVALID, "null argument");
    if (m->kind != ZETT_RETOK_BPE && m->kind != ZETT_RETOK_UNIGRAM && m->kind != ZETT_RETOK_WORDPIECE) return fail(ZETT_E_NOT_IMPLEMENTED, "hn tokenizer model kind %d", m->kind);
    if (m->kind == ZETT_RETOK_WORDPIECE && m->max_input_chars_per_word < 0) return fail(ZETT_E_INVALID, "max_input_chars_per_word must be >= 0");
    if (m->n_pieces < 0 || m->n_merges < 0 || m->n_special < 0) return fail(ZETT_E_INVALID, "negative count");
    if (m->n_pieces && (!m->piece_bytes || !m->piece_offsets || !m->piece_ids)) return fail(ZETT_E_INVALID, "piece arrays missing");
    if (m->kind == ZETT_RETOK_UNIGRAM && m->n_pieces && !m->piece_scores) return fail(ZETT_E_INVALID, "Unigram needs piece_scores");
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(ZETT_E_INVALID, "device %d out of range", device);
    ZETT_ON_DEVICE(device);
    auto* r = new zett_retok();
    std::unique_ptr<zett_retok, int (*)(zett_retok*)> guard(r, zett_retok_destroy);      // every failure below frees the handle and what it owns so far
    r->device = device;
    std::vector<int32_t> single(256, -1), bf(256, -1);
    if (m->byte_fallback && m->byte_fallback_ids) bf.assign(m->byte_fallback_ids, m->byte_fallback_ids + 256);
    HostPieceTable pt, st;
    build_piece_table(m->piece_bytes, m->piece_offsets, m->piece_ids, m->piece_scores, m->n_pieces, pt, single.data(),
                      m->kind == ZETT_RETOK_WORDPIECE ? m->piece_continuing : nullptr);
    build_piece_table(m->special_bytes, m->special_offsets, m->special_ids, nullptr, m->n_special, st, nullptr);
    std::vector<MergeEntry> mt;
    uint32_t mmask = 0xffffffffu;
    if (m->n_merges > 0) {
        const uint32_t cap = pow2_capacity((size_t)m->n_merges);
        mmask = cap - 1;
        mt.assign(cap, MergeEntry{-1, -1, 0, 0});
        for (int i = 0; i < m->n_merges; ++i) {   // a pair listed twice: the later entry wins (HashMap collect)
            const int32_t a = m->merges[3 * i], b = m->merges[3 * i + 1], nid = m->merges[3 * i + 2];
            if (a < 0 || b < 0) return fail(ZETT_E_INVALID, "merge %d has a negative id", i);
            uint32_t slot = merge_slot(a, b, mmask);
            while (mt[slot].a != -1 && !(mt[slot].a == a && mt[slot].b == b)) slot = (slot + 1) & mmask;
            mt[slot] = MergeEntry{a, b, i, nid};
        }
    }
    std::vector<int16_t> cp(324, -1);           // GPT-2 bytes_to_unicode, inverted
    {
        int extra = 0;
        for (int b = 0; b < 256; ++b) {
            const bool keep = (b >= 33 && b <= 126) || (b >= 161 && b <= 172) || (b >= 174);
            cp[keep ? b : 256 + extra++] = (int16_t)b;
        }
    }
    RetokTables& t = r->t;
    if (int rc = upload(r, pt.slots, &t.pieces)) return rc;
    if (int rc = upload(r, pt.blob, &t.piece_blob)) return rc;
    t.piece_mask = pt.mask;
    if (int rc = upload(r, pt.bits, &t.piece_bits)) return rc;
    t.piece_bits_mask = pt.bits_mask;
    if (!t.pieces) {   // empty vocabulary: one empty slot so lookups terminate
        std::vector<PieceEntry> one(16, PieceEntry{0, 0, 0, 0, 0, 0.0});
        if (int rc = upload(r, one, &t.pieces)) return rc;
        t.piece_mask = 15;
    }
    if (int rc = upload(r, st.slots, &t.specials)) return rc;
    if (int rc = upload(r, st.blob, &t.special_blob)) return rc;
    t.special_mask = st.mask;
    if (int rc = upload(r, mt, &t.merges)) return rc;
    t.merge_mask = mmask;
    if (int rc = upload(r, single, &t.single_id)) return rc;
    if (int rc = upload(r, bf, &t.bf_ids)) return rc;
    if (int rc = upload(r, cp, &t.cp_to_byte)) return rc;
    t.kind = m->kind; t.unk_id = m->unk_id; t.fuse_unk = m->fuse_unk; t.byte_fallback = m->byte_fallback;
    t.ignore_merges = m->ignore_merges; t.max_piece_len = pt.max_len; t.max_word_chars = m->max_input_chars_per_word;
#ifdef ZETT_RETOK_DEBUG
    { const char* e = getenv("ZETT_RETOK_STOP"); t.debug_stop = e ? atoi(e) : 0; }
#endif
    t.unk_score = m->unigram_min_score - 10.0;   // tokenizers kUnkPenalty
    HIP_TRY(hipHostMalloc((void**)&r->host_pinned, 128, hipHostMallocDefault));
    HIP_TRY(hipEventCreateWithFlags(&r->done, hipEventDisableTiming));
    *out = guard.release();
    return 0;
}

int zett_retok_set_option(zett_retok* r, const char* key, int64_t value) {
    using namespace zett;
    if (!r || !key) return fail(ZETT_E_INVALID, "null argument");
    if (!strcmp(key, "unigram_workgroup")) {
        if (value < 0 || value > 2) return fail(ZETT_E_INVALID, "unigram_workgroup: 0 (lane kernel), 1 (by size), 2 (workgroup kernel)");
        r->unigram_wg = (int)value;
        return 0;
    }
    return fail(ZETT_E_INVALID, "unknown retokenizer option '%s'", key);
}

int zett_retok_destroy(zett_retok* r) {
    if (!r) return 0;
    ::zett::DeviceScope _scope(r->device);
    for (void* p : r->owned) (void)hipFree(p);
    for (zett::DevBuf* b : {&r->raw, &r->raw_pos, &r->raw_off, &r->blk, &r->scratch, &r->misc}) b->release();
    if (r->host_pinned) (void)hipHostFree(r->host_pinned);
    if (r->done) (void)hipEventDestroy(r->done);
    delete r;
    return 0;
}

}  // extern "C"

namespace zett {

// result words on the device (r->misc): [0] err_pos = (call << 32 | text position) of the first character outside the byte
// table, [1] err_unk = (call << 32 | token) of the first token that needed a missing unk id, [2] tokens cut to maxlen —
// accumulated over the calls since the last result query
static int retok_reset_words(zett_retok* r, hipStream_t st) {
    unsigned long long* init = (unsigned long long*)(r->host_pinned + 12);
    init[0] = ~0ull; init[1] = ~0ull; init[2] = 0ull;
    if (int rc = r->misc.reserve(64)) return rc;
    HIP_TRY(hipMemcpyAsync(r->misc.p, init, 24, hipMemcpyHostToDevice, st));
    r->words_ready = true;
    r->calls = 0;
    r->recent.clear();
    return 0;
}

// zett_retokenize_async, and with lex.counts set the same call as stage 1 and 2 of zett_lexical_plan (lexical.hip)
int retok_enqueue_call(zett_retok* r, const uint8_t* token_chars, const int32_t* offsets, int64_t n_tokens, int64_t n_text,
                       int32_t maxlen, int32_t pad_id, int32_t* out, void* stream, LexPlan lex) {
    if (!r) return fail(ZETT_E_INVALID, "null argument");
    if (!r->tokenizes()) return fail(ZETT_E_STATE, "the handle's tables are built on the device: zett_sampled_vocab_build and zett_sampled_vocab_commit come first");
    if (n_tokens < 0 || maxlen < 1 || n_text < 0 || n_text >= (int64_t)0x7fffffff) return fail(ZETT_E_INVALID, "bad shape");
    if (n_tokens == 0) return 0;
    if (!out) return fail(ZETT_E_INVALID, "null argument");
    if (n_text > 0 && !token_chars) return fail(ZETT_E_INVALID, "token_chars is null");
    const bool sep = offsets == nullptr;      // NUL-separated text: the token boundaries are found on the device
    if (sep && n_text < n_tokens - 1) return fail(ZETT_E_INVALID, "NUL-separated text of %lld tokens needs at least %lld bytes", (long long)n_tokens, (long long)(n_tokens - 1));
    ZETT_ON_DEVICE(r->device);
    hipStream_t st = (hipStream_t)stream;
    if (!r->words_ready) { if (int rc = retok_reset_words(r, st)) return rc; }
    if (r->calls >= (1u << 20)) return fail(ZETT_E_STATE, "2^20 asynchronous calls without zett_retok_result: collect the results first");
    const int n_blocks = (int)((n_text + CH_PER_BLOCK - 1) / CH_PER_BLOCK);
    if (int rc = r->raw.reserve((size_t)n_text + 16)) return rc;
    if (int rc = r->raw_pos.reserve(((size_t)n_text + 1) * 4)) return rc;
    if (int rc = r->raw_off.reserve(((size_t)n_tokens + 1) * 4)) return rc;
    if (int rc = r->blk.reserve(((size_t)n_blocks + 2) * 4 * 4)) return rc;
    if (int rc = r->scratch.reserve(((size_t)n_text * SCR_PER_BYTE + (size_t)n_tokens * SCR_FIXED + 64) * 4)) return rc;
    int32_t* blk_count = r->blk.as<int32_t>();
    int32_t* blk_scan = blk_count + n_blocks + 1;
    int32_t* sep_count = blk_scan + n_blocks + 2;          // (separator mode: the same pair for the NUL counts)
    int32_t* sep_scan = sep_count + n_blocks + 1;
    unsigned long long* words = r->misc.as<unsigned long long>();
    const uint32_t call = r->calls++;
    r->recent.push_back({offsets, n_tokens});          // (the caller keeps `offsets` alive until zett_retok_result: include/zett_hip.h)
    // a failed enqueue takes its call back: zett_retok_result must not wait on a `done` event that was never recorded for it,
    // and the words (which kernels of this call may already have touched) start afresh with the next call
    auto enqueue = [&]() -> int {
        hipLaunchKernelGGL(fill_i32_kernel, dim3(1024), dim3(256), 0, st, out, n_tokens * (int64_t)maxlen, pad_id);   // :662-666
        if (sep) HIP_TRY(hipMemsetAsync(r->raw_off.p, 0, ((size_t)n_tokens + 1) * 4, st));
        if (n_blocks > 0 && sep) {
            hipLaunchKernelGGL((chars_to_bytes_kernel<0, true>), dim3(n_blocks), dim3(256), 0, st, token_chars, n_text, r->t.cp_to_byte,
                               blk_count, (uint8_t*)nullptr, (uint32_t*)nullptr, (unsigned long long*)nullptr, call, sep_count, (int32_t*)nullptr, n_tokens);
            hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, st, blk_count, blk_scan, (int64_t)n_blocks);
            hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, st, sep_count, sep_scan, (int64_t)n_blocks);
            hipLaunchKernelGGL((chars_to_bytes_kernel<1, true>), dim3(n_blocks), dim3(256), 0, st, token_chars, n_text, r->t.cp_to_byte,
                               blk_scan, r->raw.as<uint8_t>(), (uint32_t*)nullptr, words, call, sep_scan, r->raw_off.as<int32_t>(), n_tokens);
        } else if (n_blocks > 0) {
            hipLaunchKernelGGL((chars_to_bytes_kernel<0, false>), dim3(n_blocks), dim3(256), 0, st, token_chars, n_text, r->t.cp_to_byte,
                               blk_count, (uint8_t*)nullptr, (uint32_t*)nullptr, (unsigned long long*)nullptr, call);
            hipLaunchKernelGGL(exclusive_scan_kernel, dim3(1), dim3(1024), 0, st, blk_count, blk_scan, (int64_t)n_blocks);
            hipLaunchKernelGGL((chars_to_bytes_kernel<1, false>), dim3(n_blocks), dim3(256), 0, st, token_chars, n_text, r->t.cp_to_byte,
                               blk_scan, r->raw.as<uint8_t>(), r->raw_pos.as<uint32_t>(), words, call);
        } else {
            HIP_TRY(hipMemsetAsync(blk_scan, 0, 8, st));
        }
        if (!sep)
            hipLaunchKernelGGL(token_raw_offsets_kernel, dim3((unsigned)((n_tokens + 1 + 255) / 256)), dim3(256), 0, st, offsets, n_tokens,
                               n_text, r->raw_pos.as<uint32_t>(), blk_scan, n_blocks, r->raw_off.as<int32_t>());
        // Unigram: the workgroup kernel while its workgroups (two per CU) fit the chip in one round — a rank's shard, a CLI batch —,
        // the lane kernel beyond (five single-wave workgroups per CU, all resident): 4 096 tokens 74 vs 90 us, 50 350 tokens 125 vs 103
        // (profiles/r6_retok_ab.jsonl); "unigram_workgroup" 2 / 0 force one of them
        if (r->t.kind == ZETT_RETOK_UNIGRAM && (r->unigram_wg == 2 || (r->unigram_wg == 1 && n_tokens <= 32768)))
            hipLaunchKernelGGL(retok_unigram_kernel, dim3((unsigned)((n_tokens + UG_TOKENS - 1) / UG_TOKENS)), dim3(UG_THREADS), 0, st, r->t, r->raw.as<uint8_t>(),
                               r->raw_off.as<int32_t>(), n_tokens, maxlen, pad_id, out, r->scratch.as<int32_t>(), words + 2, words + 1, call, lex);
        else
            hipLaunchKernelGGL(retok_tokens_kernel, dim3((unsigned)((n_tokens + 63) / 64)), dim3(64), 0, st, r->t, r->raw.as<uint8_t>(),
                               r->raw_off.as<int32_t>(), n_tokens, maxlen, pad_id, out, r->scratch.as<int32_t>(), words + 2, words + 1, call, lex);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(r->host_pinned + 4, words, 24, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(r->done, st));
        return 0;
    };
    if (int rc = enqueue()) {
        (void)hipStreamSynchronize(st);
        r->calls--;
        r->recent.pop_back();
        if (r->calls == 0) r->words_ready = false;
        return rc;
    }
    return 0;
}

}  // namespace zett

extern "C" {

int zett_retokenize_async(zett_retok* r, const uint8_t* token_chars, const int32_t* offsets, int64_t n_tokens, int64_t n_text,
                          int32_t maxlen, int32_t pad_id, int32_t* out, void* stream) {
    return zett::retok_enqueue_call(r, token_chars, offsets, n_tokens, n_text, maxlen, pad_id, out, stream, zett::LexPlan{nullptr, 0, 0});
}

int zett_retok_result(zett_retok* r, int64_t* n_truncated, int64_t* bad_call, int64_t* bad_token) {
    using namespace zett;
    if (!r || !n_truncated) return fail(ZETT_E_INVALID, "null argument");
    *n_truncated = 0;
    if (bad_call) *bad_call = -1;
    if (bad_token) *bad_token = -1;
    if (r->calls == 0) return 0;
    ZETT_ON_DEVICE(r->device);
    HIP_TRY(hipEventSynchronize(r->done));
    unsigned long long w[3];
    memcpy(w, r->host_pinned + 4, 24);
    const std::vector<zett_retok::Call> recent = r->recent;
    r->words_ready = false;          // the next call starts from fresh words
    r->calls = 0;
    r->recent.clear();
    if (w[0] != ~0ull) {                                       // KeyError: locate the token of the first bad character
        const uint32_t call = (uint32_t)(w[0] >> 32);
        const int32_t pos = (int32_t)(w[0] & 0xffffffffu);
        int64_t lo = -1;
        if (call < recent.size() && recent[call].offsets == nullptr && (w[0] & 0xffffffffu) == 0xfffffffeu) {
            if (bad_call) *bad_call = call;
            return fail(ZETT_E_INVALID, "call %u: the NUL-separated text does not hold n_tokens - 1 separators", call);
        }
        if (call < recent.size() && recent[call].offsets == nullptr) {
            lo = pos;                                          // NUL-separated text: the kernel reported the token index itself
        } else if (call < recent.size()) {
            const auto& cl = recent[call];
            std::vector<int32_t> ho((size_t)cl.n_tokens + 1);
            HIP_TRY(hipMemcpy(ho.data(), cl.offsets, ((size_t)cl.n_tokens + 1) * 4, hipMemcpyDeviceToHost));
            int64_t hi = cl.n_tokens;
            lo = 0;                                            // last token with offset <= pos
            while (lo + 1 < hi) { const int64_t mid = (lo + hi) / 2; if (ho[mid] <= pos) lo = mid; else hi = mid; }
        }
        if (bad_call) *bad_call = call;
        if (bad_token) *bad_token = lo;
        return fail(ZETT_E_KEY, "token %lld holds a character outside the byte-level table (%s %d)", (long long)lo,
                    (call < recent.size() && recent[call].offsets == nullptr) ? "token" : "text offset", pos);
    }
    if (w[1] != ~0ull) {
        const int64_t tok = (int64_t)(w[1] & 0xffffffffu);
        if (bad_call) *bad_call = (int64_t)(w[1] >> 32);
        if (bad_token) *bad_token = tok;
        if (r->t.kind == ZETT_RETOK_WORDPIECE)
            return fail(ZETT_E_STATE, "WordPiece error: Missing [UNK] token from the vocabulary (token %lld)", (long long)tok);
        return fail(ZETT_E_STATE, "Encountered an unknown token but `unk_id` is missing (token %lld)", (long long)tok);
    }
    *n_truncated = (int64_t)w[2];
    return 0;
}

int zett_retokenize(zett_retok* r, const uint8_t* token_chars, const int32_t* offsets, int64_t n_tokens, int32_t maxlen,
                    int32_t pad_id, int32_t* out, int64_t* n_truncated, int64_t* bad_token, void* stream) {
    using namespace zett;
    if (!r || !n_truncated) return fail(ZETT_E_INVALID, "null argument");
    if (n_tokens < 0 || maxlen < 1) return fail(ZETT_E_INVALID, "bad shape");
    if (bad_token) *bad_token = -1;
    *n_truncated = 0;
    if (n_tokens == 0) return 0;
    if (!offsets || !out) return fail(ZETT_E_INVALID, "null argument");
    ZETT_ON_DEVICE(r->device);
    hipStream_t st = (hipStream_t)stream;
    if (r->calls) {                  // results of earlier asynchronous calls nobody asked for: drop them
        int64_t t, c, b;
        (void)zett_retok_result(r, &t, &c, &b);
    }
    // total text length = offsets[n_tokens]
    int32_t* hp = r->host_pinned;
    HIP_TRY(hipMemcpyAsync(hp, offsets + n_tokens, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int64_t n_text = hp[0];
    if (n_text < 0) return fail(ZETT_E_INVALID, "offsets must be non-decreasing from 0");
    if (int rc = zett_retokenize_async(r, token_chars, offsets, n_tokens, n_text, maxlen, pad_id, out, stream)) return rc;
    return zett_retok_result(r, n_truncated, nullptr, bad_token);
}

}  // extern "C"
