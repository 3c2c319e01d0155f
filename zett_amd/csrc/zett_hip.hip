// zett_hip.hip — the hypernet forward of libzett_hip.so's C ABI (see include/zett_hip.h): zett_forward[_into],
// zett_forward_table[_into], zett_table_rows, zett_workspace_bytes.  The handle they work on is forward_handle.hip.h; its weights,
// options and getters are model.hip, the plan of a call plan.hip.
//
// Host-side orchestration of the hypernet forward on one MI355X:
//
//   plan      surface forms -> packed positions, distinct referenced source ids (plan.hip)
//   table     for each DISTINCT source id once: gather + in_scaler/fallback ->
//             input_projection (Linear + ProjectorBlock)            [hoisting, exact]
//   encoder   RobertaEmbeddings + hn_n_layers encoder layers over the PACKED
//             positions only (pad positions never influence hidden[:,0])  [exact]
//             last layer: keys/values for every position, query / O-proj / FFN for
//             position 0 only                                            [exact]
//   heads     ProjectorBlock + Linear (+ Rescaler) per output head, bias head
//
// Every dense contraction goes through gemm.hip.h (MFMA); everything else through
// the streaming kernels of rowops.hip.h.  All launches go to the caller's stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <type_traits>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "forward_handle.hip.h"
#include "gemm.hip.h"
#include "gemm_launch.hip.h"
#include "plan.hip.h"
#include "rowops.hip.h"
#include "rowops_launch.hip.h"

using namespace zett;

namespace {

inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// Device bytes zett_forward reserves, as a function of what the plan found (packed positions
// Ttot, distinct ids D).  One definition shared by the forward, zett_table_rows and zett_workspace_bytes.
struct WorkspaceSizes {
    int64_t chunk_tokens;
    size_t table, x0, f32_rows, lo_rows, big, stats, parts;
    size_t total() const { return table + x0 + 3 * f32_rows + 3 * lo_rows + big + stats + parts; }
};

// Packed positions per encoder chunk when the caller has not set "max_chunk_tokens": 12 GiB of per-position workspace,
// never under 131 072 positions.  That is 131 072 at H = 4096 (112 KB per position), 230 k at H = 2048, 640 k at
// H = 768: a narrow hypernet's vocabulary stays ONE chunk (the 50 350-row XLM-R workload packs 169 283 positions; cut at
// 131 072 it ran a second, 38 211-position chunk whose GEMMs and ~35 extra launches cost 5 % of the step).
static int64_t chunk_token_cap(const zett_config& c, size_t es) {
    const size_t wide = (size_t)std::max(c.intermediate, 3 * c.hidden);
    const size_t per_token = (size_t)c.n_in_embd * es + 3 * (size_t)c.hidden * 4 + 3 * (size_t)c.hidden * es + wide * es + 24;
    return std::max<int64_t>(131072, (int64_t)(((size_t)12 << 30) / per_token));
}

static WorkspaceSizes workspace_sizes(const zett_config& c, size_t es, int seq, int64_t Ttot, int64_t D, int64_t cap) {
    const int lam = c.embed_lang ? 1 : 0;
    WorkspaceSizes w{};
    if (cap <= 0) cap = chunk_token_cap(c, es);
    w.chunk_tokens = std::max<int64_t>(std::min<int64_t>(cap, std::max<int64_t>(Ttot, D)), seq + lam);
    const size_t MC = (size_t)w.chunk_tokens, MCS = MC + 768;       // (384 slack rows per lane: two concurrent lanes at most)
    const size_t wide = (size_t)std::max(c.intermediate, 3 * c.hidden);
    w.table = (size_t)D * c.hidden * 4;
    w.x0 = MCS * c.n_in_embd * es;
    w.f32_rows = MCS * c.hidden * 4;               // (the second lane's slice starts 384 rows behind the first one's rows)
    w.lo_rows = MCS * c.hidden * es;
    w.big = MCS * wide * es;
    w.stats = 2 * MCS * 2 * sizeof(float);         // (mean, rstd) per row: two LayerNorms in flight
    w.parts = c.hidden % 128 == 0 ? (size_t)(c.hidden / 128) * MCS * sizeof(float2) : 0;      // LayerNorm-fold partials (reserved when ForwardMode::fold)
    return w;
}

template <typename T>
int do_forward(zett_hypernet* h, const ExtTable* ext, const int32_t* sfm, int64_t N, int seq, const void* src, int src_dtype, const zett_dest* dest,
               int lang_index, float* out_in, float* out_out, float* out_bias, hipStream_t st);
template <typename T>
int do_table_rows(zett_hypernet* h, const int32_t* id_list, int first, int count, const void* src, int src_dtype, void* table_out, float* stats_out, hipStream_t st);
// 0 when the handle's precision and options give ForwardMode::table_lo (below), else `entry`'s refusal: host state only, no device call
int check_folded_table(const zett_hypernet* h, const char* entry);

}  // namespace

namespace zett {

int check_call(const zett_hypernet* h, const CallCheck& k) {
    if (!h) return fail(ZETT_E_INVALID, "null handle");
    if (!h->finalized) return fail(ZETT_E_STATE, "zett_finalize has not been called");
    const zett_config& c = h->cfg;
    if (k.null_first && k.null_arg) return fail(ZETT_E_INVALID, "%s", k.null_text);
    if (k.shape && (k.n_rows < (k.empty_ok ? 0 : 1) || k.seq < 1)) return fail(ZETT_E_INVALID, "bad surface-form shape [%lld, %d]", (long long)k.n_rows, k.seq);
    if (k.encoder && k.seq + (c.embed_lang ? 1 : 0) > c.max_positions)
        return fail(ZETT_E_INDEX, "sequence %d exceeds position_embeddings (%d rows)", k.seq, c.max_positions);
    if (k.shape && k.n_rows == 0) return CALL_EMPTY;
    if (k.null_arg) return fail(ZETT_E_INVALID, "%s", k.null_text);
    if (k.need_out_out) return fail(ZETT_E_INVALID, "out_out is required when separate_out_embeddings is set");
    if (k.source) {
        if (!is_dtype(k.src_dtype)) return fail(ZETT_E_INVALID, "unknown source dtype %d", k.src_dtype);
        if (k.v_src < c.original_vocab_size)
            return fail(ZETT_E_INDEX, "source_embeddings has %lld rows, config.original_vocab_size is %d", (long long)k.v_src, c.original_vocab_size);
    }
    if (k.encoder && c.embed_lang && (k.lang_index < 0 || k.lang_index >= c.n_langs)) return fail(ZETT_E_INDEX, "lang_index %d outside [0,%d)", k.lang_index, c.n_langs);
    if (k.shape && k.n_rows * (int64_t)(k.seq + 1) >= (int64_t)0x7fffffff) return fail(ZETT_E_INVALID, "too many positions for one call");
    if (k.table_mode && h->precision == ZETT_PREC_F32) return fail(ZETT_E_INVALID, "%s: the folded 16-bit table exists in the 16-bit modes only", k.table_mode);
    return 0;
}

}  // namespace zett

// ---------------------------------------------------------------------------------
extern "C" {

int zett_workspace_bytes(const zett_hypernet* h, int64_t n_rows, int32_t seq, int64_t* out_bytes) {
    if (!h || !out_bytes) return fail(ZETT_E_INVALID, "null argument");
    if (n_rows < 0 || seq < 1) return fail(ZETT_E_INVALID, "bad surface-form shape [%lld, %d]", (long long)n_rows, seq);
    const zett_config& c = h->cfg;
    const int64_t V = (int64_t)c.original_vocab_size + c.n_extra;
    const int64_t max_tok = n_rows * (int64_t)(seq + (c.embed_lang ? 1 : 0));
    // worst case of the plan: no pad position, every position a different source id
    const WorkspaceSizes w = workspace_sizes(c, elt_size(h->precision), seq, max_tok, std::min<int64_t>(V, max_tok), h->opt.max_chunk_tokens);
    *out_bytes = (int64_t)(w.total() + plan_i32_bytes(h, n_rows, seq) + (size_t)n_rows + (size_t)max_tok);
    return 0;
}

}  // extern "C"

namespace {

// (zett_forward_into) the destination's own arguments; the row map is checked against n_dest_rows on the device (do_forward)
int check_dest(const zett_hypernet* h, const zett_dest* d, int64_t n_rows) {
    const zett_config& c = h->cfg;
    if (!d) return fail(ZETT_E_INVALID, "null destination");
    if (!d->in) return fail(ZETT_E_INVALID, "the destination's `in` matrix is null");
    if (c.separate_out != (d->out != nullptr))
        return fail(ZETT_E_INVALID, c.separate_out ? "the destination's `out` matrix is required when separate_out_embeddings is set"
                                                   : "the destination's `out` must be null: this config has no second output");
    if (d->dtype < ZETT_F32 || d->dtype > ZETT_BF16) return fail(ZETT_E_INVALID, "unknown destination dtype %d", d->dtype);
    if (d->bias && (d->bias_dtype < ZETT_F32 || d->bias_dtype > ZETT_BF16)) return fail(ZETT_E_INVALID, "unknown bias destination dtype %d", d->bias_dtype);
    if (d->ld_in < c.n_embd || (d->out && d->ld_out < c.n_embd))
        return fail(ZETT_E_INVALID, "destination leading dimension (%lld, %lld) below n_embd %d", (long long)d->ld_in, (long long)d->ld_out, c.n_embd);
    if (d->n_dest_rows < 0 || (!d->rows && d->n_dest_rows < n_rows))
        return fail(ZETT_E_INVALID, "the destination has %lld rows, the identity map needs %lld", (long long)d->n_dest_rows, (long long)n_rows);
    return 0;
}

int forward_entry(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq, const void* source_embeddings, int src_dtype,
                  int64_t v_src, int32_t lang_index, const zett_dest* dest, float* out_in, float* out_out, float* out_bias, void* stream) {
    CallCheck k;
    k.n_rows = n_rows; k.seq = seq; k.empty_ok = true; k.encoder = true; k.lang_index = lang_index;
    k.null_arg = !surface_forms || !source_embeddings || (!dest && (!out_in || !out_bias));
    k.need_out_out = h && !dest && h->cfg.separate_out && !out_out;
    k.source = true; k.src_dtype = src_dtype; k.v_src = v_src;
    const int checked = check_call(h, k);
    if (checked != 0 && checked != CALL_EMPTY) return checked;
    ZETT_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    if (checked == CALL_EMPTY) {
        h->stats = zett_stats{};
        if (!h->opt.range_accumulate) HIP_TRY(hipMemsetAsync(h->range_word.p, 0, 4, st));
        for (Event& e : h->out_ready) {
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e.e, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(e, st));
        }
        h->out_recorded = true;
        return 0;
    }
    return with_precision(h->precision, [&](auto a) {
        return do_forward<typename decltype(a)::type>(h, nullptr, surface_forms, n_rows, seq, source_embeddings, src_dtype, dest, lang_index, out_in, out_out, out_bias, st);
    });
}

}  // namespace

extern "C" {

int zett_forward(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq,
                 const void* source_embeddings, int src_dtype, int64_t v_src, int32_t lang_index,
                 float* out_in, float* out_out, float* out_bias, void* stream) {
    return forward_entry(h, surface_forms, n_rows, seq, source_embeddings, src_dtype, v_src, lang_index, nullptr, out_in, out_out, out_bias, stream);
}

int zett_forward_into(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq, const void* source_embeddings, int src_dtype,
                      int64_t v_src, int32_t lang_index, const zett_dest* dest, void* stream) {
    if (!h) return fail(ZETT_E_INVALID, "null handle");
    if (int rc = check_dest(h, dest, n_rows)) return rc;
    return forward_entry(h, surface_forms, n_rows, seq, source_embeddings, src_dtype, v_src, lang_index, dest, nullptr, nullptr, nullptr, stream);
}

// ---- (ABI 8) the hoisted table shared between ranks: SURVEY 8e's optional second exchange ---------------------------------
int zett_table_rows(zett_hypernet* h, const int32_t* id_list, int64_t first, int64_t count, const void* source_embeddings, int src_dtype,
                    int64_t v_src, void* table_out, float* stats_out, void* stream) {
    CallCheck k;
    k.shape = false;                    // (a range of table rows instead of surface forms: checked here, between the handle and the tensors)
    if (int rc = check_call(h, k)) return rc;
    if (first < 0 || count < 0 || first + count >= (int64_t)0x7fffffff) return fail(ZETT_E_INVALID, "bad table range [%lld, +%lld)", (long long)first, (long long)count);
    // whether this handle builds table rows at all is answered before the empty slice: the ranks of a small vocabulary, some with rows and
    // some without, then agree — and a call with count == 0 and null tensors is the probe for it
    if (int rc = check_folded_table(h, "zett_table_rows")) return rc;
    if (count == 0) return 0;
    k.null_arg = !id_list || !source_embeddings || !table_out || !stats_out;
    k.source = true; k.src_dtype = src_dtype; k.v_src = v_src;
    if (int rc = check_call(h, k)) return rc;
    ZETT_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    return with_precision(h->precision, [&](auto a) {
        using T = typename decltype(a)::type;
        if constexpr (std::is_same<T, float>::value) return fail(ZETT_E_INVALID, "zett_table_rows: the folded 16-bit table exists in the 16-bit modes only");
        else return do_table_rows<T>(h, id_list, (int)first, (int)count, source_embeddings, src_dtype, table_out, stats_out, st);
    });
}

}  // extern "C"

namespace {
int forward_table_entry(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq, const void* table, const float* table_stats,
                        const int32_t* id_slot, int32_t lang_index, const zett_dest* dest, float* out_in, float* out_out, float* out_bias, void* stream) {
    CallCheck k;
    k.n_rows = n_rows; k.seq = seq; k.encoder = true; k.lang_index = lang_index; k.table_mode = "zett_forward_table";
    k.null_arg = !surface_forms || !table || !table_stats || !id_slot || (!dest && (!out_in || !out_bias));
    k.need_out_out = h && !dest && h->cfg.separate_out && !out_out;
    if (int rc = check_call(h, k)) return rc;
    ZETT_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    const ExtTable ext{table, table_stats, id_slot};
    return with_precision(h->precision, [&](auto a) {
        return do_forward<typename decltype(a)::type>(h, &ext, surface_forms, n_rows, seq, nullptr, ZETT_F32, dest, lang_index, out_in, out_out, out_bias, st);
    });
}

}  // namespace

extern "C" {

int zett_forward_table(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq, const void* table, const float* table_stats,
                       const int32_t* id_slot, int32_t lang_index, float* out_in, float* out_out, float* out_bias, void* stream) {
    return forward_table_entry(h, surface_forms, n_rows, seq, table, table_stats, id_slot, lang_index, nullptr, out_in, out_out, out_bias, stream);
}

int zett_forward_table_into(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq, const void* table, const float* table_stats,
                            const int32_t* id_slot, int32_t lang_index, const zett_dest* dest, void* stream) {
    if (!h) return fail(ZETT_E_INVALID, "null handle");
    if (int rc = check_dest(h, dest, n_rows)) return rc;
    return forward_table_entry(h, surface_forms, n_rows, seq, table, table_stats, id_slot, lang_index, dest, nullptr, nullptr, nullptr, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------
namespace {

template <typename T>
struct Runner {
    zett_hypernet* h;
    hipStream_t st;
    int rc = 0;

    static const T* W(const Linear& l) { return (const T*)l.w; }      // a bound GEMM operand (Model) in this forward's arithmetic type

    GemmEpilogue<T> epi() {
        GemmEpilogue<T> e{};
        e.split_col = 0x7fffffff;
        e.range_flag = h->range_word.p;
        return e;
    }

    long a_rows_readable = 0;   // rows every A operand buffer can be read for (workspace slack)
    bool staged_dst = false;    // (zett_forward_into) the launch in flight writes the staged fp32 rows of a destination (gemm log bit 11)
    int stage_lane = 0;         // (zett_forward_into) which staging buffer head_gemm uses: the lane's own (h->dest_stage[lane])

    bool timing = false;        // "time_gemm": an event pair around every launch (a forward's; zett_table_rows keeps no log of its own)

    // the tile variant a launch takes: gemm_variant_for (gemm_launch.hip.h), the rule zett_op_fwd_gemm shares
    int variant_for(int M, int N, int K, const GemmEpilogue<T>& e) const { return gemm_variant_for<T>(h->opt.gemm, a_rows_readable, M, N, K, e); }

    void gemm(const T* A, int lda, const T* Wp, int ldw, int M, int N, int K, const GemmEpilogue<T>& e) {
        if (rc || M <= 0) return;
        const GemmArgs<T> g = gemm_args_for(h->opt.gemm, A, lda, Wp, ldw, M, N, K, e);
        const double fl = 2.0 * (double)M * (double)N * (double)K;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (timing) {
            while (h->ev.size() < h->ev_used + 2) {
                hipEvent_t ev;
                if (hipEventCreate(&ev) != hipSuccess) { rc = fail(ZETT_E_HIP, "hipEventCreate failed"); return; }
                h->ev.emplace_back().e = ev;
            }
            e0 = h->ev[h->ev_used++];
            e1 = h->ev[h->ev_used++];
            (void)hipEventRecord(e0, st);
        }
        const int variant = variant_for(M, N, K, e);
        {
            zett_gemm_record r{};
            r.m = M; r.n = N; r.k = K; r.variant = variant;
            r.epilogue = (e.out_lo ? 1 : 0) | ((e.out_f32 || e.out_f32_b) ? 2 : 0) | (e.residual ? 4 : 0) | ((e.scale || e.shift) ? 8 : 0) |
                         (e.stats_part ? 16 : 0) | (e.fold_stats ? 32 : 0) | (e.residual_lo ? 64 : 0) | (e.act << 8) |
                         (e.dst ? 1024 : 0) | (staged_dst ? 2048 : 0);
            r.flops = fl;
            const double mn = (double)M * (double)N;
            const double dst_es = e.dst_dtype == ZETT_F32 ? 4.0 : 2.0;
            r.bytes = ((double)M + (double)N) * (double)K * sizeof(T) + (e.out_lo ? mn * sizeof(T) : 0.0) + ((e.out_f32 || e.out_f32_b) ? mn * 4.0 : 0.0) +
                      (e.dst ? mn * dst_es : 0.0) +
                      (e.residual ? mn * 4.0 : 0.0) + (e.residual_lo ? mn * sizeof(T) : 0.0) + (e.stats_part ? (double)M * (N / 128) * 8.0 : 0.0) + ((e.fold_stats || e.res_stats) ? (double)M * 8.0 : 0.0);
            h->gemm_log.push_back(r);
        }
        const hipError_t err = launch_gemm_variant(variant, g, st);      // gemm_launch.hip.h: the tile kernels live in their own translation units
        if (timing) (void)hipEventRecord(e1, st);
        if (err != hipSuccess) { rc = fail(ZETT_E_HIP, "gemm launch failed: %s", hipGetErrorString(err)); return; }
        h->stats.executed_flops += fl;
        h->stats.gemm_launches += 1;
    }

    // (zett_forward_into) one output of a head launch in the caller's matrix: base (already at the chunk's first row for the identity
    // map), row map (already offset to the chunk; null = identity), leading dimension, zett_dtype
    struct DestOut { void* p; const int64_t* rows; int64_t ld; int dtype; };

    // An output head's final GEMM (A [M, K] . W [N, K]^T, epilogue e with an fp32 output) storing into `d` (null: e's own fp32 rows, as
    // zett_forward).  Fused where gemm4d has a destination instantiation for the launch (variant 7, F32_SCALE / F32_SCALE_FOLD); the
    // other launches write fp32 rows to the workspace and dest_store converts them.  d_b: the columns from `split` on (hn_single_head
    // with separate outputs: always staged).
    void head_gemm(const T* A, const T* Wp, int M, int N, int K, const GemmEpilogue<T>& e, const DestOut* d, const DestOut* d_b, int split) {
        if (rc || M <= 0) return;
        if (!d) { gemm(A, K, Wp, K, M, N, K, e); return; }
        GemmEpilogue<T> ed = e;
        ed.out_f32 = nullptr; ed.out_f32_b = nullptr; ed.ld_f32 = N;
        ed.dst = d->p; ed.dst_rows = d->rows; ed.ld_dst = d->ld; ed.dst_dtype = d->dtype;
        const GemmArgs<T> probe{A, K, Wp, K, M, N, K, ed};
        if (!d_b && variant_for(M, N, K, ed) == 7 && gemm_4d_dst_mode(probe) >= 0) { gemm(A, K, Wp, K, M, N, K, ed); return; }
        DevBuf& stage_buf = h->dest_stage[stage_lane];
        if (int r = stage_buf.reserve((size_t)M * (size_t)N * sizeof(float))) { rc = r; return; }
        float* S = stage_buf.as<float>();
        GemmEpilogue<T> es = e;
        es.out_f32 = S; es.ld_f32 = N;
        if (d_b) es.out_f32_b = S + split;
        staged_dst = true;
        gemm(A, K, Wp, K, M, N, K, es);
        staged_dst = false;
        dest_store(S, N, *d, M, d_b ? split : N);
        if (d_b) dest_store(S + split, N, *d_b, M, N - split);
    }

    // the staged fallback: fp32 rows (S, ld_s) converted into the destination (dest_store_rows_kernel)
    void dest_store(const float* S, int64_t ld_s, const DestOut& d, int rows, int cols) {
        if (rc || rows <= 0) return;
        const bool vec = cols % 4 == 0 && ld_s % 4 == 0 && d.ld % 4 == 0 && (uintptr_t)S % 16 == 0 && (uintptr_t)d.p % (d.dtype == ZETT_F32 ? 16 : 8) == 0;
        const dim3 grid((unsigned)std::min<int64_t>(rows, 65535 * 16));
        with_dtype(d.dtype, [&](auto dt) {
            using OT = elem_t<decltype(dt)::value>;
            if (vec) hipLaunchKernelGGL((dest_store_rows_kernel<OT, true>), grid, dim3(256), 0, st, S, ld_s, (OT*)d.p, d.ld, d.rows, (int64_t)rows, cols, h->range_word.p);
            else hipLaunchKernelGGL((dest_store_rows_kernel<OT, false>), grid, dim3(256), 0, st, S, ld_s, (OT*)d.p, d.ld, d.rows, (int64_t)rows, cols, h->range_word.p);
        });
        check("dest_store");
    }

    void check(const char* what) {
        if (rc) return;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = fail(ZETT_E_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
    }

    // One LayerNorm launch of the instantiation (EMBED, READOUT, BT): kernel, lanes per row and grid are launch_layernorm's
    // (rowops_launch.hip.h), from (H, ln_rows8, sizeof(T)).
    template <bool EMBED, bool READOUT, typename BT>
    void ln_launch(const char* what, const float* in, int rows, const float* gamma, const float* beta, float eps, float* of, T* ol, float* stats,
                   float* sum, const LnEmbed& embed, int t0, const LnReadout& readout) {
        const int H = h->cfg.hidden;
        launch_layernorm<T, EMBED, READOUT, BT>(st, H, h->opt.ln_rows8, in, H, rows, gamma, beta, eps, of, ol, stats, sum, embed, t0, readout);
        check(what);
    }

    // Every LayerNorm launch of the forward.  Rows `in` (or, embed != null, the embeddings' sum of buffer rows [t0, t0 + rows), also
    // written to `sum` unless null) -> fp32 `of` / operand copy `ol` / (mean, rstd) `stats`, each unless null.  readout.out_bias != null:
    // the position-0 readout with the bias head; bias_dtype >= 0 (zett_forward_into): the bias goes to the caller's destination of that
    // zett_dtype (no statistics are asked for).  Only these six instantiations exist: the embeddings never read out, a destination
    // type needs a readout.
    void layernorm(const float* in, int rows, const float* gamma, const float* beta, float eps, float* of, T* ol, float* stats = nullptr,
                   const LnReadout& readout = LnReadout{}, int bias_dtype = -1, const LnEmbed* embed = nullptr, int t0 = 0, float* sum = nullptr) {
        if (rc || rows <= 0) return;
        if (embed) {
            ln_launch<true, false, void>("embed_layernorm", nullptr, rows, gamma, beta, eps, nullptr, ol, stats, sum, *embed, t0, LnReadout{});
        } else if (!readout.out_bias) {
            ln_launch<false, false, void>("layernorm", in, rows, gamma, beta, eps, of, ol, stats, nullptr, LnEmbed{}, 0, readout);
        } else if (bias_dtype < 0) {
            ln_launch<false, true, void>("layernorm", in, rows, gamma, beta, eps, of, ol, stats, nullptr, LnEmbed{}, 0, readout);
        } else {
            with_dtype(bias_dtype, [&](auto dt) {
                ln_launch<false, true, elem_t<decltype(dt)::value>>("readout", in, rows, gamma, beta, eps, of, ol, nullptr, nullptr, LnEmbed{}, 0, readout);
            });
        }
    }

    // LayerNorm fold: (mean, rstd) per row from the partials the producer GEMM wrote
    void ln_stats(const float2* parts, int ld_part, int rows, float eps, float* stats) {
        if (rc || rows <= 0) return;
        launch_ln_stats(st, h->cfg.hidden, parts, ld_part, rows, eps, stats);
        check("ln_stats");
    }

    // ProjectorBlock (modeling_hypernet.py:22-40) on rows already projected to H:
    //   out = LN_1e-6( gelu_t(W2·gelu_t(W1·x + b1) + b2) + x )
    // fold_parts != null (output heads, LayerNorm fold): the block's LayerNorm is not launched — dense2 writes the 16-bit copy of
    // the pre-LayerNorm sum to `ol` and partial row statistics, fold_stats receives (mean, rstd), and the caller's next GEMM
    // runs on the gamma-folded weight (no fp32 sum is written: nothing else reads it)
    void projector(const Projector& b, const T* x_lo, const float* x_f32, int rows, T* big, float* pre, float* of, T* ol,
                   float2* fold_parts = nullptr, int ld_part = 0, float* fold_stats = nullptr) {
        const zett_config& c = h->cfg;
        GemmEpilogue<T> e1 = epi();
        e1.bias = b.dense1.b; e1.act = ACT_GELU_TANH; e1.out_lo = big; e1.ld_lo = c.intermediate;
        gemm(x_lo, c.hidden, W(b.dense1), c.hidden, rows, c.intermediate, c.hidden, e1);
        GemmEpilogue<T> e2 = epi();
        e2.bias = b.dense2.b; e2.act = ACT_GELU_TANH; e2.residual = x_f32; e2.ld_res = c.hidden;
        e2.ld_f32 = c.hidden;
        if (fold_parts) { e2.out_lo = ol; e2.ld_lo = c.hidden; e2.stats_part = fold_parts; e2.ld_part = ld_part; }
        else e2.out_f32 = pre;
        gemm(big, c.intermediate, W(b.dense2), c.intermediate, rows, c.hidden, c.intermediate, e2);
        if (fold_parts) ln_stats(fold_parts, ld_part, rows, c.ln_eps_projector, fold_stats);
        else layernorm(pre, rows, b.ln.w, b.ln.b, c.ln_eps_projector, of, ol);
    }
};

// ---- what a forward does with this handle, decided once --------------------------------------------------------------------------
// fold — LayerNorm fold: in the 16-bit modes the LayerNorms inside the encoder are not launches — the residual GEMM
//   in front writes the 16-bit copy of its fp32 rows and per-row partial statistics, the GEMM behind runs on gamma-folded
//   weights and normalises in its epilogue.  gemm4d only: off when a tile variant is forced.
// lo_stream — 16-bit residual stream (r4): with the fold on, the encoder's hidden state travels ONLY as the 16-bit copy of the
//   pre-LayerNorm sum (+ statistics): the producers read their residual rows from it (LN16 epilogue: 4 instead of 10 bytes
//   per element, 16-byte accesses on both sides) and no fp32 sum is written; Zt and Ct alternate as its buffers (Ct is free
//   until the readout).  f16 only by default: the rounding of the stream is 2^-11 per layer there (rel-L2 of the outputs
//   0.8e-3 -> 1.0e-3 against a tolerance of 2.5e-3), in bf16 2^-8 would leave the tolerance.
// table_lo — 16-bit hoisted table (r6; with the 16-bit residual stream, i.e. f16 by default): the ProjectorBlock of the input projection
//   ends in the LayerNorm-fold PRODUCER the output heads use (dense2 writes the 16-bit copy of its pre-LayerNorm sum + partial row
//   statistics; ln_stats makes (mean, rstd)), and the embeddings' kernel normalises a table row as it reads it: the block's
//   LayerNorm launch is gone (0.40 ms on the headline, 0.16 of XLM-R's 7.3), a table element is 2 bytes on both sides, and a
//   table exchanged between ranks (SURVEY 8e's optional second exchange) would be 239 instead of 478 MB.  One 16-bit rounding of
//   the pre-LayerNorm sum replaces none: the same step the encoder's stream takes per layer.  The buffer keeps its fp32 size:
//   [D, H] 16-bit values, then [D] (mean, rstd).  zett_table_rows / zett_forward_table exist in this mode only.
// fold_heads — LayerNorm fold of the heads (r3): the ProjectorBlock's LayerNorm in front of each final Linear is not a launch either.
// (zett_workspace_bytes does not ask: it is an upper bound over the options, so workspace_sizes counts the fold's partials whenever
// H % 128 == 0 — the part of `fold` no option can change — and the forward reserves them only when `fold` holds.)
struct ForwardMode { bool fold, lo_stream, table_lo, fold_heads; };
template <typename T>
ForwardMode forward_mode(const zett_hypernet* h) {
    const zett_config& c = h->cfg;
    ForwardMode m{};
    m.fold = h->opt.ln_fold && !std::is_same<T, float>::value && h->opt.gemm.gemm_variant == 0 && c.hidden % 128 == 0 && c.hidden >= 512 && h->m.layers.back().fold_up.w != nullptr;
    m.lo_stream = m.fold && c.layers >= 1 && sizeof(T) == 2 && (h->opt.residual_lo == 2 || (h->opt.residual_lo == 1 && std::is_same<T, f16_t>::value));
    m.table_lo = m.lo_stream && h->opt.table_lo != 0;
    m.fold_heads = m.fold && h->opt.ln_fold == 1 && h->m.head_in.fold.w != nullptr;
    return m;
}
int needs_folded_table(const char* entry) {
    return fail(ZETT_E_INVALID, "%s needs the folded 16-bit table: f16 arithmetic with the LayerNorm fold, the 16-bit residual stream and table_lo on", entry);
}
int check_folded_table(const zett_hypernet* h, const char* entry) {
    if (h->precision == ZETT_PREC_F32) return fail(ZETT_E_INVALID, "%s: the folded 16-bit table exists in the 16-bit modes only", entry);
    const bool table_lo = with_precision(h->precision, [&](auto a) { return forward_mode<typename decltype(a)::type>(h).table_lo; });
    return table_lo ? 0 : needs_folded_table(entry);
}

// ---- workspace ---------------------------------------------------------------------------------------------------------------------
// The buffers behind WorkspaceSizes.  encoder = false: what the table phase alone touches (zett_table_rows reserves no more).
int reserve_workspace(zett_hypernet* h, const WorkspaceSizes& ws, bool fold, bool encoder) {
    const struct { DevBuf* buf; size_t bytes; bool encoder_only; } list[] = {
        {&h->table, ws.table, true}, {&h->x0, ws.x0, false}, {&h->yf, ws.f32_rows, false}, {&h->yt, ws.lo_rows, false}, {&h->big, ws.big, false},
        {&h->pre, ws.f32_rows, false}, {&h->ctx, ws.lo_rows, true}, {&h->cf, ws.f32_rows, true}, {&h->ct, ws.lo_rows, true},
        {&h->lnstats, ws.stats, true}, {&h->lnparts, fold ? ws.parts : 0, false}};
    for (const auto& r : list)
        if (encoder || !r.encoder_only)
            if (int rc = r.buf->reserve(r.bytes)) return rc;
    return 0;
}

// The workspace as one lane sees it: every buffer `off` rows in (lane 0, the table phase and zett_table_rows: off = 0), MCS rows each.
// LayerNorm statistics: the encoder keeps its hidden state as (pre-LayerNorm sum, statistics, gamma, beta): the LayerNorm kernel
// writes the 16-bit GEMM operand and the two statistics, and whoever needs the fp32 LayerNorm output (the next residual epilogue)
// recomputes it with ln_affine from the sum it reads anyway.  Zf and PRE alternate as the sum buffers, STa and STb as their statistics.
template <typename T>
struct Workspace {
    T* X0; float* Zf; T* Zt; T* BIG; float* PRE; T* CTX; float* Cf; T* Ct; float* STa; float* STb; float2* PARTS;
    int ld_parts;
    long a_rows;          // rows every A operand buffer can be read for: the 384-row GEMM tile reads whole tiles of A
};
template <typename U> U* buf_at(const DevBuf& b, size_t n) { return b.p ? (U*)b.p + n : nullptr; }      // (null: a buffer the call did not reserve)
template <typename T>
Workspace<T> lane_workspace(const zett_hypernet* h, size_t off, size_t MCS) {
    const size_t H = h->cfg.hidden, wide = (size_t)std::max(h->cfg.intermediate, 3 * h->cfg.hidden);
    Workspace<T> w{};
    w.X0 = buf_at<T>(h->x0, 0);                   // (the table phase only)
    w.Zf = buf_at<float>(h->yf, off * H); w.Zt = buf_at<T>(h->yt, off * H);
    w.BIG = buf_at<T>(h->big, off * wide); w.PRE = buf_at<float>(h->pre, off * H);
    w.CTX = buf_at<T>(h->ctx, off * H); w.Cf = buf_at<float>(h->cf, off * H); w.Ct = buf_at<T>(h->ct, off * H);
    w.STa = buf_at<float>(h->lnstats, 2 * off); w.STb = buf_at<float>(h->lnstats, 2 * off + 2 * MCS);
    w.PARTS = buf_at<float2>(h->lnparts, off);
    w.ld_parts = (int)MCS;
    w.a_rows = (long)(MCS - off);
    return w;
}

// The hoisted table (A2-A4): input_projection once per distinct source id — rows id_list[first .. first + count) into table rows
// [first, first + count) (the fp32 table `tbl32`, or — folded — the 16-bit pre-LayerNorm sums `tbl16` with (mean, rstd) in
// `tblst`), in chunks of MC rows through the caller's workspace.  Errors land in R.rc.
template <typename T>
void table_phase(Runner<T>& R, const Workspace<T>& w, const int32_t* id_list, int first, int count, const void* src, int src_dtype, int64_t MC,
                 bool table_lo, T* tbl16, float* tblst, float* tbl32) {
    zett_hypernet* h = R.h;
    const zett_config& c = h->cfg;
    const Model& md = h->m;
    const int H = c.hidden, EIN = c.n_in_embd;
    for (int s0 = first; s0 < first + count && !R.rc; s0 += (int)MC) {
        const int m = (int)std::min<int64_t>(MC, first + count - s0);
        with_dtype(src_dtype, [&](auto sd) {          // (in_scaler: null without hn_rescale_embeddings)
            launch_gather_src<T, decltype(sd)::value>(R.st, id_list, s0, m, src, c.n_in_embd, c.original_vocab_size, md.fallback, md.in_scaler.w, md.in_scaler.b, w.X0, h->range_word.p);
        });
        R.check("gather_src");
        GemmEpilogue<T> e0 = R.epi();
        e0.bias = md.in_proj.b; e0.out_f32 = w.Zf; e0.ld_f32 = H; e0.out_lo = w.Zt; e0.ld_lo = H;
        R.gemm(w.X0, EIN, R.W(md.in_proj), EIN, m, H, EIN, e0);
        if (table_lo) R.projector(md.in_block, w.Zt, w.Zf, m, w.BIG, w.PRE, nullptr, tbl16 + (size_t)s0 * H, w.PARTS, w.ld_parts, tblst + 2 * (size_t)s0);
        else R.projector(md.in_block, w.Zt, w.Zf, m, w.BIG, w.PRE, tbl32 + (size_t)s0 * H, nullptr);
    }
}

// (ABI 8) zett_table_rows: rows [first, first + count) of the folded table of the distinct-id list `id_list` into the caller's buffers
template <typename T>
int do_table_rows(zett_hypernet* h, const int32_t* id_list, int first, int count, const void* src, int src_dtype, void* table_out, float* stats_out, hipStream_t st) {
    const ForwardMode mode = forward_mode<T>(h);
    if (!mode.table_lo) return needs_folded_table("zett_table_rows");
    const WorkspaceSizes ws = workspace_sizes(h->cfg, sizeof(T), 1, count, count, h->opt.max_chunk_tokens);
    const size_t MCS = (size_t)ws.chunk_tokens + 768;
    if (int rc = reserve_workspace(h, ws, mode.fold, false)) return rc;
    Runner<T> R{h, st};
    R.a_rows_readable = (long)MCS;
    // (R.timing stays off: per-launch events and the launch log belong to a forward, which resets both when it starts)
    table_phase<T>(R, lane_workspace<T>(h, 0, MCS), id_list, first, count, src, src_dtype, ws.chunk_tokens, true, (T*)table_out, stats_out, nullptr);
    return R.rc;
}

// From the moment a forward has taken its plan slot, kernels that read the slot (and the pinned host words) may be enqueued: whatever
// way the forward is left — a failed launch, a failed workspace reservation, a lane that fails after the other one was launched — the
// second lane is joined to `st` and ps.released is recorded behind everything, so that a later zett_forward_prepare / zett_forward
// never rewrites the plan under kernels still in flight.
struct SlotGuard {
    zett_hypernet* h; PlanSlot* ps; hipStream_t st; bool lane_forked = false;
    ~SlotGuard() {
        if (lane_forked && h->lane_stream && h->lane_ev[3]) {
            (void)hipEventRecord(h->lane_ev[3], h->lane_stream);
            (void)hipStreamWaitEvent(st, h->lane_ev[3], 0);
        }
        if (ps->released) (void)hipEventRecord(ps->released, st);
    }
};

// "time_gemm": the HIP-event pairs of the forward's GEMM launches, read back once the stream has drained
int read_gemm_timing(zett_hypernet* h, hipStream_t st) {
    HIP_TRY(hipStreamSynchronize(st));
    const bool print = getenv("ZETT_GEMM_LOG") != nullptr;
    double ms = 0.0, fl = 0.0;
    for (size_t k = 0; 2 * k + 1 < h->ev_used && k < h->gemm_log.size(); ++k) {
        zett_gemm_record& r = h->gemm_log[k];
        float t = 0.f;
        if (hipEventElapsedTime(&t, h->ev[2 * k], h->ev[2 * k + 1]) == hipSuccess) { ms += t; fl += r.flops; r.ms = t; }
        if (print)
            fprintf(stderr, "[zett gemm] M=%6d N=%6d K=%5d tile=%s %8.3f ms %7.1f TF\n", r.m, r.n, r.k,
                    r.variant == 7 ? "4d " : r.variant == 8 ? "4dg" : r.variant == 3 ? "384" : r.variant == 2 ? "8r " : "128", t, r.flops / (t * 1e9));
    }
    h->stats.gemm_ms = ms;
    h->stats.gemm_flops_timed = fl;
    return 0;
}

// One forward (zett_forward / _into / _table / _table_into), in stages: run() names them in order.
template <typename T>
struct Forward {
    using DestOut = typename Runner<T>::DestOut;
    // the call (ext: the caller's table of zett_forward_table[_into], else null)
    zett_hypernet* h; const ExtTable* ext; const int32_t* sfm; int64_t N; int seq; const void* src; int src_dtype; const zett_dest* dest; int lang_index;
    float* out_in; float* out_out; float* out_bias; hipStream_t st;
    // what the stages find
    Runner<T> R{h, st};
    const zett_config& c = h->cfg;
    const Model& md = h->m;
    const int H = c.hidden, I = c.intermediate, E = c.n_embd;
    const ForwardMode mode = forward_mode<T>(h);
    PlanSlot* ps = nullptr;
    PlanArrays p{};
    bool pair_plan = false;
    const int32_t* hoff = nullptr;        // pinned: row offsets [N + 1], then distinct ids, error word, distinct pairs
    int64_t Ttot = 0;                     // packed positions of the call
    int D = 0;                            // distinct source ids
    int64_t MC = 0; size_t MCS = 0;       // packed positions per chunk, and rows of every workspace buffer (MC + slack)
    float* TBL = nullptr; T* TBL16 = nullptr; float* TBLST = nullptr;      // the hoisted table: fp32, or folded (16-bit sums + statistics)
    const float* lang_vec = nullptr;
    const float scaling = 1.0f / std::sqrt((float)(H / c.heads));
    // lever 5 (plan_single_rows): single rows of the call (0: not taken), and the maps of the position-0 block on the device
    int n_s = 0;
    const int32_t* cls_slot = nullptr;    // [N] vocabulary row -> buffer row of its position 0
    const int64_t* cls_row = nullptr;     // [N] buffer row -> vocabulary row
    const int64_t* out_rows = nullptr;    // [N] buffer row -> row of the outputs: cls_row, or a destination's own map behind it
    // lever 6 (id_qkv_rows): rows of the table in use (0: not taken) and U [Du, 3H] = their product with layer 0's folded qkv
    int Du = 0;
    T* U = nullptr;

    int run() {
        h->stats = zett_stats{};
        h->stats.rows = N;
        h->ev_used = 0;
        h->gemm_log.clear();
        R.timing = h->opt.time_gemm != 0;
        if (int rc = take_plan()) return rc;
        SlotGuard guard{h, ps, st};
        if (int rc = read_plan()) return rc;
        if (int rc = reserve()) return rc;
        // ---- table: input_projection once per distinct source id (A2-A4) -----------------
        if (!ext)
            table_phase<T>(R, lane_workspace<T>(h, 0, MCS), p.id_list, 0, D, src, src_dtype, MC, mode.table_lo, TBL16, TBLST, TBL);
        id_qkv_rows();
        if (R.rc) return R.rc;
        if (int rc = plan_single_rows()) return rc;      // (host work, under the table phase enqueued above)
        if (int rc = run_chunks(guard)) return rc;
        h->out_recorded = true;          // (ps.released — the plan slot may be rewritten behind it, zett_forward_prepare — is recorded by the guard)
        return h->opt.time_gemm ? read_gemm_timing(h, st) : 0;
    }

    // ---- plan ---------------------------------------------------------------------
    // The slot the previous forward did not use.  Prepared for exactly this call (zett_forward_prepare): its plan ran on the
    // plan stream, the host waits for THAT (not for earlier work on st) and st is ordered behind it.  Otherwise the plan is
    // made here, on st, and the host waits for it — and so for whatever was enqueued on st before.
    int take_plan() {
        PlanSlot& s = h->plan[h->plan_cur ^ 1];
        if (s.pending && s.sfm == sfm && s.n_rows == N && s.seq == seq && s.pair_plan == plan_layout(h, &s, N, seq).pair_plan &&
            s.ext_id_slot == (ext ? ext->id_slot : nullptr) && s.local_slots == id_qkv_configured(h)) {
            HIP_TRY(hipStreamWaitEvent(st, s.done, 0));
        } else {
            if (s.pending) HIP_TRY(hipEventSynchronize(s.done));       // a prepared plan nobody took: let it finish before the slot is reused
            if (s.released) HIP_TRY(hipStreamWaitEvent(st, s.released, 0));      // (the forward before the previous one read this slot)
            if (int rc = enqueue_plan(h, s, ext, sfm, N, seq, st)) return rc;
        }
        s.pending = false;
        h->plan_cur ^= 1;
        ps = &s;
        return 0;
    }

    // The host's one wait: the plan's counters and error word, and — (zett_forward_into) — the row map against the destination,
    // answered with the plan's error word: on `stream`, behind whatever wrote the map (with a prepared plan the host therefore
    // waits for `stream` too).
    int read_plan() {
        const PlanLayout PL = plan_layout(h, ps, N, seq);
        p = PL.p;
        pair_plan = PL.pair_plan;
        if (!h->opt.range_accumulate) HIP_TRY(hipMemsetAsync(h->range_word.p, 0, 4, st));          // range guard: the word of THIS forward (zett_check_range)
        for (Event& e : h->out_ready)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e.e, hipEventDisableTiming));
        const bool dest_check = dest && dest->rows;
        if (dest_check) {
            if (int rc = h->dest_word.reserve(4)) return rc;
            if (!h->dest_host.p) HIP_TRY(h->dest_host.alloc(4));
            if (!h->dest_checked) HIP_TRY(hipEventCreateWithFlags(&h->dest_checked.e, hipEventDisableTiming));
            HIP_TRY(hipMemsetAsync(h->dest_word.p, 0, 4, st));
            hipLaunchKernelGGL(dest_rows_check_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, dest->rows, N, dest->n_dest_rows, h->dest_word.as<int32_t>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h->dest_host.p, h->dest_word.p, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(h->dest_checked, st));
        }
        HIP_TRY(hipEventSynchronize(ps->done));
        hoff = ps->host.p;
        if (int rc = plan_error(h, hoff[N + 2])) return rc;          // an id outside the vocabulary, or (a caller's table) one the table does not hold
        if (dest_check) {
            HIP_TRY(hipEventSynchronize(h->dest_checked));
            if (h->dest_host.p[0] != 0)
                return fail(ZETT_E_INDEX, "destination row map: rows[%d] is outside the destination's %lld rows", h->dest_host.p[0] - 1, (long long)dest->n_dest_rows);
        }
        Ttot = hoff[N];
        D = hoff[N + 1];
        h->stats.packed_tokens = Ttot;
        h->stats.distinct_ids = D;
        h->stats.distinct_positions = Ttot;
        return 0;
    }

    // ---- workspace ------------------------------------------------------------------
    int reserve() {
        const WorkspaceSizes ws = workspace_sizes(c, sizeof(T), seq, Ttot, D, h->opt.max_chunk_tokens);
        MC = ws.chunk_tokens;
        MCS = (size_t)MC + 768;      // slack rows: the 384-row GEMM tile reads whole tiles of A (per lane, two lanes)
        if (int rc = reserve_workspace(h, ws, mode.fold, true)) return rc;
        R.a_rows_readable = (long)MCS;
        // (ABI 8) zett_forward_table: the table is the caller's — rows of the GLOBAL distinct-id list in the folded 16-bit layout,
        // computed by zett_table_rows here and on the peer ranks; tok_slot already holds global slots (enqueue_plan)
        if (ext && !mode.table_lo) return needs_folded_table("zett_forward_table");
        TBL = h->table.as<float>();
        // (lever 6: the call's rows of a caller's table are gathered into the handle's own table — gather_ext_table — and read from there)
        const bool ext_direct = ext && !id_qkv_configured(h);
        TBL16 = ext_direct ? (T*)const_cast<void*>(ext->table) : (T*)h->table.as<float>();
        TBLST = ext_direct ? const_cast<float*>(ext->stats) : (float*)((char*)h->table.as<float>() + (((size_t)D * H * sizeof(T) + 15) / 16) * 16);
        lang_vec = c.embed_lang ? md.lang + (size_t)lang_index * H : nullptr;
        return reserve_id_qkv(ws);
    }

    // ---- lever 6: layer 0's Q/K/V once per distinct source id ----------------------------
    // Taken from the configuration and the options alone (so that every call shape of a handle — shards, chunks, pairs or not, a
    // caller's table — computes layer 0 the same way, bit for bit): the folded 16-bit table, layer 0 not the position-0-only layer,
    // no language position (zett_finalize built the operands), and hidden >= ID_QKV_MIN_HIDDEN unless the option says "whenever possible".
    // U [Du, 3H] lives for the whole call (every chunk reads it).  X0 is written and read by the table phase only, which is over
    // before U's GEMM is enqueued: U goes there when it fits (MCS x n_in_embd against Du x 3H elements: the whole vocabulary of the
    // headline does, 131 840 x 8192 against 29 187 x 12 288).  No workspace buffer is large enough for EVERY call shape (a call whose
    // positions are all distinct ids), so otherwise the table allocation
    // grows by Du x 3H elements behind the table's own rows and statistics — outside zett_workspace_bytes, like single_map.
    int reserve_id_qkv(const WorkspaceSizes& ws) {
        h->id_qkv_last = 0;
        if (!id_qkv_configured(h) || !mode.table_lo || D <= 0) return 0;      // (a caller's table without table_lo was refused above)
        Du = D;
        const size_t u_bytes = (size_t)Du * 3 * H * sizeof(T);
        if (ws.x0 >= u_bytes) {
            U = h->x0.as<T>();
        } else {
            const size_t own = round_up(round_up((size_t)D * H * sizeof(T), 16) + (size_t)D * 8, 256);
            if (int rc = h->table.reserve(own + u_bytes)) return rc;
            TBL = h->table.as<float>();
            TBL16 = (T*)h->table.p;
            TBLST = (float*)((char*)h->table.p + round_up((size_t)D * H * sizeof(T), 16));
            U = (T*)((char*)h->table.p + own);
        }
        h->id_qkv_last = Du;
        return 0;
    }

    // U = ln_affine(table rows) (gamma (.) W_qkv)^T as a LayerNorm-fold consumer launch on the raw 16-bit table and its statistics.
    // With a caller's table (zett_forward_table) the rows of THIS call's distinct ids are first copied out of it, in the order of the
    // plan's own slots (id_list), into the handle's table: U then costs the call's ids, not the whole vocabulary's, and everything
    // behind reads the copy — the same bits.
    void id_qkv_rows() {
        if (!Du || R.rc) return;
        if (ext) {
            if constexpr (sizeof(T) == 2) launch_table_gather<T>(st, (const T*)ext->table, ext->stats, ext->id_slot, p.id_list, D, H, TBL16, TBLST);
            R.check("table_gather");
        }
        GemmEpilogue<T> e = R.epi();
        e.bias = md.id_u.b; e.out_lo = U; e.ld_lo = 3 * H;
        e.fold_stats = TBLST; e.fold_c = md.id_u.c;
        R.gemm(TBL16, H, (const T*)md.id_u.w, H, Du, 3 * H, H, e);
    }

    // ---- lever 5: rows with a single kept position --------------------------------------
    // Such a row (row_offset[n + 1] - row_offset[n] == 1 in a call with seq + lang > 1: never a uniform row, and its one position is
    // a visible key) attends to exactly one key: the softmax weight is exactly 1 and its context is its own value row, bit for bit
    // (attention_rows_kernel), so its query and key are never needed.  The host orders the position-0 block singles first — stable
    // within both groups — from the row offsets it already holds; the GEMMs then skip those rows with a pointer offset: Q|K of a
    // middle layer over buffer rows [n_s, m), the last layer's K over [n_s, m) and its query over [n_s, rows); V over every row.  The
    // Q/K cells of single rows stay unwritten and are never read.  The block is read out through cls_row (readout, heads).
    // Taken for a call that is ONE chunk on one lane; auto: when floor(n_s / 256) * (2H / 256) tiles — what a middle layer's Q|K
    // launch loses — fill at least one round of the 256 CUs (less only empties part of a last round that is partly empty anyway).
    int plan_single_rows() {
        h->single_rows_last = 0;
        if (!h->opt.single_rows || seq + (c.embed_lang ? 1 : 0) <= 1 || Ttot > MC || two_lanes()) return 0;
        int64_t ns = 0;
        for (int64_t n = 0; n < N; ++n) ns += hoff[n + 1] - hoff[n] == 1;
        if (ns == 0 || (h->opt.single_rows == 1 && (ns / 256) * (int64_t)(2 * H / 256) < 256)) return 0;
        const size_t map_bytes = (size_t)N * 12, comp_at = round_up(map_bytes, 16);
        if (h->single_copied) HIP_TRY(hipEventSynchronize(h->single_copied));      // the staging's last copy has left it
        else HIP_TRY(hipEventCreateWithFlags(&h->single_copied.e, hipEventDisableTiming));
        if (h->single_host_bytes < map_bytes) {
            h->single_host_bytes = 0;
            HIP_TRY(h->single_host.alloc(map_bytes));
            h->single_host_bytes = map_bytes;
        }
        if (int rc = h->single_map.reserve(comp_at + (size_t)N * 8)) return rc;
        int64_t* hrow = (int64_t*)h->single_host.p;
        int32_t* hslot = (int32_t*)(hrow + N);
        int64_t at_single = 0, at_other = ns;
        for (int64_t n = 0; n < N; ++n) {
            const int64_t slot = hoff[n + 1] - hoff[n] == 1 ? at_single++ : at_other++;
            hslot[n] = (int32_t)slot;
            hrow[slot] = n;
        }
        HIP_TRY(hipMemcpyAsync(h->single_map.p, h->single_host.p, map_bytes, hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(h->single_copied, st));
        n_s = (int)ns;
        cls_row = h->single_map.as<int64_t>();
        cls_slot = (const int32_t*)(cls_row + N);
        out_rows = cls_row;
        if (dest && dest->rows) {
            int64_t* comp = (int64_t*)((char*)h->single_map.p + comp_at);
            hipLaunchKernelGGL(compose_rows_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, dest->rows, cls_row, N, comp);
            HIP_TRY(hipGetLastError());
            out_rows = comp;
        }
        h->single_rows_last = ns;
        return 0;
    }

    // ---- encoder + heads over row chunks -----------------------------------------------
    // Buffer rows of a chunk are ordered POSITION 0 FIRST (rowops.hip.h chunk_row): rows [0, rows) are position 0 of the
    // chunk's vocabulary rows, the other packed positions follow.  What the last layer and the heads consume — position 0
    // only (modeling_hypernet.py:234) — is then the first `rows` rows of every buffer, with no gather in between.
    // (Lever 5 taken: that block is permuted, single rows first — cls_slot / cls_row above.)
    // One chunk = vocabulary rows [r0, r1) on one LANE: a stream and a slice of every workspace buffer starting `off` rows in.
    // Normally there is one lane (the caller's stream, offset 0) and the chunks follow each other.  A call that is ONE chunk
    // can instead run as two half-vocabulary chunks on two lanes at once (r4, "concurrent_lanes"): rows are independent, so the
    // two chains of launches interleave on the chip workgroup by workgroup — the last, partly filled round of 256 CUs of one
    // chain's GEMM is filled by the other's, and one chain's prologues / epilogues run under the other's K loops.  That is what
    // a 4 096-row shard of 8 GPUs needs: its N = 4096 launches are 608 tiles = 2.375 rounds.  (Same bits: a row's arithmetic
    // does not depend on the chunk it is in.)  ev_mode: 0 = no completion events, 1 = record out_ready on this lane's stream,
    // 2 = lane 1 of a pair (records lane_ev[1..3]), 3 = lane 0 of a pair (out_ready follows lane 1's events).
    struct Chunk {
        int64_t r0; int rows, tok0, m; hipStream_t st; int ev_mode; Workspace<T> w;
        // hidden state = (sum buffer, statistics, gamma, beta); the embeddings' LayerNorm starts it in (Zf, STb)
        float* hs_sum; float* hs_stats; const float* hs_gamma; const float* hs_beta;
        int zrows;                // rows of the current hidden state: m, or `rows` (position 0 only) in a position-0-only last layer
        bool raw = false;         // Zt = 16-bit copy of the un-normalised sum (LayerNorm fold) instead of the LayerNorm output
        bool pairs = false;       // lever 4 taken: until layer 0's attention output the hidden state exists per distinct pair only
        int P = 0;                // distinct (source id, position) pairs of the call
        float* other(float* b) const { return b == w.Zf ? w.PRE : w.Zf; }
        float* other_stats(float* b) const { return b == w.STa ? w.STb : w.STa; }
    };

    int run_chunk(int64_t r0, int64_t r1, hipStream_t lane_st, size_t off, int ev_mode) {
        Chunk k{r0, (int)(r1 - r0), hoff[r0], hoff[r1] - hoff[r0], lane_st, ev_mode, lane_workspace<T>(h, off, MCS)};
        h->stats.chunks += 1;
        R.st = lane_st;
        R.stage_lane = ev_mode == 2 ? 1 : 0;      // (the staged fallback of the destination store: each lane of a pair has its own buffer)
        R.a_rows_readable = k.w.a_rows;
        embeddings(k);
        for (int l = 0; l < c.layers && !R.rc; ++l) {
            attention(k, l, md.layers[l]);
            feed_forward(k, l, md.layers[l]);
        }
        if (R.rc) return R.rc;
        if (int rc = readout(k)) return rc;
        return heads(k);
    }

    // RobertaEmbeddings: table row + position (+ language) + token type, LayerNorm.
    // Lever 4: the embeddings' output depends on (source id, position) only, so the embeddings' LayerNorm and layer 0's
    // Q/K/V are computed once per DISTINCT pair (P rows instead of m).  The attention kernel reads a packed position's
    // q / k / v through tok_pair, and layer 0's attention-output epilogue adds the residual row of the position's pair
    // (GemmEpilogue::res_index = pair slot per buffer row): until that GEMM has run, the hidden state (operand, sum,
    // statistics) exists per pair only.  Same values, same bits.  Taken when the call is one chunk and at least 15 % of
    // the positions repeat a pair.
    void embeddings(Chunk& k) {
        LnEmbed emb{TBL, p.tok_slot, p.tok_pos, md.token_type, md.position, lang_vec, seq, p.tok_row, p.row_offset, k.r0, k.rows,
                    mode.table_lo ? (const void*)TBL16 : nullptr, TBLST, md.in_block.ln.w, md.in_block.ln.b, cls_slot};
        k.hs_sum = k.w.Zf;
        k.hs_stats = k.w.STb;
        k.hs_gamma = md.emb_ln.w;
        k.hs_beta = md.emb_ln.b;
        k.zrows = k.m;
        k.P = pair_plan ? hoff[N + 3] : 0;
        k.pairs = pair_plan && k.rows == N && k.P > 0 && (int64_t)k.P * 100 <= (int64_t)k.m * 85;
        float* sum = mode.lo_stream ? (float*)nullptr : k.hs_sum;
        if (k.pairs) {
            emb.tok_slot = p.pair_tslot; emb.tok_pos = p.pair_pos; emb.tok_row = nullptr;
            R.layernorm(nullptr, k.P, k.hs_gamma, k.hs_beta, c.ln_eps_encoder, nullptr, k.w.Zt, k.hs_stats, LnReadout{}, -1, &emb, 0, sum);
            // p.tok_pkey becomes the pair slot of every buffer row (the keys are dead once plan_pairs_kernel has run)
            hipLaunchKernelGGL(pair_rows_kernel, dim3((k.m + 255) / 256), dim3(256), 0, k.st, k.m, k.tok0, k.r0, k.rows, p, p.tok_pkey, cls_slot);
            R.check("pair_rows");
            h->stats.distinct_positions = k.P;
        } else {
            R.layernorm(nullptr, k.m, k.hs_gamma, k.hs_beta, c.ln_eps_encoder, nullptr, k.w.Zt, k.hs_stats, LnReadout{}, -1, &emb, k.tok0, sum);
        }
    }

    // Self-attention of layer l: fused QKV (per distinct pair in layer 0 under lever 4), attention_rows_kernel into CTX.
    void attention(Chunk& k, int l, const Layer& L) {
        const Workspace<T>& w = k.w;
        const bool cls_only = h->opt.cls_only_last && l == c.layers - 1;
        // raw: Zt holds the 16-bit copy of the pre-LayerNorm sum (LayerNorm fold: the previous layer's FFN-down wrote it
        // with the statistics in hs_stats) instead of the normalised operand — then this layer's QKV runs on the folded weight
        const T* wqkv = k.raw ? (const T*)L.fold_qkv.w : R.W(L.qkv);
        const float* bqkv = k.raw ? L.fold_qkv.b : L.qkv.b;
        const float* cqkv = k.raw ? L.fold_qkv.c : nullptr;
        // columns [col0, col0 + cols) of [q | k | v] for buffer rows [row0, M), into the same rows of `out` (leading dimension ld)
        auto qkv = [&](int col0, int cols, int row0, int M, T* out, size_t ld) {
            GemmEpilogue<T> e = R.epi();
            e.bias = bqkv + col0; e.out_lo = out + (size_t)row0 * ld; e.ld_lo = (int)ld;
            if (k.raw) { e.fold_stats = k.hs_stats + 2 * (size_t)row0; e.fold_c = cqkv + col0; }
            R.a_rows_readable = k.w.a_rows - row0;
            R.gemm(w.Zt + (size_t)row0 * H, H, wqkv + (size_t)col0 * H, H, M - row0, cols, H, e);
            R.a_rows_readable = k.w.a_rows;
        };
        const bool by_pair = !cls_only && k.pairs && l == 0;       // Zt holds the P pair rows; BIG gets their Q/K/V
        const T* Q = w.BIG;                               // [m | P, 3H]: q | k | v
        const T* KV = w.BIG + H;
        size_t ld_q = (size_t)3 * H, ld_kv = (size_t)3 * H;
        if (Du && l == 0 && !cls_only) {
            // lever 6: the rows from U (per pair, or per buffer row in the order the embeddings' LayerNorm wrote its statistics in);
            // independent of lever 5 — every row gets its q | k | v
            if constexpr (sizeof(T) == 2) {
                const PairQkvRows rw = by_pair ? PairQkvRows{p.pair_tslot, p.pair_pos, 0, nullptr, nullptr, 0, 0, nullptr}
                                               : PairQkvRows{p.tok_slot, p.tok_pos, k.tok0, p.tok_row, p.row_offset, k.r0, k.rows, cls_slot};
                launch_pair_qkv<T>(k.st, U, rw, by_pair ? k.P : k.m, k.hs_stats, md.id_cpos, seq, md.id_cw, md.id_bq, 3 * H, w.BIG, ld_q, h->range_word.p);
                R.check("pair_qkv");
            }
        } else if (!cls_only) {
            if (n_s && !by_pair) {          // lever 5: no query / key for the single rows, which are buffer rows [0, n_s)
                qkv(0, 2 * H, n_s, k.m, w.BIG, ld_q);
                qkv(2 * H, H, 0, k.m, w.BIG + 2 * H, ld_q);
            } else {
                qkv(0, 3 * H, 0, by_pair ? k.P : k.m, w.BIG, ld_q);
            }
        } else {
            // Only hidden[:,0] is consumed after this layer (modeling_hypernet.py:234): keys and values for every
            // position, the query (and everything downstream) for position 0 = the first `rows` rows of the
            // hidden state (sum, statistics and 16-bit operand alike).
            KV = w.BIG; Q = w.BIG + (size_t)k.m * 2 * H;
            ld_q = (size_t)H; ld_kv = (size_t)2 * H;
            if (n_s) {                                                   // lever 5: K and the query without the single rows
                qkv(H, H, n_s, k.m, w.BIG, ld_kv);
                qkv(2 * H, H, 0, k.m, w.BIG + H, ld_kv);
            } else {
                qkv(H, 2 * H, 0, k.m, w.BIG, ld_kv);                     // KV [m, 2H]
            }
            qkv(0, H, n_s, k.rows, w.BIG + (size_t)k.m * 2 * H, ld_q);   // Q [rows, H]  (rows <= m, BIG holds >= m x 3H)
            k.zrows = k.rows;
        }
        launch_attention<T>(k.st, H, h->opt.attention_fast, h->opt.attention_pack, Q, ld_q, KV, KV + H, ld_kv, H / c.heads, p.row_offset, p.row_uniform, p.tok_key,
                            k.r0, k.rows, k.tok0, scaling, cls_only ? 1 : 0, by_pair ? (const int32_t*)p.tok_pair : (const int32_t*)nullptr, w.CTX, cls_slot, n_s ? 1 : 0);
        R.check(cls_only ? "attention(position 0)" : "attention");
    }

    // The rest of layer l on CTX: attention output + residual, intermediate, FFN output + residual; the LayerNorms in between are
    // launches (fp32 modes), or folded into the GEMMs around them.
    void feed_forward(Chunk& k, int l, const Layer& L) {
        const Workspace<T>& w = k.w;
        const bool last = l == c.layers - 1, fold = mode.fold, lo_stream = mode.lo_stream;
        const int zrows = k.zrows;
        // attention output: sum = dense(ctx) + LN(hidden)   (the residual is the LayerNorm of hs_sum, recomputed)
        float* s1 = k.other(k.hs_sum);
        float* st1 = k.other_stats(k.hs_stats);
        GemmEpilogue<T> eo = R.epi();
        eo.bias = L.attn_out.b;
        if (k.pairs && l == 0) eo.res_index = p.tok_pkey;       // hs_sum / hs_stats are still per pair here
        if (lo_stream) {
            // the hidden state is Zt: the embeddings' LayerNorm output itself (layer 0: used as stored), or the raw 16-bit
            // sum of the previous layer with its statistics; the new sum goes to Ct
            eo.residual_lo = w.Zt; eo.ld_res_lo = H;
            if (k.raw) { eo.res_stats = k.hs_stats; eo.res_gamma = k.hs_gamma; eo.res_beta = k.hs_beta; }
            eo.out_lo = w.Ct; eo.ld_lo = H; eo.stats_part = w.PARTS; eo.ld_part = w.ld_parts;
        } else {
            eo.residual = k.hs_sum; eo.ld_res = H;
            eo.res_stats = k.hs_stats; eo.res_gamma = k.hs_gamma; eo.res_beta = k.hs_beta;
            eo.out_f32 = s1; eo.ld_f32 = H;
            if (fold) { eo.out_lo = w.Zt; eo.ld_lo = H; eo.stats_part = w.PARTS; eo.ld_part = w.ld_parts; }
        }
        R.gemm(w.CTX, H, R.W(L.attn_out), H, zrows, H, H, eo);
        const float* g1 = L.attn_ln.w;
        const float* b1 = L.attn_ln.b;
        const T* mid = lo_stream ? w.Ct : w.Zt;                  // 16-bit operand of intermediate.dense
        GemmEpilogue<T> ei = R.epi();
        ei.act = ACT_GELU_ERF; ei.out_lo = w.BIG; ei.ld_lo = I;
        if (fold) {          // the attention-output LayerNorm is folded into intermediate.dense
            R.ln_stats(w.PARTS, w.ld_parts, zrows, c.ln_eps_encoder, st1);
            ei.bias = L.fold_up.b; ei.fold_stats = st1; ei.fold_c = L.fold_up.c;
            R.gemm(mid, H, (const T*)L.fold_up.w, H, zrows, I, H, ei);
        } else {
            R.layernorm(s1, zrows, g1, b1, c.ln_eps_encoder, nullptr, w.Zt, st1);
            ei.bias = L.up.b;
            R.gemm(w.Zt, H, R.W(L.up), H, zrows, I, H, ei);
        }
        // FFN output: sum = dense(gelu) + LN(s1)
        float* s2 = k.other(s1);
        float* st2 = k.other_stats(st1);
        GemmEpilogue<T> ef = R.epi();
        ef.bias = L.down.b;
        if (lo_stream) {      // (also in the last layer: the readout takes the 16-bit sum)
            ef.residual_lo = w.Ct; ef.ld_res_lo = H; ef.res_stats = st1; ef.res_gamma = g1; ef.res_beta = b1;
            ef.out_lo = w.Zt; ef.ld_lo = H; ef.stats_part = w.PARTS; ef.ld_part = w.ld_parts;
        } else {
            ef.residual = s1; ef.ld_res = H;
            ef.res_stats = st1; ef.res_gamma = g1; ef.res_beta = b1;
            ef.out_f32 = s2; ef.ld_f32 = H;
            if (fold && !last) { ef.out_lo = w.Zt; ef.ld_lo = H; ef.stats_part = w.PARTS; ef.ld_part = w.ld_parts; }
        }
        R.gemm(w.BIG, I, R.W(L.down), I, zrows, H, I, ef);
        k.hs_gamma = L.out_ln.w;
        k.hs_beta = L.out_ln.b;
        k.hs_sum = s2; k.hs_stats = st2;
        // (the last layer's output LayerNorm is the readout: position 0 only, whatever the layer computed)
        if (!last) {
            if (fold) { R.ln_stats(w.PARTS, w.ld_parts, zrows, c.ln_eps_encoder, st2); k.raw = true; }
            else R.layernorm(s2, zrows, k.hs_gamma, k.hs_beta, c.ln_eps_encoder, nullptr, w.Zt, st2);
        }
    }

    // an output of the chunk is complete (zett_stream_wait_output): lane 1 of a pair records `lane_ev`, lane 0 waits for it first
    int output_ready(const Chunk& k, int which, hipEvent_t lane_ev) {
        if (k.ev_mode == 2) HIP_TRY(hipEventRecord(lane_ev, k.st));
        if (k.ev_mode == 3) HIP_TRY(hipStreamWaitEvent(k.st, lane_ev, 0));
        if (k.ev_mode == 1 || k.ev_mode == 3) HIP_TRY(hipEventRecord(h->out_ready[which], k.st));
        return 0;
    }

    // position-0 readout + bias head (modeling_hypernet.py:231-234, 260-265) = the last LayerNorm, on the first `rows`
    // buffer rows: Cf = fp32 hidden[:,0] (residual of the heads' ProjectorBlocks), Ct its operand copy, bias head fused.
    // (no encoder layer: the embeddings' LayerNorm is simply taken again for those rows)
    // (zett_forward_into: the bias goes to the destination's bias vector — row map offset to the chunk, or the identity from r0 on.
    //  A destination without one still takes the READOUT instantiation — only it reads the 16-bit residual stream — into a
    //  workspace vector that nothing reads)
    int readout(Chunk& k) {
        LnReadout ro{md.bias.w, md.bias.b, out_bias ? out_bias + k.r0 : nullptr};      // (bias projection: null without hn_predict_bias)
        int bias_dtype = -1;
        if (dest && dest->bias) {
            const size_t bes = dest->bias_dtype == ZETT_F32 ? 4 : 2;
            ro.bias_rows = dest->rows ? dest->rows + k.r0 : nullptr;
            ro.out_bias = (float*)((char*)dest->bias + (dest->rows ? 0 : (size_t)k.r0 * bes));
            bias_dtype = dest->bias_dtype;
        } else if (dest) {
            if (int rc = h->dest_sink.reserve((size_t)N * sizeof(float))) return rc;      // (the whole call: both lanes of a pair share it)
            ro.out_bias = h->dest_sink.as<float>() + k.r0;
        }
        // lever 5: buffer row r is vocabulary row cls_row[r] — every bias goes through the row map (one chunk: r0 = 0), zett_forward's
        // fp32 vector through the fp32 destination store (the same bytes)
        if (n_s && (!dest || dest->bias)) {
            ro.bias_rows = out_rows;
            if (!dest) bias_dtype = ZETT_F32;
            else ro.out_bias = (float*)dest->bias;
        }
        ro.range_flag = h->range_word.p;
        ro.in_lo = mode.lo_stream ? (const T*)k.w.Zt : (const T*)nullptr;       // (16-bit residual stream: the rows are read from the 16-bit copy of the sum)
        R.layernorm(k.hs_sum, k.rows, k.hs_gamma, k.hs_beta, c.ln_eps_encoder, k.w.Cf, k.w.Ct, nullptr, ro, bias_dtype);
        return R.rc ? 0 : output_ready(k, ZETT_OUT_BIAS, h->lane_ev[1]);      // out_bias complete
    }

    // (zett_forward_into) a destination matrix as the heads of the chunk starting at vocabulary row r0 see it
    DestOut dest_out(void* base, int64_t ld, int64_t r0) const {
        const size_t es = dest->dtype == ZETT_F32 ? 4 : 2;
        if (n_s) return DestOut{base, out_rows, ld, dest->dtype};      // lever 5 (one chunk): the position-0 block's own order behind the caller's map
        return DestOut{dest->rows ? base : (void*)((char*)base + (size_t)r0 * (size_t)ld * es), dest->rows ? dest->rows + r0 : nullptr, ld, dest->dtype};
    }

    // One output head (modeling_hypernet.py:236-258): its ProjectorBlock on hidden[:,0], its Linear, its Rescaler, into rows
    // [r0, r0 + rows) of zett_forward's fp32 matrix `out` or of the destination's `dst`.  out_b / dst_b: the split single head, whose
    // columns from n_embd on are a second matrix.  mode.fold_heads: the block's LayerNorm is folded into the Linear (hd.fold).
    void head(const Chunk& k, const Head& hd, bool split, float* out, float* out_b, void* dst, int64_t ld_dst, void* dst_b, int64_t ld_dst_b) {
        const Workspace<T>& w = k.w;
        const bool fold = mode.fold_heads;
        const Folded& f = hd.fold;
        if (fold) R.projector(hd.block, w.Ct, w.Cf, k.rows, w.BIG, w.PRE, nullptr, w.CTX, w.PARTS, w.ld_parts, w.STa);
        else R.projector(hd.block, w.Ct, w.Cf, k.rows, w.BIG, w.PRE, nullptr, w.CTX);
        GemmEpilogue<T> e = R.epi();
        e.bias = fold ? f.b : hd.out.b;
        e.scale = c.rescale ? hd.scale : (fold ? md.head_one : nullptr);
        e.shift = c.rescale ? hd.shift : (fold ? md.head_zero : nullptr);
        if (fold) { e.fold_stats = w.STa; e.fold_c = f.c; }
        e.ld_f32 = E; e.range_final = 1;
        if (split) e.split_col = E;
        const int width = split ? 2 * E : E;
        const T* wl = fold ? (const T*)f.w : R.W(hd.out);
        if (dest) {
            const DestOut d = dest_out(dst, ld_dst, k.r0), d_b = split ? dest_out(dst_b, ld_dst_b, k.r0) : DestOut{};
            R.head_gemm(w.CTX, wl, k.rows, width, H, e, &d, split ? &d_b : nullptr, E);
        } else if (n_s) {      // lever 5: zett_forward's fp32 matrices through the fp32 destination store and cls_row (the same bytes)
            const DestOut d{out, out_rows, E, ZETT_F32}, d_b{out_b, out_rows, E, ZETT_F32};
            R.head_gemm(w.CTX, wl, k.rows, width, H, e, &d, split ? &d_b : nullptr, E);
        } else {
            e.out_f32 = out + (size_t)k.r0 * E;
            if (split) e.out_f32_b = out_b + (size_t)k.r0 * E;
            R.gemm(w.CTX, H, wl, H, k.rows, width, H, e);
        }
    }

    int heads(const Chunk& k) {
        const bool split = c.single_head && c.separate_out;      // one head of 2 * n_embd columns: [in | out]
        head(k, md.head_in, split, out_in, out_out, dest ? dest->in : nullptr, dest ? dest->ld_in : 0, dest ? dest->out : nullptr, dest ? dest->ld_out : 0);
        if (!R.rc)           // out_in complete: the second head runs behind it
            if (int rc = output_ready(k, ZETT_OUT_IN, h->lane_ev[2])) return rc;
        if (c.separate_out && !c.single_head)
            head(k, md.head_out, false, out_out, nullptr, dest ? dest->out : nullptr, dest ? dest->ld_out : 0, nullptr, 0);
        return R.rc;
    }

    // two lanes?  Only a call that is one chunk and would not take the pair lever (which needs the whole call in one chunk and is
    // worth more).  auto = the launches of width H (attention output, FFN down: the fewest tiles) would leave more than 8 % of the
    // CU-rounds they occupy idle, on a hypernet wide enough for that to be the cost (H >= 1024), and per-launch timing is off
    // (concurrent launches share the chip: their HIP-event durations overlap and would be counted twice).
    // Measured (r4, same box, Mistral shape): 4 096 rows 9.25 -> 9.11 ms; 8 192 rows 16.14 -> 16.12; 16 384 rows and every full
    // vocabulary slower (28.9 -> 29.8; headline 53.1 -> 55.2 with the pair lever lost): the dispatcher interleaves the two
    // chains' workgroups, but each 256x256 tile still owns its CU, so only the partial last rounds gain.
    bool two_lanes() const {
        if (!h->opt.concurrent_lanes || Ttot > MC || N < 512) return false;
        const int Pn = pair_plan ? hoff[N + 3] : 0;
        const bool pairs_taken = pair_plan && Pn > 0 && (int64_t)Pn * 100 <= Ttot * 85;
        const double r = (double)((Ttot + 255) / 256) * (double)((H + 255) / 256) / 256.0;
        return h->opt.concurrent_lanes == 2 || (!pairs_taken && !h->opt.time_gemm && H >= 1024 && r < 4.0 && (std::ceil(r) - r) / std::ceil(r) > 0.08);
    }

    // lane selection and the join
    int run_chunks(SlotGuard& guard) {
        if (two_lanes()) {
            if (!h->lane_stream) HIP_TRY(hipStreamCreateWithFlags(&h->lane_stream.s, hipStreamNonBlocking));
            for (Event& e : h->lane_ev)
                if (!e) HIP_TRY(hipEventCreateWithFlags(&e.e, hipEventDisableTiming));
            // the split is a multiple of 256 rows (the position-0-only last layer and the heads keep their number of row tiles)
            int64_t ra = ((N / 2 + 128) / 256) * 256;
            ra = std::min<int64_t>(std::max<int64_t>(ra, 256), N - 1);
            const size_t off1 = (size_t)(hoff[ra] - hoff[0]) + 384;       // (the second lane's slice starts 384 rows behind the first one's rows)
            HIP_TRY(hipEventRecord(h->lane_ev[0], st));                       // fork: the plan and the table are complete
            HIP_TRY(hipStreamWaitEvent(h->lane_stream, h->lane_ev[0], 0));
            guard.lane_forked = true;                                         // (joined by the guard on every exit path)
            if (int rc = run_chunk(ra, N, h->lane_stream, off1, 2)) return rc;
            if (int rc = run_chunk(0, ra, st, 0, 3)) return rc;
        } else {
            int64_t r0 = 0;
            while (r0 < N) {
                int64_t r1 = r0 + 1;
                while (r1 < N && (int64_t)hoff[r1 + 1] - hoff[r0] <= MC) ++r1;
                if (int rc = run_chunk(r0, r1, st, 0, r1 == N ? 1 : 0)) return rc;
                r0 = r1;
            }
        }
        R.st = st;
        if (R.rc) return R.rc;
        if (guard.lane_forked) {                      // join now (the guard then has nothing left to join)
            HIP_TRY(hipEventRecord(h->lane_ev[3], h->lane_stream));
            HIP_TRY(hipStreamWaitEvent(st, h->lane_ev[3], 0));
            guard.lane_forked = false;
        }
        return 0;
    }
};

template <typename T>
int do_forward(zett_hypernet* h, const ExtTable* ext, const int32_t* sfm, int64_t N, int seq, const void* src, int src_dtype, const zett_dest* dest,
               int lang_index, float* out_in, float* out_out, float* out_bias, hipStream_t st) {
    Forward<T> f{h, ext, sfm, N, seq, src, src_dtype, dest, lang_index, out_in, out_out, out_bias, st};
    return f.run();
}

}  // namespace
