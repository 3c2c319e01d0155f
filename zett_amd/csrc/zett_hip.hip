// zett_hip.hip — C ABI of libzett_hip.so (see include/zett_hip.h).
//
// Host-side orchestration of the hypernet forward on one MI355X:
//
//   plan      surface forms -> packed positions, distinct referenced source ids
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
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "gemm.hip.h"
#include "gemm_launch.hip.h"
#include "rowops.hip.h"
#include "rowops_launch.hip.h"

using namespace zett;

namespace {

struct Tensor {
    float* f32 = nullptr;       // device fp32 copy (biases, LN, embeddings, ... and GEMM weights in F32 mode)
    void* lo = nullptr;         // GEMM operand copy in the handle's arithmetic type
    std::vector<int64_t> shape;
    size_t numel = 0;
};

inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }

// The model as the forward reads it: device pointers that own nothing (the handle's tensors and `owned` do), bound once by
// zett_finalize.  A GEMM operand (Linear::w, Folded::w) is in the handle's arithmetic type, everything else fp32.  What the
// config switches off stays null.
struct Linear { const void* w = nullptr; const float* b = nullptr; };
struct Affine { const float* w = nullptr; const float* b = nullptr; };      // LayerNorm (gamma, beta), Rescaler, bias projection
struct Projector { Linear dense1, dense2; Affine ln; };
// LayerNorm fold (16-bit modes): the gamma-folded operand of a GEMM that follows a LayerNorm, its row sums and beta-folded bias
struct Folded { void* w = nullptr; float* c = nullptr; float* b = nullptr; };
struct Layer {
    Linear q, k, v;                    // as the checkpoint has them: read by zett_finalize only, which fuses them into
    Linear qkv;                        // rows [q | k | v]: [3H, H], [3H]
    Linear attn_out, up, down; Affine attn_ln, out_ln;
    Folded fold_qkv, fold_up;          // qkv of layers >= 1 folded with the previous layer's out_ln, up with attn_ln
};
struct Head {
    Projector block; Linear out;
    const float* scale = nullptr; const float* shift = nullptr;      // Rescaler over the head's columns (first head: scaler | out_scaler for single_head)
    Folded fold;                       // `out` folded with the block's LayerNorm (not for the split single head: its two-destination epilogue is the generic one)
};
struct Model {
    const float* lang = nullptr; const float* token_type = nullptr; const float* position = nullptr; Affine emb_ln;
    std::vector<Layer> layers;
    const float* fallback = nullptr; Affine in_scaler, scaler, out_scaler, bias;
    Linear in_proj; Projector in_block;      // input_projection.0 / .1
    Head head_in, head_out;
    float* head_one = nullptr;         // [head_out_width] ones / zeros: the Rescaler of a config without hn_rescale_embeddings, for the
    float* head_zero = nullptr;        // folded head epilogue, which is compiled with it
    // Lever 6 (id_qkv; null where it is not possible): layer 0's fused qkv folded with BOTH LayerNorms in front of it, for the GEMM on
    // raw table rows — w = lo(gamma_t (.) gamma (.) W), c its row sums, b = (beta_t (.) gamma) W^T — and what the row kernel adds per
    // position and column: id_cpos [max_positions, 3H] = (type0 + pos[p]) (gamma (.) W)^T, id_cw = colsum(gamma (.) W), id_bq = beta W^T + b
    Folded id_u; float* id_cpos = nullptr; float* id_cw = nullptr; float* id_bq = nullptr;
};
// One weight of the declaration (declare_weights): its checkpoint name and shape, and the field of Model its device pointer goes
// to — `operand` for a GEMM operand (converted to the arithmetic type, fp32 original freed in the 16-bit modes), else `vec`.
struct WeightDecl { std::string name; std::vector<int64_t> shape; const void** operand; const float** vec; };

}  // namespace

constexpr int ID_QKV_MIN_HIDDEN = 4096;      // lever 6's default rule

struct zett_hypernet {
    zett_config cfg{};
    int device = 0;
    int precision = ZETT_PREC_BF16;
    bool finalized = false;
    std::map<std::string, Tensor> w;  // the uploaded tensors, by name: their owner (zett_load_weight, zett_finalize, zett_destroy)
    std::vector<WeightDecl> decl;     // every weight the library reads, sorted by name (zett_create); its slots point into `m`
    Model m;                          // what the forward reads
    int ln_fold = 1;
    std::vector<void*> owned;         // the fused / derived operands zett_finalize built: everything else to hipFree at destroy
    // options
    int64_t max_chunk_tokens = 0;          // 0 = auto: chunk_token_cap() below (131 072 at H = 4096, more for narrower hypernets)
    int time_gemm = 0;
    int cls_only_last = 1;
    int pair_dedupe = 1;              // layer 0's Q/K/V once per distinct (source id, position) pair (do_forward)
    int residual_lo = 1;              // 16-bit residual stream of the encoder (gemm4d LN16 producers): 1 = in f16 mode, 2 = in bf16 mode too (A/B), 0 = fp32 stream
    int concurrent_lanes = 0;         // a one-chunk call as TWO half-vocabulary chunks on two streams (do_forward): 0 never, 1 auto (when the narrow GEMMs
                                      // of the call leave > 8 % of their last round of 256 CUs idle: the 4 096-row shards of 8 GPUs), 2 always
    hipStream_t lane_stream = nullptr;
    hipEvent_t lane_ev[4] = {nullptr, nullptr, nullptr, nullptr};      // fork, lane 1: bias written / out_in written / done
    int attention_fast = 1;           // rows of <= 8 packed positions: keys / values fetched once, all keys of a query side by side (rowops.hip.h)
    int attention_pack = 1;           // a last column group of 256 / 128 / 64 columns (H = 768) takes 2 / 4 / 8 rows per wave instead of idle lanes (r6; same bits)
    int gemm_tail_split = 1;          // gemm4d: a launch's partly filled last round of 256 CUs as 128x256 tiles (gemm4d.hip.h gemm4d_row_split): 0 never,
                                      // 1 when the split is cheaper (default), 2 = cut every launch in the middle, 3 = half tiles only (tests: same bits)
    int gemm_tile_order = 0;          // gemm4d: 0 = column-tile-major groups, 1 = row-tile-major groups (A/B)
    int ln_rows8 = 1;                 // 16-bit modes, H <= 2048: LayerNorm launches on layernorm_rows8_kernel (eight columns per lane; rowops.hip.h); 0 = the float4 kernel (A/B)
    int table_lo = 1;                 // 16-bit hoisted table with the ProjectorBlock's LayerNorm folded into the embeddings' kernel (with the 16-bit residual stream); 0 = fp32 table (A/B)
    int gemm_group = 0;               // gemm4d: column (order 0) / row (order 1) tiles per group; 0 = the kernel's default, 4 (A/B)
    int gemm4d_min_k = 512;           // 16-bit launches with K >= this take the four-wave direct-to-LDS tile (r2: with the streamlined epilogues it is ahead of gemm8r down to K = 768: +1.8 % on the XLM-R workload)
    int gemm_variant = 0;             // 0 auto, 1 = 128x128, 2 = 256x256 register-staged (8 waves), 3 = 384x256 LDS-DMA,
                                      // 7 = 256x256 four-wave direct-to-LDS, 8 = as 7 with the generic epilogue drain
    // workspace
    // The plan of a forward (integers: packed positions, distinct ids, pairs) lives in one of TWO slots that forwards take in
    // turn, so that the plan of the NEXT forward can be made (zett_forward_prepare, on plan_stream) while the kernels of the
    // current one still read theirs.
    struct PlanSlot {
        DevBuf i32, u8;
        int32_t* host = nullptr;          // pinned: row offsets [N+1], distinct ids, error word, distinct pairs
        size_t host_ints = 0;
        hipEvent_t done = nullptr;        // the plan's kernels and copies have run
        hipEvent_t released = nullptr;    // the forward that used this slot has finished with it
        const int32_t* sfm = nullptr;     // what the slot was prepared for (zett_forward_prepare), pending until a forward takes it
        int64_t n_rows = 0;
        int seq = 0;
        bool pair_plan = false;           // the layout it was made with (an option changed in between: the forward plans again)
        const int32_t* ext_id_slot = nullptr;   // the id -> table-slot map its tok_slot was written with (null: the plan's own)
        bool local_slots = false;         // lever 6 was configured: tok_slot holds the plan's own slots even with a caller's table
        bool pending = false;
    } plan[2];
    PlanSlot table_plan;              // (ABI 8) scratch plan of zett_table_plan: the distinct ids of a WHOLE vocabulary, never taken by a forward
    // (ABI 8) the hoisted table of the forward in flight comes from the caller (zett_forward_table): rows of the global distinct-id
    // list computed by zett_table_rows — on this rank and on its peers — instead of this call's own distinct ids
    struct ExtTable { const void* table = nullptr; const float* stats = nullptr; const int32_t* id_slot = nullptr; } ext;
    int plan_cur = 0;                 // slot of the most recent forward
    hipStream_t plan_stream = nullptr;
    hipEvent_t plan_fork = nullptr;
    DevBuf table, x0, yf, yt, big, pre, ctx, cf, ct, lnstats, lnparts;
    hipEvent_t out_ready[2] = {nullptr, nullptr};      // zett_stream_wait_output: out_in / out_bias of the last forward complete
    bool out_recorded = false;
    int range_accumulate = 0;         // 1: zett_forward does not clear the range word, zett_check_range clears it after reading (a caller
                                      // that runs several asynchronous forwards and asks once at the end: zett_amd/sharding.py)
    int32_t* range_word = nullptr;    // device: zett_range_bits of the forward in flight (cleared when a forward starts)
    int32_t* range_host = nullptr;    // pinned: where zett_check_range / zett_finalize read it
    // (zett_forward_into) the row map's check against the destination (read with the plan's error word), and the fp32 rows of the head
    // launches that take the staged fallback of the destination store (Runner::head_gemm)
    // (dest_stage[1]: lane 1 of a "concurrent_lanes" pair — the two lanes' staged heads run at the same time)
    DevBuf dest_word, dest_stage[2], dest_sink;
    int32_t* dest_host = nullptr;
    hipEvent_t dest_checked = nullptr;
    // Lever 5 (Forward::plan_single_rows): rows with a single kept position first in the position-0 block, their query /
    // key GEMM rows skipped.  single_map — reserved only when a forward takes the lever, outside zett_workspace_bytes like dest_sink —
    // holds cls_row int64 [N] (buffer row -> vocabulary row), cls_slot int32 [N] (the inverse) and, behind them, the composition with a
    // caller's row map; single_host is the pinned staging of the first two, single_copied the event behind their copy.
    int single_rows = 1;              // 0 off, 1 auto (one chunk on one lane, at least one full round of 256x256 tiles saved per launch), 2 whenever possible
    int64_t single_rows_last = 0;     // single rows the last forward skipped (zett_single_rows)
    // Lever 6 (Forward::id_qkv_rows): layer 0's Q/K/V once per distinct source id
    int id_qkv = 1;                   // 0 off, 1 when possible and hidden >= ID_QKV_MIN_HIDDEN, 2 whenever possible
    int64_t id_qkv_last = 0;          // table rows layer 0's Q/K/V GEMM of the last forward ran on (zett_id_qkv)
    DevBuf single_map;
    void* single_host = nullptr;
    size_t single_host_bytes = 0;
    hipEvent_t single_copied = nullptr;
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    std::vector<zett_gemm_record> gemm_log;     // every GEMM launch of the last forward (zett_get_gemm_log); "time_gemm": launch k has the event pair ev[2k], ev[2k + 1]
    zett_stats stats{};
};

namespace {

size_t elt_size(int precision) { return precision == ZETT_PREC_F32 ? 4 : 2; }

// The ONE declaration of the model's weights (names and shapes: zett_amd/dims.py weight_shapes, minus the word-embedding table,
// which nothing reads): what zett_load_weight accepts, what zett_finalize requires, converts and binds.  m.layers is sized here.
std::vector<WeightDecl> declare_weights(const zett_config& c, Model& m) {
    const int64_t H = c.hidden, I = c.intermediate, E = c.n_embd, EIN = c.n_in_embd;
    std::vector<WeightDecl> d;
    auto vec = [&](const std::string& n, std::vector<int64_t> shape, const float*& slot) { d.push_back({n, std::move(shape), nullptr, &slot}); };
    auto linear = [&](const std::string& p, int64_t n, int64_t k, Linear& l) { d.push_back({p + "weight", {n, k}, &l.w, nullptr}); vec(p + "bias", {n}, l.b); };
    auto norm = [&](const std::string& p, Affine& a) { vec(p + "weight", {H}, a.w); vec(p + "bias", {H}, a.b); };
    auto scaler = [&](const std::string& p, int64_t n, Affine& a) { vec(p + "w", {1, n}, a.w); vec(p + "b", {1, n}, a.b); };
    auto block = [&](const std::string& p, Projector& b) { linear(p + "dense1.", I, H, b.dense1); linear(p + "dense2.", H, I, b.dense2); norm(p + "ln.", b.ln); };
    if (c.embed_lang) vec("lang_embeddings.weight", {c.n_langs, H}, m.lang);
    vec("model.embeddings.token_type_embeddings.weight", {1, H}, m.token_type);
    norm("model.embeddings.LayerNorm.", m.emb_ln);
    vec("model.embeddings.position_embeddings.weight", {c.max_positions, H}, m.position);
    m.layers.resize(c.layers);
    for (int l = 0; l < c.layers; ++l) {
        const std::string p = "model.encoder.layer." + std::to_string(l) + ".";
        Layer& L = m.layers[l];
        linear(p + "attention.self.query.", H, H, L.q); linear(p + "attention.self.key.", H, H, L.k); linear(p + "attention.self.value.", H, H, L.v);
        linear(p + "attention.output.dense.", H, H, L.attn_out); norm(p + "attention.output.LayerNorm.", L.attn_ln);
        linear(p + "intermediate.dense.", I, H, L.up);
        linear(p + "output.dense.", H, I, L.down); norm(p + "output.LayerNorm.", L.out_ln);
    }
    vec("fallback_embeddings.weight", {c.n_extra, EIN}, m.fallback);
    linear("input_projection.0.", H, EIN, m.in_proj); block("input_projection.1.", m.in_block);
    block("output_projection.0.", m.head_in.block); linear("output_projection.1.", c.single_head ? EIN : E, H, m.head_in.out);
    if (c.separate_out && !c.single_head) { block("output_projection_out.0.", m.head_out.block); linear("output_projection_out.1.", E, H, m.head_out.out); }
    if (c.rescale) {
        scaler("in_scaler.", EIN, m.in_scaler); scaler("scaler.", E, m.scaler);
        if (c.separate_out) scaler("out_scaler.", E, m.out_scaler);
    }
    if (c.predict_bias) { vec("bias_projection.weight", {1, H}, m.bias.w); vec("bias_projection.bias", {1}, m.bias.b); }
    std::sort(d.begin(), d.end(), [](const WeightDecl& a, const WeightDecl& b) { return a.name < b.name; });
    return d;
}

int validate_config(const zett_config& c, int precision) {
    if (c.n_embd <= 0 || c.hidden <= 0 || c.intermediate <= 0 || c.heads <= 0 || c.layers <= 0)
        return fail(ZETT_E_INVALID, "non-positive dimension in zett_config");
    if (c.n_in_embd != (c.separate_out ? 2 * c.n_embd : c.n_embd))
        return fail(ZETT_E_INVALID, "n_in_embd must be 2*n_embd iff separate_out");
    if (c.hidden % c.heads) return fail(ZETT_E_INVALID, "hidden %d not divisible by heads %d", c.hidden, c.heads);
    const int d = c.hidden / c.heads;
    if (d < 8 || d > 512 || (d & (d - 1))) return fail(ZETT_E_INVALID, "head_dim %d unsupported (need a power of two in [8,512])", d);
    const int kq = precision == ZETT_PREC_F32 ? 32 : 64;
    for (int k : {c.n_in_embd, c.hidden, c.intermediate})
        if (k % kq) return fail(ZETT_E_INVALID, "contraction width %d is not a multiple of %d", k, kq);
    if (c.n_embd % 4) return fail(ZETT_E_INVALID, "n_embd must be a multiple of 4");
    if (c.n_extra < 1) return fail(ZETT_E_INVALID, "n_extra must be >= 1 (reference allocates max(hn_n_extra_tokens,1))");
    if (c.pad_token_id < 0) return fail(ZETT_E_INVALID, "pad_token_id is required");
    if (c.embed_lang && c.n_langs <= 0) return fail(ZETT_E_INVALID, "hn_embed_lang_id needs n_langs");
    return 0;
}

// Device bytes zett_forward reserves, as a function of what the plan found (packed positions
// Ttot, distinct ids D).  One definition shared by the forward, zett_table_rows and zett_workspace_bytes.
struct WorkspaceSizes {
    int64_t chunk_tokens;
    size_t table, x0, f32_rows, lo_rows, big, stats, parts;
    size_t total() const { return table + x0 + 3 * f32_rows + 3 * lo_rows + big + stats + parts; }
};

static int64_t pair_keys(const zett_config& c, int seq) {
    return ((int64_t)c.original_vocab_size + c.n_extra + 1) * (int64_t)(seq + (c.embed_lang ? 1 : 0));
}

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

// Where the arrays of a plan lie in a slot (pure pointer arithmetic: the same answer when the plan is made and when a
// forward takes it).  Pair plan (lever 4): only where it can pay — at least two encoder layers (layer 0 must not be the
// position-0-only one), and a key space not much larger than the batch (a 250 k-id source vocabulary against 50 k rows
// repeats few pairs and would pay for clearing and scanning 2 M flags).
struct PlanLayout {
    PlanArrays p{};
    int32_t* scan_tmp = nullptr;
    bool pair_plan = false;
    int64_t PK = 0;
    size_t n_clear = 0;          // int32 words at the head of the arena that a plan starts from zero
    size_t words = 0;            // int32 words of the whole arena, scan scratch included
};
// s == null: sizes only (every pointer null).  worst_case: the arena of a plan WITH the pair plan, whatever the options say now.
static PlanLayout plan_layout(const zett_hypernet* h, const zett_hypernet::PlanSlot* s, int64_t N, int seq, bool worst_case = false) {
    const zett_config& c = h->cfg;
    const int lam = c.embed_lang ? 1 : 0;
    const int64_t V = (int64_t)c.original_vocab_size + c.n_extra;
    const int64_t max_tok = N * (int64_t)(seq + lam);
    PlanLayout L;
    PlanArrays& p = L.p;
    L.PK = pair_keys(c, seq);          // K = (V+1)(L+lang)
    L.pair_plan = worst_case || (h->pair_dedupe && c.layers >= 2 && L.PK <= std::max<int64_t>(4 * max_tok, (int64_t)1 << 23) && L.PK < (int64_t)0x7fffffff);
    int32_t* const base = s ? s->i32.as<int32_t>() : nullptr;
    auto take = [&](int32_t*& array, int64_t n) { array = base ? base + L.words : nullptr; L.words += (size_t)n; };
    // int32 arena, the one list of its arrays: what a plan clears first, in one piece — id_flag[V] pair_flag[PK] err[1] — then
    // row_count[N] row_offset[N+1] counters[3] (read by the host in one copy with the row offsets) id_slot[V+1] id_list[V]
    // tok_slot[T] tok_pos[T] tok_row[T] [pair plan: tok_pkey[T] tok_pair[T] pair_tslot[T] pair_pos[T] pair_slot[PK+1]] scan scratch
    take(p.id_flag, V);
    if (L.pair_plan) take(p.pair_flag, L.PK);
    take(p.err, 1);
    L.n_clear = L.words;
    take(p.row_count, N); take(p.row_offset, N + 1); take(p.counters, 3);
    take(p.id_slot, V + 1); take(p.id_list, V);
    take(p.tok_slot, max_tok); take(p.tok_pos, max_tok); take(p.tok_row, max_tok);
    p.n_pair_keys = L.pair_plan ? (int32_t)L.PK : 0;
    if (L.pair_plan) {
        take(p.tok_pkey, max_tok); take(p.tok_pair, max_tok); take(p.pair_tslot, max_tok); take(p.pair_pos, max_tok);
        take(p.pair_slot, L.PK + 1);
    }
    take(L.scan_tmp, 2 * (std::max<int64_t>(std::max<int64_t>(N, V), L.PK) / SCAN_CHUNK + 2) + 1);
    if (s) {
        p.row_uniform = s->u8.as<uint8_t>();
        p.tok_key = p.row_uniform + N;
    }
    return L;
}
// worst case of a slot's int32 arena for [N, seq] surface forms: what enqueue_plan reserves and zett_workspace_bytes counts
static size_t plan_i32_bytes(const zett_hypernet* h, int64_t N, int seq) { return plan_layout(h, nullptr, N, seq, true).words * 4; }

// Lever 6 as far as the configuration and the options decide it (what is left to the forward: ForwardMode::table_lo, which a
// caller's table needs anyway): zett_finalize built the operands (16-bit mode, >= 2 layers, no language position) and the rule holds.
static bool id_qkv_configured(const zett_hypernet* h) {
    return h->id_qkv && h->m.id_u.w && (h->id_qkv == 2 || h->cfg.hidden >= ID_QKV_MIN_HIDDEN);
}

// The plan of one forward into slot s, on stream st: six small kernels, three scans, and the copy of the row offsets and the
// three counters to pinned memory; s.done is recorded behind them.
static int enqueue_plan(zett_hypernet* h, zett_hypernet::PlanSlot& s, const int32_t* sfm, int64_t N, int seq, hipStream_t st) {
    const zett_config& c = h->cfg;
    const int lam = c.embed_lang ? 1 : 0;
    const int V = c.original_vocab_size + c.n_extra;
    const int64_t max_tok = N * (int64_t)(seq + lam);
    if (int rc = s.i32.reserve(plan_i32_bytes(h, N, seq))) return rc;
    if (int rc = s.u8.reserve((size_t)N + (size_t)max_tok)) return rc;
    const size_t need_ints = (size_t)N + 1 + 3;
    if (s.host_ints < need_ints) {
        if (s.host) (void)hipHostFree(s.host);
        s.host = nullptr;
        HIP_TRY(hipHostMalloc((void**)&s.host, need_ints * 4, hipHostMallocDefault));
        s.host_ints = need_ints;
    }
    if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming));
    if (!s.released) HIP_TRY(hipEventCreateWithFlags(&s.released, hipEventDisableTiming));
    const PlanLayout L = plan_layout(h, &s, N, seq);
    const PlanArrays& p = L.p;
    HIP_TRY(hipMemsetAsync(s.i32.p, 0, L.n_clear * 4, st));          // id_flag, pair_flag, err: one piece of the arena
    const int rb = (int)((N + 255) / 256);
    hipLaunchKernelGGL(plan_rows_kernel, dim3(rb), dim3(256), 0, st, sfm, N, seq, c.pad_token_id, lam, V, p);
    launch_exclusive_scan(p.row_count, p.row_offset, N, L.scan_tmp, st);
    launch_exclusive_scan(p.id_flag, p.id_slot, (int64_t)V, L.scan_tmp, st);
    {
        // (ABI 8) a forward on a caller-provided table: a token's table slot is its id's slot in the GLOBAL distinct-id list
        PlanArrays pt = p;
        // (lever 6 gathers the call's rows of that table into the handle's own table first and keeps the plan's own slots)
        if (h->ext.id_slot && !id_qkv_configured(h)) pt.id_slot = const_cast<int32_t*>(h->ext.id_slot);
        hipLaunchKernelGGL(plan_tokens_kernel, dim3(rb), dim3(256), 0, st, sfm, N, seq, c.pad_token_id, lam, V, pt);
    }
    if (L.pair_plan) {
        launch_exclusive_scan(p.pair_flag, p.pair_slot, L.PK, L.scan_tmp, st);
        hipLaunchKernelGGL(plan_pairs_kernel, dim3((unsigned)((max_tok + 255) / 256)), dim3(256), 0, st, N, p);
    }
    hipLaunchKernelGGL(plan_idlist_kernel, dim3((V + 255) / 256), dim3(256), 0, st, V, p);
    HIP_TRY(hipGetLastError());
    // the row offsets and, right behind them, the three counters (distinct ids, error word, distinct pairs) to the host: one copy
    HIP_TRY(hipMemcpyAsync(s.host, p.row_offset, ((size_t)N + 1 + 3) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(s.done, st));
    s.sfm = sfm; s.n_rows = N; s.seq = seq; s.pair_plan = L.pair_plan; s.ext_id_slot = h->ext.id_slot; s.local_slots = id_qkv_configured(h);
    return 0;
}

template <typename T>
int do_forward(zett_hypernet* h, const int32_t* sfm, int64_t N, int seq, const void* src, int src_dtype, const zett_dest* dest,
               int lang_index, float* out_in, float* out_out, float* out_bias, hipStream_t st);
template <typename T>
int do_table_rows(zett_hypernet* h, const int32_t* id_list, int first, int count, const void* src, int src_dtype, void* table_out, float* stats_out, hipStream_t st);

// What the entry points of the forward family (zett_forward[_into], zett_forward_table[_into], zett_forward_prepare, zett_table_plan,
// zett_table_rows) check before they touch the device, in the one order in which they report it.  An entry point fills in what it
// has; the fields say where the entry points differ.  Returns 0, an error code, or CALL_EMPTY: a valid call on no rows.
constexpr int CALL_EMPTY = 1;
struct CallCheck {
    int64_t n_rows = 0; int32_t seq = 1;
    bool shape = true;                  // [n_rows, seq] surface forms (zett_table_rows has a table range of its own instead)
    bool empty_ok = false;              // n_rows == 0 is a call that does nothing, not a bad shape
    bool null_arg = false, null_first = false;      // a required pointer is null; reported before the shape (zett_table_plan)
    const char* null_text = "null tensor argument";
    bool encoder = false, need_out_out = false; int32_t lang_index = 0;      // the call runs the encoder: positions, outputs, language
    bool source = false; int src_dtype = ZETT_F32; int64_t v_src = 0;        // the call reads source embeddings
    const char* table_mode = nullptr;   // the entry point's name when it needs the folded table, i.e. a 16-bit precision
};
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

}  // namespace

// ---------------------------------------------------------------------------------
extern "C" {

const char* zett_last_error(void) { return g_err.c_str(); }
int zett_abi_version(void) { return ZETT_ABI_VERSION; }

int zett_create(const zett_config* cfg, int device, int precision, zett_hypernet** out) {
    if (!cfg || !out) return fail(ZETT_E_INVALID, "null argument");
    if (precision != ZETT_PREC_BF16 && precision != ZETT_PREC_F32 && precision != ZETT_PREC_F16) return fail(ZETT_E_INVALID, "unknown precision %d", precision);
    if (int rc = validate_config(*cfg, precision)) return rc;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(ZETT_E_INVALID, "device %d out of range (%d visible)", device, ndev);
    ZETT_ON_DEVICE(device);
    auto* h = new zett_hypernet();
    h->cfg = *cfg;
    h->device = device;
    h->precision = precision;
    h->decl = declare_weights(h->cfg, h->m);
    if (hipMalloc((void**)&h->range_word, 64) != hipSuccess || hipHostMalloc((void**)&h->range_host, 64, hipHostMallocDefault) != hipSuccess ||
        hipMemset(h->range_word, 0, 64) != hipSuccess) {
        if (h->range_word) (void)hipFree(h->range_word);
        if (h->range_host) (void)hipHostFree(h->range_host);
        delete h;
        return fail(ZETT_E_HIP, "allocation of the range word failed");
    }
    *out = h;
    return 0;
}

int zett_destroy(zett_hypernet* h) {
    if (!h) return 0;
    ::zett::DeviceScope _scope(h->device);
    for (auto& kv : h->w) {
        if (kv.second.f32) (void)hipFree(kv.second.f32);
        if (kv.second.lo && kv.second.lo != (void*)kv.second.f32) (void)hipFree(kv.second.lo);
    }
    for (void* p : h->owned) (void)hipFree(p);
    for (DevBuf* b : {&h->table, &h->x0, &h->yf, &h->yt, &h->big, &h->pre, &h->ctx, &h->cf, &h->ct, &h->lnstats, &h->lnparts, &h->dest_word, &h->dest_stage[0], &h->dest_stage[1], &h->dest_sink, &h->single_map})
        b->release();
    if (h->single_host) (void)hipHostFree(h->single_host);
    if (h->single_copied) (void)hipEventDestroy(h->single_copied);
    for (zett_hypernet::PlanSlot* psp : {&h->plan[0], &h->plan[1], &h->table_plan}) {
        zett_hypernet::PlanSlot& ps = *psp;
        ps.i32.release(); ps.u8.release();
        if (ps.host) (void)hipHostFree(ps.host);
        if (ps.done) (void)hipEventDestroy(ps.done);
        if (ps.released) (void)hipEventDestroy(ps.released);
    }
    if (h->plan_stream) (void)hipStreamDestroy(h->plan_stream);
    if (h->plan_fork) (void)hipEventDestroy(h->plan_fork);
    if (h->range_word) (void)hipFree(h->range_word);
    if (h->range_host) (void)hipHostFree(h->range_host);
    if (h->dest_host) (void)hipHostFree(h->dest_host);
    if (h->dest_checked) (void)hipEventDestroy(h->dest_checked);
    for (hipEvent_t e : h->out_ready) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->lane_ev) if (e) (void)hipEventDestroy(e);
    if (h->lane_stream) (void)hipStreamDestroy(h->lane_stream);
    for (hipEvent_t e : h->ev) (void)hipEventDestroy(e);
    delete h;
    return 0;
}

int zett_load_weight(zett_hypernet* h, const char* name, const void* data, int dtype, const int64_t* shape, int ndim) {
    if (!h || !name || !data || !shape || ndim < 1) return fail(ZETT_E_INVALID, "null argument");
    if (h->finalized) return fail(ZETT_E_STATE, "weights are frozen after zett_finalize");
    const std::string n(name);
    auto it = std::lower_bound(h->decl.begin(), h->decl.end(), n, [](const WeightDecl& d, const std::string& key) { return d.name < key; });
    if (it == h->decl.end() || it->name != n) return 0;   // e.g. model.embeddings.word_embeddings.weight: never read
    std::vector<int64_t> got(shape, shape + ndim);
    if (got != it->shape) {
        std::string a, b;
        for (auto v : got) a += std::to_string(v) + ",";
        for (auto v : it->shape) b += std::to_string(v) + ",";
        return fail(ZETT_E_INVALID, "%s: shape [%s] does not match the config's [%s]", name, a.c_str(), b.c_str());
    }
    ZETT_ON_DEVICE(h->device);
    size_t numel = 1;
    for (auto v : got) numel *= (size_t)v;
    Tensor& t = h->w[n];
    if (t.f32) { (void)hipFree(t.f32); t.f32 = nullptr; }
    t.shape = got;
    t.numel = numel;
    HIP_TRY(hipMalloc((void**)&t.f32, numel * 4));
    if (dtype == ZETT_F32) {
        HIP_TRY(hipMemcpy(t.f32, data, numel * 4, hipMemcpyDefault));
    } else if (dtype == ZETT_F16 || dtype == ZETT_BF16) {
        void* stage = nullptr;
        HIP_TRY(hipMalloc(&stage, numel * 2));
        hipError_t e = hipMemcpy(stage, data, numel * 2, hipMemcpyDefault);
        if (e == hipSuccess) {
            const int blocks = (int)std::min<size_t>((numel + 255) / 256, 65535);
            if (dtype == ZETT_F16) hipLaunchKernelGGL(convert_to_f32_kernel<1>, dim3(blocks), dim3(256), 0, 0, stage, t.f32, numel);
            else hipLaunchKernelGGL(convert_to_f32_kernel<2>, dim3(blocks), dim3(256), 0, 0, stage, t.f32, numel);
            e = hipDeviceSynchronize();
        }
        (void)hipFree(stage);
        if (e != hipSuccess) return fail(ZETT_E_HIP, "upload of %s failed: %s", name, hipGetErrorString(e));
    } else {
        return fail(ZETT_E_INVALID, "unknown dtype %d", dtype);
    }
    return 0;
}

int zett_finalize(zett_hypernet* h) {
    if (!h) return fail(ZETT_E_INVALID, "null handle");
    if (h->finalized) return 0;
    ZETT_ON_DEVICE(h->device);
    std::vector<Tensor*> ts;          // the uploaded tensor of every declared weight, in the declaration's order
    for (const WeightDecl& d : h->decl) {
        auto it = h->w.find(d.name);
        if (it == h->w.end()) return fail(ZETT_E_STATE, "missing weight: %s", d.name.c_str());
        ts.push_back(&it->second);
    }
    const zett_config& c = h->cfg;
    Model& m = h->m;
    const size_t es = elt_size(h->precision);
    // GEMM operands in the arithmetic type
    for (size_t i = 0; i < ts.size(); ++i) {
        Tensor& t = *ts[i];
        if (!h->decl[i].operand) continue;
        if (h->precision == ZETT_PREC_F32) { t.lo = t.f32; continue; }
        HIP_TRY(hipMalloc(&t.lo, t.numel * 2));
        const int blocks = (int)std::min<size_t>((t.numel / 4 + 255) / 256 + 1, 65535);
        with_precision(h->precision, [&](auto a) {
            using T = typename decltype(a)::type;
            if constexpr (sizeof(T) == 2)       // (the fp32 mode left the loop above: no fp32 instantiation of the kernel exists)
                hipLaunchKernelGGL(convert_f32_to_lo_kernel<T>, dim3(blocks), dim3(256), 0, 0, t.f32, (T*)t.lo, t.numel, h->range_word);
        });
    }
    HIP_TRY(hipDeviceSynchronize());
    // bind the model: a GEMM operand's copy in the arithmetic type, the fp32 tensor of everything else — the tensors as they are
    // NOW, whatever order they were uploaded in and however often
    for (size_t i = 0; i < ts.size(); ++i)
        if (h->decl[i].operand) *h->decl[i].operand = ts[i]->lo;
        else *h->decl[i].vec = ts[i]->f32;
    auto original = [&](const Linear& l) -> const float* {      // the fp32 original of an operand (until it is freed below)
        for (size_t i = 0; i < ts.size(); ++i)
            if (h->decl[i].operand == &l.w) return ts[i]->f32;
        return nullptr;
    };
    // fused QKV operand per layer: rows [q | k | v]
    const size_t H = c.hidden;
    for (Layer& L : m.layers) {
        void* wq = nullptr; float* bq = nullptr;
        HIP_TRY(hipMalloc(&wq, 3 * H * H * es));
        HIP_TRY(hipMalloc((void**)&bq, 3 * H * 4));
        h->owned.push_back(wq); h->owned.push_back(bq);
        int k = 0;
        for (const Linear* part : {&L.q, &L.k, &L.v}) {
            HIP_TRY(hipMemcpy((char*)wq + (size_t)k * H * H * es, part->w, H * H * es, hipMemcpyDeviceToDevice));
            HIP_TRY(hipMemcpy(bq + (size_t)k * H, part->b, H * 4, hipMemcpyDeviceToDevice));
            ++k;
        }
        L.qkv = Linear{wq, bq};
    }
    // LayerNorm fold operands (rowops.hip.h fold_weight_kernel); needs the fp32 originals, which are freed below
    if (h->precision != ZETT_PREC_F32 && c.hidden % 128 == 0) {
        auto fold = [&](const float* w32, size_t N, size_t K, const Affine& ln, const float* bias, Folded& f) -> int {
            HIP_TRY(hipMalloc(&f.w, N * K * es));
            HIP_TRY(hipMalloc((void**)&f.c, N * 4));
            HIP_TRY(hipMalloc((void**)&f.b, N * 4));
            h->owned.push_back(f.w); h->owned.push_back(f.c); h->owned.push_back(f.b);
            with_precision(h->precision, [&](auto a) {
                using T = typename decltype(a)::type;
                if constexpr (sizeof(T) == 2)
                    launch_fold_weight<T>(0, w32, (int)N, (int)K, ln.w, ln.b, bias, (T*)f.w, f.c, f.b, h->range_word);
            });
            return 0;
        };
        float* tmp = nullptr;                       // fp32 [3H, H] fused QKV of one layer
        HIP_TRY(hipMalloc((void**)&tmp, 3 * H * H * 4));
        for (int l = 0; l < c.layers; ++l) {
            Layer& L = m.layers[l];
            if (int rc = fold(original(L.up), c.intermediate, H, L.attn_ln, L.up.b, L.fold_up)) return rc;
            // lever 6 is possible for this configuration (what the options add: forward_mode's table_lo)
            const bool id_qkv = l == 0 && c.layers >= 2 && !c.embed_lang && H * sizeof(float) <= 64 * 1024;
            if (l == 0 && !id_qkv) continue;
            int k = 0;
            for (const Linear* part : {&L.q, &L.k, &L.v}) {
                HIP_TRY(hipMemcpy(tmp + (size_t)k * H * H, original(*part), H * H * 4, hipMemcpyDeviceToDevice));
                ++k;
            }
            if (l > 0) {
                if (int rc = fold(tmp, 3 * H, H, m.layers[l - 1].out_ln, L.qkv.b, L.fold_qkv)) return rc;
                continue;
            }
            // gamma_t (.) gamma and beta_t (.) gamma (fp32 products, made on the host), no bias: the fold of layer 0's qkv onto raw table rows
            std::vector<float> gt(H), bt(H), ge(H), g2(H), b2(H);
            HIP_TRY(hipMemcpy(gt.data(), m.in_block.ln.w, H * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(bt.data(), m.in_block.ln.b, H * 4, hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(ge.data(), m.emb_ln.w, H * 4, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < H; ++i) { g2[i] = gt[i] * ge[i]; b2[i] = bt[i] * ge[i]; }
            float* aux = nullptr;                   // [H] gamma'', [H] beta'', [3H] zero bias
            HIP_TRY(hipMalloc((void**)&aux, 5 * H * 4));
            HIP_TRY(hipMemset(aux, 0, 5 * H * 4));
            HIP_TRY(hipMemcpy(aux, g2.data(), H * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(aux + H, b2.data(), H * 4, hipMemcpyHostToDevice));
            const Affine ln2{aux, aux + H};
            if (int rc = fold(tmp, 3 * H, H, ln2, aux + 2 * H, m.id_u)) return rc;
            HIP_TRY(hipMalloc((void**)&m.id_cpos, (size_t)c.max_positions * 3 * H * 4));
            HIP_TRY(hipMalloc((void**)&m.id_cw, 3 * H * 4));
            HIP_TRY(hipMalloc((void**)&m.id_bq, 3 * H * 4));
            h->owned.push_back(m.id_cpos); h->owned.push_back(m.id_cw); h->owned.push_back(m.id_bq);
            launch_pos_qkv(0, tmp, (int)(3 * H), (int)H, m.emb_ln.w, m.emb_ln.b, L.qkv.b, m.token_type, m.position, c.max_positions, m.id_cpos, m.id_cw, m.id_bq);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipDeviceSynchronize());
            (void)hipFree(aux);
        }
        // the output heads: Linear(LN_1e-6(.)) with the ProjectorBlock's LayerNorm folded in (not for the split single head,
        // whose two-destination epilogue is the generic one)
        if (!(c.single_head && c.separate_out)) {
            const size_t w0 = c.single_head ? c.n_in_embd : c.n_embd;      // (= n_embd: a single head is not split here)
            for (Head* hd : {&m.head_in, &m.head_out})
                if (hd->out.w)
                    if (int rc = fold(original(hd->out), w0, H, hd->block.ln, hd->out.b, hd->fold)) return rc;
            std::vector<float> ones(w0, 1.0f), zeros(w0, 0.0f);
            HIP_TRY(hipMalloc((void**)&m.head_one, w0 * 4));
            HIP_TRY(hipMalloc((void**)&m.head_zero, w0 * 4));
            h->owned.push_back(m.head_one); h->owned.push_back(m.head_zero);
            HIP_TRY(hipMemcpy(m.head_one, ones.data(), w0 * 4, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(m.head_zero, zeros.data(), w0 * 4, hipMemcpyHostToDevice));
        }
        HIP_TRY(hipDeviceSynchronize());
        (void)hipFree(tmp);
    }
    // range guard: a weight (or gamma-folded weight) that does not fit the operand type is an error here, not an inf later
    HIP_TRY(hipMemcpy(h->range_host, h->range_word, 4, hipMemcpyDeviceToHost));
    if (h->range_host[0] & ZETT_RANGE_WEIGHT)
        return fail(ZETT_E_RANGE, "a GEMM weight (or a LayerNorm-folded weight W*gamma) exceeds the half range (|w| > 65504 or not finite): "
                                  "this checkpoint needs ZETT_PREC_BF16 or ZETT_PREC_F32");
    // output Rescaler vectors laid out over the first head's columns
    if (c.rescale) {
        const size_t w0 = c.single_head ? c.n_in_embd : c.n_embd;
        float* scale = nullptr; float* shift = nullptr;
        HIP_TRY(hipMalloc((void**)&scale, w0 * 4));
        HIP_TRY(hipMalloc((void**)&shift, w0 * 4));
        h->owned.push_back(scale); h->owned.push_back(shift);
        HIP_TRY(hipMemcpy(scale, m.scaler.w, c.n_embd * 4, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(shift, m.scaler.b, c.n_embd * 4, hipMemcpyDeviceToDevice));
        if (c.single_head && c.separate_out) {
            HIP_TRY(hipMemcpy(scale + c.n_embd, m.out_scaler.w, c.n_embd * 4, hipMemcpyDeviceToDevice));
            HIP_TRY(hipMemcpy(shift + c.n_embd, m.out_scaler.b, c.n_embd * 4, hipMemcpyDeviceToDevice));
        }
        m.head_in.scale = scale; m.head_in.shift = shift;
        m.head_out.scale = m.out_scaler.w; m.head_out.shift = m.out_scaler.b;
    }
    // the fp32 originals of 16-bit GEMM operands are no longer needed
    if (h->precision != ZETT_PREC_F32)
        for (size_t i = 0; i < ts.size(); ++i)
            if (h->decl[i].operand && ts[i]->f32) { (void)hipFree(ts[i]->f32); ts[i]->f32 = nullptr; }
    h->finalized = true;
    return 0;
}

int zett_set_option(zett_hypernet* h, const char* key, int64_t value) {
    if (!h || !key) return fail(ZETT_E_INVALID, "null argument");
    const std::string k(key);
    if (k == "max_chunk_tokens") {
        if (value < 1024) return fail(ZETT_E_INVALID, "max_chunk_tokens must be >= 1024");
        h->max_chunk_tokens = value;
    } else if (k == "time_gemm") {
        h->time_gemm = value != 0;
    } else if (k == "cls_only_last_layer") {
        h->cls_only_last = value != 0;
    } else if (k == "pair_dedupe") {
        h->pair_dedupe = value != 0;
    } else if (k == "residual_lo") {
        if (value < 0 || value > 2) return fail(ZETT_E_INVALID, "residual_lo must be 0 (fp32 residual stream), 1 (16-bit stream in f16 mode) or 2 (in bf16 mode too)");
        h->residual_lo = (int)value;
    } else if (k == "concurrent_lanes") {
        if (value < 0 || value > 2) return fail(ZETT_E_INVALID, "concurrent_lanes must be 0 (never), 1 (auto) or 2 (whenever a call is one chunk of >= 512 rows)");
        h->concurrent_lanes = (int)value;
    } else if (k == "attention_fast") {
        h->attention_fast = value != 0;
    } else if (k == "ln_fold") {
        if (value < 0 || value > 2) return fail(ZETT_E_INVALID, "ln_fold must be 0 (off), 1 (encoder and output heads) or 2 (encoder only: A/B)");
        h->ln_fold = (int)value;
    } else if (k == "gemm_tail_split") {
        if (value < 0 || value > 3) return fail(ZETT_E_INVALID, "gemm_tail_split must be 0 (never), 1 (auto), 2 (cut every gemm4d launch in the middle) or 3 (128x256 tiles only)");
        h->gemm_tail_split = (int)value;
    } else if (k == "attention_pack") {
        h->attention_pack = value != 0;
    } else if (k == "ln_rows8") {
        h->ln_rows8 = value != 0;
    } else if (k == "table_lo") {
        h->table_lo = value != 0;
    } else if (k == "gemm_group") {
        if (value < 0 || value > 64) return fail(ZETT_E_INVALID, "gemm_group must be 0 (default: 4) .. 64");
        h->gemm_group = (int)value;
    } else if (k == "gemm_tile_order") {
        if (value < 0 || value > 1) return fail(ZETT_E_INVALID, "gemm_tile_order must be 0 or 1");
        h->gemm_tile_order = (int)value;
    } else if (k == "gemm4d_min_k") {
        if (value < 64) return fail(ZETT_E_INVALID, "gemm4d_min_k must be >= 64");
        h->gemm4d_min_k = (int)value;
    } else if (k == "range_accumulate") {
        h->range_accumulate = value != 0;
    } else if (k == "single_rows") {
        if (value < 0 || value > 2) return fail(ZETT_E_INVALID, "single_rows must be 0 (off), 1 (auto) or 2 (whenever a call is one chunk on one lane)");
        h->single_rows = (int)value;
    } else if (k == "id_qkv") {
        if (value < 0 || value > 2) return fail(ZETT_E_INVALID, "id_qkv must be 0 (off), 1 (when possible and hidden >= 4096) or 2 (whenever possible)");
        h->id_qkv = (int)value;
    } else if (k == "gemm_variant") {
        if (value != 0 && value != 1 && value != 2 && value != 3 && value != 7 && value != 8)
            return fail(ZETT_E_INVALID, "gemm_variant must be 0 (auto), 1 (128x128), 2 (256x256 register-staged), 3 (384x256), 7 (256x256 four-wave direct-to-LDS) or 8 (7 with the generic epilogue drain)");
        h->gemm_variant = (int)value;
    } else {
        return fail(ZETT_E_INVALID, "unknown option %s", key);
    }
    return 0;
}

int zett_workspace_bytes(const zett_hypernet* h, int64_t n_rows, int32_t seq, int64_t* out_bytes) {
    if (!h || !out_bytes) return fail(ZETT_E_INVALID, "null argument");
    if (n_rows < 0 || seq < 1) return fail(ZETT_E_INVALID, "bad surface-form shape [%lld, %d]", (long long)n_rows, seq);
    const zett_config& c = h->cfg;
    const int64_t V = (int64_t)c.original_vocab_size + c.n_extra;
    const int64_t max_tok = n_rows * (int64_t)(seq + (c.embed_lang ? 1 : 0));
    // worst case of the plan: no pad position, every position a different source id
    const WorkspaceSizes w = workspace_sizes(c, elt_size(h->precision), seq, max_tok, std::min<int64_t>(V, max_tok), h->max_chunk_tokens);
    *out_bytes = (int64_t)(w.total() + plan_i32_bytes(h, n_rows, seq) + (size_t)n_rows + (size_t)max_tok);
    return 0;
}

int zett_get_stats(const zett_hypernet* h, zett_stats* out) {
    if (!h || !out) return fail(ZETT_E_INVALID, "null argument");
    *out = h->stats;
    return 0;
}

int zett_single_rows(const zett_hypernet* h, int64_t* out) {
    if (!h || !out) return fail(ZETT_E_INVALID, "null argument");
    *out = h->single_rows_last;
    return 0;
}

int zett_id_qkv(const zett_hypernet* h, int64_t* out) {
    if (!h || !out) return fail(ZETT_E_INVALID, "null argument");
    *out = h->id_qkv_last;
    return 0;
}

int zett_stream_wait_output(zett_hypernet* h, int which, void* stream) {
    if (!h) return fail(ZETT_E_INVALID, "null handle");
    if (which != ZETT_OUT_IN && which != ZETT_OUT_BIAS) return fail(ZETT_E_INVALID, "which must be ZETT_OUT_IN or ZETT_OUT_BIAS");
    if (!h->out_recorded) return fail(ZETT_E_STATE, "no forward has run on this handle");
    ZETT_ON_DEVICE(h->device);
    HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, h->out_ready[which], 0));
    return 0;
}

int zett_get_gemm_log(const zett_hypernet* h, zett_gemm_record* out, int64_t capacity, int64_t* count) {
    if (!h || !count || capacity < 0 || (capacity > 0 && !out)) return fail(ZETT_E_INVALID, "null argument");
    *count = (int64_t)h->gemm_log.size();
    for (int64_t i = 0; i < capacity && i < *count; ++i) out[i] = h->gemm_log[(size_t)i];
    return 0;
}

int zett_check_range(zett_hypernet* h, void* stream, int32_t* flags) {
    if (!h) return fail(ZETT_E_INVALID, "null handle");
    ZETT_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(h->range_host, h->range_word, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int32_t w = h->range_host[0];
    if (h->range_accumulate && w) HIP_TRY(hipMemsetAsync(h->range_word, 0, 4, st));
    if (flags) *flags = w;
    if (!w) return 0;
    return fail(ZETT_E_RANGE, "the last forward left the range of its arithmetic:%s%s%s%s (precision %s)",
                (w & ZETT_RANGE_SOURCE) ? " in_scaler(source_embeddings) beyond the half range;" : "",
                (w & ZETT_RANGE_ACTIVATION) ? " a 16-bit activation (Q/K/V, FFN intermediate or the operand copy of the residual sum) beyond the half range;" : "",
                (w & ZETT_RANGE_OUTPUT) ? " non-finite predicted embeddings;" : "",
                (w & ZETT_RANGE_DEST) ? " a finite value beyond the range of an f16 destination (stored as inf);" : "",
                h->precision == ZETT_PREC_F16 ? "f16: re-run with ZETT_PREC_BF16" : h->precision == ZETT_PREC_BF16 ? "bf16" : "f32");
}

int zett_forward_prepare(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq, void* input_stream) {
    CallCheck k;
    k.n_rows = n_rows; k.seq = seq; k.empty_ok = true; k.null_arg = !surface_forms;
    if (int rc = check_call(h, k)) return rc == CALL_EMPTY ? 0 : rc;
    ZETT_ON_DEVICE(h->device);
    if (!h->plan_stream) {      // highest priority: the plan's small workgroups must get CUs while a forward's GEMM tiles own the chip
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&h->plan_stream, hipStreamNonBlocking, greatest));
    }
    if (!h->plan_fork) HIP_TRY(hipEventCreateWithFlags(&h->plan_fork, hipEventDisableTiming));
    zett_hypernet::PlanSlot& ps = h->plan[h->plan_cur ^ 1];
    if (ps.pending) HIP_TRY(hipEventSynchronize(ps.done));           // replaces a prepared plan nobody took
    // behind the surface forms (whatever input_stream holds now) and behind the forward that last read this slot
    HIP_TRY(hipEventRecord(h->plan_fork, (hipStream_t)input_stream));
    HIP_TRY(hipStreamWaitEvent(h->plan_stream, h->plan_fork, 0));
    if (ps.released) HIP_TRY(hipStreamWaitEvent(h->plan_stream, ps.released, 0));
    if (int rc = enqueue_plan(h, ps, surface_forms, n_rows, seq, h->plan_stream)) return rc;
    ps.pending = true;
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
        if (!h->range_accumulate) HIP_TRY(hipMemsetAsync(h->range_word, 0, 4, st));
        for (hipEvent_t& e : h->out_ready) {
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(e, st));
        }
        h->out_recorded = true;
        return 0;
    }
    return with_precision(h->precision, [&](auto a) {
        return do_forward<typename decltype(a)::type>(h, surface_forms, n_rows, seq, source_embeddings, src_dtype, dest, lang_index, out_in, out_out, out_bias, st);
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
int zett_table_plan(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq, int32_t* id_slot_out, int32_t* id_list_out,
                    int64_t* n_ids_out, void* stream) {
    CallCheck k;
    k.n_rows = n_rows; k.seq = seq;
    k.null_arg = !surface_forms || !id_slot_out || !id_list_out || !n_ids_out; k.null_text = "null argument"; k.null_first = true;
    if (int rc = check_call(h, k)) return rc;
    const zett_config& c = h->cfg;
    const int V = c.original_vocab_size + c.n_extra;
    ZETT_ON_DEVICE(h->device);
    hipStream_t st = (hipStream_t)stream;
    zett_hypernet::PlanSlot& ps = h->table_plan;
    const zett_hypernet::ExtTable saved = h->ext;
    h->ext = zett_hypernet::ExtTable{};          // (this plan numbers the ids itself)
    const int rc = enqueue_plan(h, ps, surface_forms, n_rows, seq, st);
    h->ext = saved;
    if (rc) return rc;
    HIP_TRY(hipEventSynchronize(ps.done));
    const int32_t* hoff = ps.host;
    if (hoff[n_rows + 2] != 0)
        return fail(ZETT_E_INDEX, "surface-form row %d holds an id outside [0, %d) (original_vocab_size %d + %d fallback rows)",
                    hoff[n_rows + 2] - 1, V, c.original_vocab_size, c.n_extra);
    const int D = hoff[n_rows + 1];
    const PlanLayout L = plan_layout(h, &ps, n_rows, seq);
    HIP_TRY(hipMemcpyAsync(id_slot_out, L.p.id_slot, ((size_t)V + 1) * 4, hipMemcpyDeviceToDevice, st));
    if (D > 0) HIP_TRY(hipMemcpyAsync(id_list_out, L.p.id_list, (size_t)D * 4, hipMemcpyDeviceToDevice, st));
    *n_ids_out = D;
    return 0;
}

int zett_table_rows(zett_hypernet* h, const int32_t* id_list, int64_t first, int64_t count, const void* source_embeddings, int src_dtype,
                    int64_t v_src, void* table_out, float* stats_out, void* stream) {
    CallCheck k;
    k.shape = false;                    // (a range of table rows instead of surface forms: checked here, between the handle and the tensors)
    if (int rc = check_call(h, k)) return rc;
    if (first < 0 || count < 0 || first + count >= (int64_t)0x7fffffff) return fail(ZETT_E_INVALID, "bad table range [%lld, +%lld)", (long long)first, (long long)count);
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
    h->ext.table = table; h->ext.stats = table_stats; h->ext.id_slot = id_slot;
    const int rc = with_precision(h->precision, [&](auto a) {
        return do_forward<typename decltype(a)::type>(h, surface_forms, n_rows, seq, nullptr, ZETT_F32, dest, lang_index, out_in, out_out, out_bias, st);
    });
    h->ext = zett_hypernet::ExtTable{};
    return rc;
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
        e.range_flag = h->range_word;
        return e;
    }

    long a_rows_readable = 0;   // rows every A operand buffer can be read for (workspace slack)
    bool staged_dst = false;    // (zett_forward_into) the launch in flight writes the staged fp32 rows of a destination (gemm log bit 11)
    int stage_lane = 0;         // (zett_forward_into) which staging buffer head_gemm uses: the lane's own (h->dest_stage[lane])

    // the handle's options that decide a launch (gemm_launch.hip.h)
    GemmOptions gemm_options() const {
        GemmOptions o;
        o.gemm_variant = h->gemm_variant; o.gemm4d_min_k = h->gemm4d_min_k; o.gemm_tail_split = h->gemm_tail_split;
        o.gemm_tile_order = h->gemm_tile_order; o.gemm_group = h->gemm_group;
        return o;
    }
    // the tile variant a launch takes: gemm_variant_for (gemm_launch.hip.h), the rule zett_op_fwd_gemm shares
    int variant_for(int M, int N, int K, const GemmEpilogue<T>& e) const { return gemm_variant_for<T>(gemm_options(), a_rows_readable, M, N, K, e); }

    void gemm(const T* A, int lda, const T* Wp, int ldw, int M, int N, int K, const GemmEpilogue<T>& e) {
        if (rc || M <= 0) return;
        GemmArgs<T> g{A, lda, Wp, ldw, M, N, K, e};
        g.tile_order = h->gemm_tile_order;
        g.group = h->gemm_group;
        g.row0 = gemm_row0_for(h->gemm_tail_split, M);
        const double fl = 2.0 * (double)M * (double)N * (double)K;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (h->time_gemm) {
            while (h->ev.size() < h->ev_used + 2) {
                hipEvent_t ev;
                if (hipEventCreate(&ev) != hipSuccess) { rc = fail(ZETT_E_HIP, "hipEventCreate failed"); return; }
                h->ev.push_back(ev);
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
        if (h->time_gemm) (void)hipEventRecord(e1, st);
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
            if (vec) hipLaunchKernelGGL((dest_store_rows_kernel<OT, true>), grid, dim3(256), 0, st, S, ld_s, (OT*)d.p, d.ld, d.rows, (int64_t)rows, cols, h->range_word);
            else hipLaunchKernelGGL((dest_store_rows_kernel<OT, false>), grid, dim3(256), 0, st, S, ld_s, (OT*)d.p, d.ld, d.rows, (int64_t)rows, cols, h->range_word);
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
        launch_layernorm<T, EMBED, READOUT, BT>(st, H, h->ln_rows8, in, H, rows, gamma, beta, eps, of, ol, stats, sum, embed, t0, readout);
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
    m.fold = h->ln_fold && !std::is_same<T, float>::value && h->gemm_variant == 0 && c.hidden % 128 == 0 && c.hidden >= 512 && h->m.layers.back().fold_up.w != nullptr;
    m.lo_stream = m.fold && c.layers >= 1 && sizeof(T) == 2 && (h->residual_lo == 2 || (h->residual_lo == 1 && std::is_same<T, f16_t>::value));
    m.table_lo = m.lo_stream && h->table_lo != 0;
    m.fold_heads = m.fold && h->ln_fold == 1 && h->m.head_in.fold.w != nullptr;
    return m;
}
int needs_folded_table(const char* entry) {
    return fail(ZETT_E_INVALID, "%s needs the folded 16-bit table: f16 arithmetic with the LayerNorm fold, the 16-bit residual stream and table_lo on", entry);
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
            launch_gather_src<T, decltype(sd)::value>(R.st, id_list, s0, m, src, c.n_in_embd, c.original_vocab_size, md.fallback, md.in_scaler.w, md.in_scaler.b, w.X0, h->range_word);
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
    const WorkspaceSizes ws = workspace_sizes(h->cfg, sizeof(T), 1, count, count, h->max_chunk_tokens);
    const size_t MCS = (size_t)ws.chunk_tokens + 768;
    if (int rc = reserve_workspace(h, ws, mode.fold, false)) return rc;
    Runner<T> R{h, st};
    R.a_rows_readable = (long)MCS;
    // (per-launch events and the launch log belong to a forward: zett_forward resets both when it starts)
    struct NoTiming { zett_hypernet* h; int saved; ~NoTiming() { h->time_gemm = saved; } } no_timing{h, h->time_gemm};
    h->time_gemm = 0;
    table_phase<T>(R, lane_workspace<T>(h, 0, MCS), id_list, first, count, src, src_dtype, ws.chunk_tokens, true, (T*)table_out, stats_out, nullptr);
    return R.rc;
}

// From the moment a forward has taken its plan slot, kernels that read the slot (and the pinned host words) may be enqueued: whatever
// way the forward is left — a failed launch, a failed workspace reservation, a lane that fails after the other one was launched — the
// second lane is joined to `st` and ps.released is recorded behind everything, so that a later zett_forward_prepare / zett_forward
// never rewrites the plan under kernels still in flight.
struct SlotGuard {
    zett_hypernet* h; zett_hypernet::PlanSlot* ps; hipStream_t st; bool lane_forked = false;
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
    // the call
    zett_hypernet* h; const int32_t* sfm; int64_t N; int seq; const void* src; int src_dtype; const zett_dest* dest; int lang_index;
    float* out_in; float* out_out; float* out_bias; hipStream_t st;
    // what the stages find
    Runner<T> R{h, st};
    const zett_config& c = h->cfg;
    const Model& md = h->m;
    const int H = c.hidden, I = c.intermediate, E = c.n_embd;
    const ForwardMode mode = forward_mode<T>(h);
    zett_hypernet::PlanSlot* ps = nullptr;
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
        if (int rc = take_plan()) return rc;
        SlotGuard guard{h, ps, st};
        if (int rc = read_plan()) return rc;
        if (int rc = reserve()) return rc;
        // ---- table: input_projection once per distinct source id (A2-A4) -----------------
        if (!h->ext.table)
            table_phase<T>(R, lane_workspace<T>(h, 0, MCS), p.id_list, 0, D, src, src_dtype, MC, mode.table_lo, TBL16, TBLST, TBL);
        id_qkv_rows();
        if (R.rc) return R.rc;
        if (int rc = plan_single_rows()) return rc;      // (host work, under the table phase enqueued above)
        if (int rc = run_chunks(guard)) return rc;
        h->out_recorded = true;          // (ps.released — the plan slot may be rewritten behind it, zett_forward_prepare — is recorded by the guard)
        return h->time_gemm ? read_gemm_timing(h, st) : 0;
    }

    // ---- plan ---------------------------------------------------------------------
    // The slot the previous forward did not use.  Prepared for exactly this call (zett_forward_prepare): its plan ran on the
    // plan stream, the host waits for THAT (not for earlier work on st) and st is ordered behind it.  Otherwise the plan is
    // made here, on st, and the host waits for it — and so for whatever was enqueued on st before.
    int take_plan() {
        zett_hypernet::PlanSlot& s = h->plan[h->plan_cur ^ 1];
        if (s.pending && s.sfm == sfm && s.n_rows == N && s.seq == seq && s.pair_plan == plan_layout(h, &s, N, seq).pair_plan &&
            s.ext_id_slot == h->ext.id_slot && s.local_slots == id_qkv_configured(h)) {
            HIP_TRY(hipStreamWaitEvent(st, s.done, 0));
        } else {
            if (s.pending) HIP_TRY(hipEventSynchronize(s.done));       // a prepared plan nobody took: let it finish before the slot is reused
            if (s.released) HIP_TRY(hipStreamWaitEvent(st, s.released, 0));      // (the forward before the previous one read this slot)
            if (int rc = enqueue_plan(h, s, sfm, N, seq, st)) return rc;
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
        if (!h->range_accumulate) HIP_TRY(hipMemsetAsync(h->range_word, 0, 4, st));          // range guard: the word of THIS forward (zett_check_range)
        for (hipEvent_t& e : h->out_ready)
            if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        const bool dest_check = dest && dest->rows;
        if (dest_check) {
            if (int rc = h->dest_word.reserve(4)) return rc;
            if (!h->dest_host) HIP_TRY(hipHostMalloc((void**)&h->dest_host, 4, hipHostMallocDefault));
            if (!h->dest_checked) HIP_TRY(hipEventCreateWithFlags(&h->dest_checked, hipEventDisableTiming));
            HIP_TRY(hipMemsetAsync(h->dest_word.p, 0, 4, st));
            hipLaunchKernelGGL(dest_rows_check_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, dest->rows, N, dest->n_dest_rows, h->dest_word.as<int32_t>());
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(h->dest_host, h->dest_word.p, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipEventRecord(h->dest_checked, st));
        }
        HIP_TRY(hipEventSynchronize(ps->done));
        hoff = ps->host;
        if (hoff[N + 2] != 0)
            return fail(ZETT_E_INDEX, "surface-form row %d holds an id outside [0, %d) (original_vocab_size %d + %d fallback rows)",
                        hoff[N + 2] - 1, c.original_vocab_size + c.n_extra, c.original_vocab_size, c.n_extra);
        if (dest_check) {
            HIP_TRY(hipEventSynchronize(h->dest_checked));
            if (h->dest_host[0] != 0)
                return fail(ZETT_E_INDEX, "destination row map: rows[%d] is outside the destination's %lld rows", h->dest_host[0] - 1, (long long)dest->n_dest_rows);
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
        const WorkspaceSizes ws = workspace_sizes(c, sizeof(T), seq, Ttot, D, h->max_chunk_tokens);
        MC = ws.chunk_tokens;
        MCS = (size_t)MC + 768;      // slack rows: the 384-row GEMM tile reads whole tiles of A (per lane, two lanes)
        if (int rc = reserve_workspace(h, ws, mode.fold, true)) return rc;
        R.a_rows_readable = (long)MCS;
        // (ABI 8) zett_forward_table: the table is the caller's — rows of the GLOBAL distinct-id list in the folded 16-bit layout,
        // computed by zett_table_rows here and on the peer ranks; tok_slot already holds global slots (enqueue_plan)
        const bool ext_table = h->ext.table != nullptr;
        if (ext_table && !mode.table_lo) return needs_folded_table("zett_forward_table");
        TBL = h->table.as<float>();
        // (lever 6: the call's rows of a caller's table are gathered into the handle's own table — gather_ext_table — and read from there)
        const bool ext_direct = ext_table && !id_qkv_configured(h);
        TBL16 = ext_direct ? (T*)const_cast<void*>(h->ext.table) : (T*)h->table.as<float>();
        TBLST = ext_direct ? const_cast<float*>(h->ext.stats) : (float*)((char*)h->table.as<float>() + (((size_t)D * H * sizeof(T) + 15) / 16) * 16);
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
        if (h->ext.table) {
            if constexpr (sizeof(T) == 2) launch_table_gather<T>(st, (const T*)h->ext.table, h->ext.stats, h->ext.id_slot, p.id_list, D, H, TBL16, TBLST);
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
        if (!h->single_rows || seq + (c.embed_lang ? 1 : 0) <= 1 || Ttot > MC || two_lanes()) return 0;
        int64_t ns = 0;
        for (int64_t n = 0; n < N; ++n) ns += hoff[n + 1] - hoff[n] == 1;
        if (ns == 0 || (h->single_rows == 1 && (ns / 256) * (int64_t)(2 * H / 256) < 256)) return 0;
        const size_t map_bytes = (size_t)N * 12, comp_at = round_up(map_bytes, 16);
        if (h->single_copied) HIP_TRY(hipEventSynchronize(h->single_copied));      // the staging's last copy has left it
        else HIP_TRY(hipEventCreateWithFlags(&h->single_copied, hipEventDisableTiming));
        if (h->single_host_bytes < map_bytes) {
            if (h->single_host) (void)hipHostFree(h->single_host);
            h->single_host = nullptr; h->single_host_bytes = 0;
            HIP_TRY(hipHostMalloc(&h->single_host, map_bytes, hipHostMallocDefault));
            h->single_host_bytes = map_bytes;
        }
        if (int rc = h->single_map.reserve(comp_at + (size_t)N * 8)) return rc;
        int64_t* hrow = (int64_t*)h->single_host;
        int32_t* hslot = (int32_t*)(hrow + N);
        int64_t at_single = 0, at_other = ns;
        for (int64_t n = 0; n < N; ++n) {
            const int64_t slot = hoff[n + 1] - hoff[n] == 1 ? at_single++ : at_other++;
            hslot[n] = (int32_t)slot;
            hrow[slot] = n;
        }
        HIP_TRY(hipMemcpyAsync(h->single_map.p, h->single_host, map_bytes, hipMemcpyHostToDevice, st));
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
        const bool cls_only = h->cls_only_last && l == c.layers - 1;
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
                launch_pair_qkv<T>(k.st, U, rw, by_pair ? k.P : k.m, k.hs_stats, md.id_cpos, seq, md.id_cw, md.id_bq, 3 * H, w.BIG, ld_q, h->range_word);
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
        launch_attention<T>(k.st, H, h->attention_fast, h->attention_pack, Q, ld_q, KV, KV + H, ld_kv, H / c.heads, p.row_offset, p.row_uniform, p.tok_key,
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
        ro.range_flag = h->range_word;
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
        if (!h->concurrent_lanes || Ttot > MC || N < 512) return false;
        const int Pn = pair_plan ? hoff[N + 3] : 0;
        const bool pairs_taken = pair_plan && Pn > 0 && (int64_t)Pn * 100 <= Ttot * 85;
        const double r = (double)((Ttot + 255) / 256) * (double)((H + 255) / 256) / 256.0;
        return h->concurrent_lanes == 2 || (!pairs_taken && !h->time_gemm && H >= 1024 && r < 4.0 && (std::ceil(r) - r) / std::ceil(r) > 0.08);
    }

    // lane selection and the join
    int run_chunks(SlotGuard& guard) {
        if (two_lanes()) {
            if (!h->lane_stream) HIP_TRY(hipStreamCreateWithFlags(&h->lane_stream, hipStreamNonBlocking));
            for (hipEvent_t& e : h->lane_ev)
                if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
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
int do_forward(zett_hypernet* h, const int32_t* sfm, int64_t N, int seq, const void* src, int src_dtype, const zett_dest* dest,
               int lang_index, float* out_in, float* out_out, float* out_bias, hipStream_t st) {
    Forward<T> f{h, sfm, N, seq, src, src_dtype, dest, lang_index, out_in, out_out, out_bias, st};
    return f.run();
}

}  // namespace
