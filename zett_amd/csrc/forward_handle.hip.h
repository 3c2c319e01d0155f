// forward_handle.hip.h — the handle of the hypernet forward (zett_hypernet) as its three units see it: model.hip (weights, options,
// getters), plan.hip (the integer plan of a call) and zett_hip.hip (the forward proper).  Private: not part of include/.
//
// The handle owns what it holds BY TYPE: every device allocation, pinned allocation, event and stream below is a member whose
// destructor releases it, so zett_destroy is `delete h` and a failed zett_create / zett_finalize frees what it had got.  What
// belongs to ONE call (the caller's table, whether launches are timed) is an argument of that call, never a field here.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <deque>
#include <map>
#include <string>
#include <vector>

#include "../../include/zett_hip.h"
#include "common.hip.h"

namespace zett {

// ---- owners: a pointer and a destructor each; creation stays with the code that needs the thing (most are made lazily) ----------
struct Event {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(const Event&) = delete;
    Event& operator=(const Event&) = delete;
    ~Event() { if (e) (void)hipEventDestroy(e); }
    operator hipEvent_t() const { return e; }
};
struct Stream {
    hipStream_t s = nullptr;
    Stream() = default;
    Stream(const Stream&) = delete;
    Stream& operator=(const Stream&) = delete;
    ~Stream() { if (s) (void)hipStreamDestroy(s); }
    operator hipStream_t() const { return s; }
};
template <typename T>
struct Pinned {          // pinned host memory
    T* p = nullptr;
    Pinned() = default;
    Pinned(const Pinned&) = delete;
    Pinned& operator=(const Pinned&) = delete;
    ~Pinned() { release(); }
    void release() { if (p) (void)hipHostFree(p); p = nullptr; }
    hipError_t alloc(size_t bytes) { release(); return hipHostMalloc((void**)&p, bytes, hipHostMallocDefault); }
};
template <typename T>
struct DevMem {          // one device allocation of a fixed size (DevBuf, common.hip.h, is the grow-only one)
    T* p = nullptr;
    DevMem() = default;
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
    hipError_t alloc(size_t bytes) { release(); return hipMalloc((void**)&p, bytes); }
};

// ---- the model ---------------------------------------------------------------------------------------------------------------------
struct Tensor {          // an uploaded weight
    DevMem<float> f32;          // device fp32 copy (biases, LN, embeddings, ... and GEMM weights in F32 mode)
    DevMem<void> lo;            // 16-bit modes: GEMM operand copy in the handle's arithmetic type (the fp32 mode reads f32)
    std::vector<int64_t> shape;
    size_t numel = 0;
};

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

inline size_t elt_size(int precision) { return precision == ZETT_PREC_F32 ? 4 : 2; }

// ---- options (zett_set_option; include/zett_hip.h documents them): the ONE place an option lives, read where it is used ----------
struct Options {
    int64_t max_chunk_tokens = 0;     // 0 = auto: chunk_token_cap() (131 072 at H = 4096, more for narrower hypernets)
    int time_gemm = 0;
    int cls_only_last = 1;
    int pair_dedupe = 1;              // layer 0's Q/K/V once per distinct (source id, position) pair (do_forward)
    int residual_lo = 1;              // 16-bit residual stream of the encoder (gemm4d LN16 producers): 1 = in f16 mode, 2 = in bf16 mode too (A/B), 0 = fp32 stream
    int concurrent_lanes = 0;         // a one-chunk call as TWO half-vocabulary chunks on two streams (do_forward): 0 never, 1 auto (when the narrow GEMMs
                                      // of the call leave > 8 % of their last round of 256 CUs idle: the 4 096-row shards of 8 GPUs), 2 always
    int attention_fast = 1;           // rows of <= 8 packed positions: keys / values fetched once, all keys of a query side by side (rowops.hip.h)
    int attention_pack = 1;           // a last column group of 256 / 128 / 64 columns (H = 768) takes 2 / 4 / 8 rows per wave instead of idle lanes (r6; same bits)
    int ln_fold = 1;
    int ln_rows8 = 1;                 // 16-bit modes, H <= 2048: LayerNorm launches on layernorm_rows8_kernel (eight columns per lane; rowops.hip.h); 0 = the float4 kernel (A/B)
    int table_lo = 1;                 // 16-bit hoisted table with the ProjectorBlock's LayerNorm folded into the embeddings' kernel (with the 16-bit residual stream); 0 = fp32 table (A/B)
    int range_accumulate = 0;         // 1: zett_forward does not clear the range word, zett_check_range clears it after reading (a caller
                                      // that runs several asynchronous forwards and asks once at the end: zett_amd/sharding.py)
    int single_rows = 1;              // lever 5: 0 off, 1 auto (one chunk on one lane, at least one full round of 256x256 tiles saved per launch), 2 whenever possible
    int id_qkv = 1;                   // lever 6: 0 off, 1 when possible and hidden >= ID_QKV_MIN_HIDDEN, 2 whenever possible
    GemmOptions gemm;                 // gemm_variant, gemm4d_min_k, gemm_tail_split, gemm_tile_order, gemm_group: what Runner::gemm passes on
};

// ---- per-call state that is NOT the handle's -----------------------------------------------------------------------------------------
// (ABI 8) the hoisted table of a forward that comes from the caller (zett_forward_table): rows of the global distinct-id list
// computed by zett_table_rows — on this rank and on its peers — instead of this call's own distinct ids.  An argument of the
// call (null for zett_forward, zett_forward_into, zett_forward_prepare and zett_table_plan).
struct ExtTable { const void* table = nullptr; const float* stats = nullptr; const int32_t* id_slot = nullptr; };

// The plan of a forward (integers: packed positions, distinct ids, pairs) lives in one of TWO slots that forwards take in
// turn, so that the plan of the NEXT forward can be made (zett_forward_prepare, on plan_stream) while the kernels of the
// current one still read theirs.
struct PlanSlot {
    DevBuf i32, u8;
    Pinned<int32_t> host;             // row offsets [N+1], distinct ids, error word, distinct pairs
    size_t host_ints = 0;
    Event done;                       // the plan's kernels and copies have run
    Event released;                   // the forward that used this slot has finished with it
    const int32_t* sfm = nullptr;     // what the slot was prepared for (zett_forward_prepare), pending until a forward takes it
    int64_t n_rows = 0;
    int seq = 0;
    bool pair_plan = false;           // the layout it was made with (an option changed in between: the forward plans again)
    const int32_t* ext_id_slot = nullptr;   // the id -> table-slot map its tok_slot was written with (null: the plan's own)
    bool local_slots = false;         // lever 6 was configured: tok_slot holds the plan's own slots even with a caller's table
    bool pending = false;
};

// What the entry points of the forward family (zett_forward[_into], zett_forward_table[_into], zett_forward_prepare, zett_table_plan,
// zett_table_rows) check before they touch the device, in the one order in which they report it (check_call, zett_hip.hip).  An
// entry point fills in what it has; the fields say where the entry points differ.  Returns 0, an error code, or CALL_EMPTY: a
// valid call on no rows.
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

int check_call(const zett_hypernet* h, const CallCheck& k);

}  // namespace zett

struct zett_hypernet {
    zett_config cfg{};
    int device = 0;
    int precision = ZETT_PREC_BF16;
    bool finalized = false;
    std::map<std::string, zett::Tensor> w;    // the uploaded tensors, by name, and their owner (zett_load_weight, zett_finalize)
    std::vector<zett::WeightDecl> decl;       // every weight the library reads, sorted by name (zett_create); its slots point into `m`
    zett::Model m;                            // what the forward reads
    std::deque<zett::DevMem<void>> owned;     // the fused / derived operands zett_finalize built (keep)
    zett::Options opt;
    // workspace
    zett::PlanSlot plan[2];
    zett::PlanSlot table_plan;        // (ABI 8) scratch plan of zett_table_plan: the distinct ids of a WHOLE vocabulary, never taken by a forward
    int plan_cur = 0;                 // slot of the most recent forward
    zett::Stream plan_stream;
    zett::Event plan_fork;
    zett::Stream lane_stream;         // "concurrent_lanes": the second lane
    zett::Event lane_ev[4];           // fork, lane 1: bias written / out_in written / done
    zett::DevBuf table, x0, yf, yt, big, pre, ctx, cf, ct, lnstats, lnparts;
    zett::Event out_ready[2];         // zett_stream_wait_output: out_in / out_bias of the last forward complete
    bool out_recorded = false;
    zett::DevMem<int32_t> range_word; // zett_range_bits of the forward in flight (cleared when a forward starts)
    zett::Pinned<int32_t> range_host; // where zett_check_range / zett_finalize read it
    // (zett_forward_into) the row map's check against the destination (read with the plan's error word), and the fp32 rows of the head
    // launches that take the staged fallback of the destination store (Runner::head_gemm)
    // (dest_stage[1]: lane 1 of a "concurrent_lanes" pair — the two lanes' staged heads run at the same time)
    zett::DevBuf dest_word, dest_stage[2], dest_sink;
    zett::Pinned<int32_t> dest_host;
    zett::Event dest_checked;
    // Lever 5 (Forward::plan_single_rows): rows with a single kept position first in the position-0 block, their query /
    // key GEMM rows skipped.  single_map — reserved only when a forward takes the lever, outside zett_workspace_bytes like dest_sink —
    // holds cls_row int64 [N] (buffer row -> vocabulary row), cls_slot int32 [N] (the inverse) and, behind them, the composition with a
    // caller's row map; single_host is the pinned staging of the first two, single_copied the event behind their copy.
    int64_t single_rows_last = 0;     // single rows the last forward skipped (zett_single_rows)
    // Lever 6 (Forward::id_qkv_rows): layer 0's Q/K/V once per distinct source id
    int64_t id_qkv_last = 0;          // table rows layer 0's Q/K/V GEMM of the last forward ran on (zett_id_qkv)
    zett::DevBuf single_map;
    zett::Pinned<void> single_host;
    size_t single_host_bytes = 0;
    zett::Event single_copied;
    std::deque<zett::Event> ev;       // "time_gemm": launch k of the last forward has the event pair ev[2k], ev[2k + 1]
    size_t ev_used = 0;
    std::vector<zett_gemm_record> gemm_log;     // every GEMM launch of the last forward (zett_get_gemm_log)
    zett_stats stats{};

    // a device allocation that lives as long as the handle
    template <typename U> hipError_t keep(U*& out, size_t bytes) {
        owned.emplace_back();
        const hipError_t e = owned.back().alloc(bytes);
        out = (U*)owned.back().p;
        return e;
    }
};
