// plan.hip.h — the integer plan of one forward: where its arrays lie (PlanArrays, PlanLayout) and how it is made (plan.hip).
//
// Reference semantics being preserved (modeling_hypernet.py:190, 220-234 and the eager RobertaSelfAttention mask):
//   * key j of row n is visible iff ids[n,j] != pad (the language token always is);
//   * only hidden[:,0] is read out, so a position matters only as a visible key or as
//     position 0 (a query even when it is pad);
//   * a row whose keys are ALL masked attends uniformly to every position (additive
//     finfo.min on every key), so such a row keeps all L positions, flagged uniform.
// Everything else (pad positions of ordinary rows) never influences an output and is
// not computed.
//
// Light on purpose (no handle, no kernel): the row kernels that READ a plan (rowops.hip.h) include it for PlanArrays.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

struct zett_hypernet;

namespace zett {

struct PlanSlot;
struct ExtTable;

struct PlanArrays {
    int32_t* row_count;     // [N]   packed positions of row n
    int32_t* row_offset;    // [N+1] exclusive scan of row_count
    uint8_t* row_uniform;   // [N]
    int32_t* id_flag;       // [V]   1 if the id is referenced by a kept position
    int32_t* id_slot;       // [V+1] exclusive scan of id_flag; id_slot[V] = distinct ids
    int32_t* id_list;       // [<=V] slot -> id
    int32_t* tok_slot;      // [T]   table slot of the token, -1 = language token
    int32_t* tok_pos;       // [T]   position index (for position_embeddings)
    int32_t* tok_row;       // [T]   row the packed position belongs to
    // distinct (source id, position) pairs: what the embeddings' output — and so layer 0's Q/K/V — depends on
    int32_t* tok_pkey;      // [T]   id * Lp + position (Lp = L + lang; the language token counts as id V)
    int32_t* pair_flag;     // [(V+1)*Lp]   1 if the pair occurs (null: the lever is off for this call)
    int32_t* pair_slot;     // [(V+1)*Lp+1] exclusive scan of pair_flag; last = distinct pairs
    int32_t* tok_pair;      // [T]   pair slot of the packed position
    int32_t* pair_tslot;    // [P]   table slot of the pair (-1 = language token)
    int32_t* pair_pos;      // [P]   its position index
    uint8_t* tok_key;       // [T]   visible as key
    int32_t* err;           // [1]   the plan's error word (plan_error): the largest of PLAN_ERR_RANGE | (1 + row) over the rows with an id outside the
                            //       vocabulary and 1 + row over the rows that reference an id a caller's table does not hold
    int32_t* counters;      // [3]   behind row_offset[N]: distinct ids, the error word, distinct pairs — what the host reads with the row offsets, in ONE copy
    int32_t n_pair_keys;    //       size of pair_flag (0: no pair plan)
};

// A row number fits under the bit: a call holds fewer than 2^31 - 1 positions of at least two per row (check_call).
constexpr int32_t PLAN_ERR_RANGE = 0x40000000;
// the plan's error word as the host read it -> 0, or ZETT_E_INDEX with the message of its kind
int plan_error(const zett_hypernet* h, int32_t word);

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
PlanLayout plan_layout(const zett_hypernet* h, const PlanSlot* s, int64_t N, int seq, bool worst_case = false);
// worst case of a slot's int32 arena for [N, seq] surface forms: what enqueue_plan reserves and zett_workspace_bytes counts
size_t plan_i32_bytes(const zett_hypernet* h, int64_t N, int seq);

// Lever 6 as far as the configuration and the options decide it (what is left to the forward: ForwardMode::table_lo, which a
// caller's table needs anyway): zett_finalize built the operands (16-bit mode, >= 2 layers, no language position) and the rule holds.
bool id_qkv_configured(const zett_hypernet* h);

// The plan of one forward into slot s, on stream st: six small kernels, three scans, and the copy of the row offsets and the
// three counters to pinned memory; s.done is recorded behind them.  ext: the caller's table of the forward the plan is for (null:
// the plan numbers the ids itself); every id the call references must then own a row of it, or the error word says which row does not.
int enqueue_plan(zett_hypernet* h, PlanSlot& s, const ExtTable* ext, const int32_t* sfm, int64_t N, int seq, hipStream_t st);

}  // namespace zett
