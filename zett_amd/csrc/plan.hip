// plan.hip — the plan of a forward (plan.hip.h): surface forms -> packed positions, distinct referenced source ids and distinct
// (source id, position) pairs, on the device; and the two entry points that make a plan without running a forward
// (zett_forward_prepare, zett_table_plan).  The forward itself (zett_hip.hip) plans through enqueue_plan when nothing was prepared.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/zett_hip.h"
#include "common.hip.h"
#include "forward_handle.hip.h"
#include "plan.hip.h"
#include "scan.hip.h"

using namespace zett;

namespace zett {

constexpr int ID_QKV_MIN_HIDDEN = 4096;      // lever 6's default rule

static int64_t pair_keys(const zett_config& c, int seq) {
    return ((int64_t)c.original_vocab_size + c.n_extra + 1) * (int64_t)(seq + (c.embed_lang ? 1 : 0));
}

// ---- the plan's kernels (launched by enqueue_plan below and from nowhere else) ---------------------------------------------------
// ext_slot: the id_slot of a caller's table (zett_forward_table; null otherwise).  An id this row REFERENCES — what id_flag marks — must
// own a row of that table: id_slot is an exclusive scan, so an id the table's matrix never referenced carries the NEXT id's slot.
static __global__ void plan_rows_kernel(const int32_t* __restrict__ sfm, int64_t n_rows, int seq, int pad, int lam,
                                 int n_ids, const int32_t* __restrict__ ext_slot, PlanArrays p) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_rows) return;
    const int32_t* row = sfm + n * seq;
    int visible = 0;
    for (int j = 0; j < seq; ++j) {
        const int id = row[j];
        if (id < 0 || id >= n_ids) {          // F.embedding would raise IndexError here
            atomicMax(p.err, PLAN_ERR_RANGE | (int)(n + 1));
            p.row_count[n] = 0;
            p.row_uniform[n] = 2;             // poisoned: skipped by plan_tokens_kernel
            return;
        }
        visible += (id != pad);
    }
    const bool uniform = (visible + lam) == 0;
    int count;
    bool absent = false;
    auto reference = [&](int id) {
        p.id_flag[id] = 1;
        if (ext_slot && ext_slot[id + 1] == ext_slot[id]) absent = true;
    };
    if (uniform) {
        count = seq;
        for (int j = 0; j < seq; ++j) reference(row[j]);
    } else {
        count = visible + lam + (row[0] == pad ? 1 : 0);
        for (int j = 0; j < seq; ++j)
            if (j == 0 || row[j] != pad) reference(row[j]);
    }
    if (absent) atomicMax(p.err, (int)(n + 1));          // (below every PLAN_ERR_RANGE word: an id outside the vocabulary is reported first)
    p.row_count[n] = count;
    p.row_uniform[n] = uniform ? 1 : 0;
}

static __global__ void plan_tokens_kernel(const int32_t* __restrict__ sfm, int64_t n_rows, int seq, int pad, int lam,
                                   int n_ids, PlanArrays p) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= n_rows) return;
    const int32_t* row = sfm + n * seq;
    int t = p.row_offset[n];
    if (p.row_uniform[n] == 2) return;
    const bool uniform = p.row_uniform[n] == 1;
    const int lp = seq + lam;
    for (int j = 0; j < seq; ++j) {
        const int id = row[j];
        const bool vis = id != pad;
        if (uniform || vis || j == 0) {
            p.tok_slot[t] = p.id_slot[id];
            p.tok_pos[t] = j;
            p.tok_row[t] = (int32_t)n;
            p.tok_key[t] = vis ? 1 : 0;
            if (p.pair_flag) { const int key = id * lp + j; p.tok_pkey[t] = key; p.pair_flag[key] = 1; }
            ++t;
        }
    }
    if (lam) {
        p.tok_slot[t] = -1;
        p.tok_pos[t] = seq;
        p.tok_row[t] = (int32_t)n;
        p.tok_key[t] = 1;
        if (p.pair_flag) { const int key = n_ids * lp + seq; p.tok_pkey[t] = key; p.pair_flag[key] = 1; }
    }
}

// pair slot of every packed position, and (table slot, position) of every pair (tokens of one pair write the same values)
static __global__ void plan_pairs_kernel(int64_t n_rows, PlanArrays p) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= p.row_offset[n_rows]) return;          // (the grid covers the worst case: the host does not know T yet)
    const int ps = p.pair_slot[p.tok_pkey[t]];
    p.tok_pair[t] = ps;
    p.pair_tslot[ps] = p.tok_slot[t];
    p.pair_pos[ps] = p.tok_pos[t];
}

static __global__ void plan_idlist_kernel(int n_ids, PlanArrays p) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id < n_ids && p.id_flag[id]) p.id_list[p.id_slot[id]] = id;
    if (id == 0) {          // (the last kernel of a plan: every scan has run)
        p.counters[0] = p.id_slot[n_ids];
        p.counters[1] = p.err[0];
        p.counters[2] = p.n_pair_keys ? p.pair_slot[p.n_pair_keys] : 0;
    }
}

// ---- host --------------------------------------------------------------------------------------------------------------------------

int plan_error(const zett_hypernet* h, int32_t word) {
    const zett_config& c = h->cfg;
    if (word & PLAN_ERR_RANGE)
        return fail(ZETT_E_INDEX, "surface-form row %d holds an id outside [0, %d) (original_vocab_size %d + %d fallback rows)",
                    (word & ~PLAN_ERR_RANGE) - 1, c.original_vocab_size + c.n_extra, c.original_vocab_size, c.n_extra);
    if (word)
        return fail(ZETT_E_INDEX, "surface-form row %d references a source id that is not in the table: the matrix the table was planned from "
                                  "(zett_table_plan) never referenced it, so id_slot gives it no row", word - 1);
    return 0;
}

PlanLayout plan_layout(const zett_hypernet* h, const PlanSlot* s, int64_t N, int seq, bool worst_case) {
    const zett_config& c = h->cfg;
    const int lam = c.embed_lang ? 1 : 0;
    const int64_t V = (int64_t)c.original_vocab_size + c.n_extra;
    const int64_t max_tok = N * (int64_t)(seq + lam);
    PlanLayout L;
    PlanArrays& p = L.p;
    L.PK = pair_keys(c, seq);          // K = (V+1)(L+lang)
    L.pair_plan = worst_case || (h->opt.pair_dedupe && c.layers >= 2 && L.PK <= std::max<int64_t>(4 * max_tok, (int64_t)1 << 23) && L.PK < (int64_t)0x7fffffff);
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

size_t plan_i32_bytes(const zett_hypernet* h, int64_t N, int seq) { return plan_layout(h, nullptr, N, seq, true).words * 4; }

bool id_qkv_configured(const zett_hypernet* h) {
    return h->opt.id_qkv && h->m.id_u.w && (h->opt.id_qkv == 2 || h->cfg.hidden >= ID_QKV_MIN_HIDDEN);
}

int enqueue_plan(zett_hypernet* h, PlanSlot& s, const ExtTable* ext, const int32_t* sfm, int64_t N, int seq, hipStream_t st) {
    const zett_config& c = h->cfg;
    const int lam = c.embed_lang ? 1 : 0;
    const int V = c.original_vocab_size + c.n_extra;
    const int64_t max_tok = N * (int64_t)(seq + lam);
    if (int rc = s.i32.reserve(plan_i32_bytes(h, N, seq))) return rc;
    if (int rc = s.u8.reserve((size_t)N + (size_t)max_tok)) return rc;
    const size_t need_ints = (size_t)N + 1 + 3;
    if (s.host_ints < need_ints) {
        s.host_ints = 0;
        HIP_TRY(s.host.alloc(need_ints * 4));
        s.host_ints = need_ints;
    }
    if (!s.done) HIP_TRY(hipEventCreateWithFlags(&s.done.e, hipEventDisableTiming));
    if (!s.released) HIP_TRY(hipEventCreateWithFlags(&s.released.e, hipEventDisableTiming));
    const PlanLayout L = plan_layout(h, &s, N, seq);
    const PlanArrays& p = L.p;
    HIP_TRY(hipMemsetAsync(s.i32.p, 0, L.n_clear * 4, st));          // id_flag, pair_flag, err: one piece of the arena
    const int rb = (int)((N + 255) / 256);
    const int32_t* ext_id_slot = ext ? ext->id_slot : nullptr;
    // (both arms of a forward on a caller's table — plan_tokens_kernel's lookup below, lever 6's gather — are checked here, where every referenced id passes)
    hipLaunchKernelGGL(plan_rows_kernel, dim3(rb), dim3(256), 0, st, sfm, N, seq, c.pad_token_id, lam, V, ext_id_slot, p);
    launch_exclusive_scan(p.row_count, p.row_offset, N, L.scan_tmp, st);
    launch_exclusive_scan(p.id_flag, p.id_slot, (int64_t)V, L.scan_tmp, st);
    {
        // (ABI 8) a forward on a caller-provided table: a token's table slot is its id's slot in the GLOBAL distinct-id list
        PlanArrays pt = p;
        // (lever 6 gathers the call's rows of that table into the handle's own table first and keeps the plan's own slots)
        if (ext_id_slot && !id_qkv_configured(h)) pt.id_slot = const_cast<int32_t*>(ext_id_slot);
        hipLaunchKernelGGL(plan_tokens_kernel, dim3(rb), dim3(256), 0, st, sfm, N, seq, c.pad_token_id, lam, V, pt);
    }
    if (L.pair_plan) {
        launch_exclusive_scan(p.pair_flag, p.pair_slot, L.PK, L.scan_tmp, st);
        hipLaunchKernelGGL(plan_pairs_kernel, dim3((unsigned)((max_tok + 255) / 256)), dim3(256), 0, st, N, p);
    }
    hipLaunchKernelGGL(plan_idlist_kernel, dim3((V + 255) / 256), dim3(256), 0, st, V, p);
    HIP_TRY(hipGetLastError());
    // the row offsets and, right behind them, the three counters (distinct ids, error word, distinct pairs) to the host: one copy
    HIP_TRY(hipMemcpyAsync(s.host.p, p.row_offset, ((size_t)N + 1 + 3) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipEventRecord(s.done, st));
    s.sfm = sfm; s.n_rows = N; s.seq = seq; s.pair_plan = L.pair_plan; s.ext_id_slot = ext_id_slot; s.local_slots = id_qkv_configured(h);
    return 0;
}

}  // namespace zett

extern "C" {

int zett_forward_prepare(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq, void* input_stream) {
    CallCheck k;
    k.n_rows = n_rows; k.seq = seq; k.empty_ok = true; k.null_arg = !surface_forms;
    if (int rc = check_call(h, k)) return rc == CALL_EMPTY ? 0 : rc;
    ZETT_ON_DEVICE(h->device);
    if (!h->plan_stream) {      // highest priority: the plan's small workgroups must get CUs while a forward's GEMM tiles own the chip
        int least = 0, greatest = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&least, &greatest));
        HIP_TRY(hipStreamCreateWithPriority(&h->plan_stream.s, hipStreamNonBlocking, greatest));
    }
    if (!h->plan_fork) HIP_TRY(hipEventCreateWithFlags(&h->plan_fork.e, hipEventDisableTiming));
    PlanSlot& ps = h->plan[h->plan_cur ^ 1];
    if (ps.pending) HIP_TRY(hipEventSynchronize(ps.done));           // replaces a prepared plan nobody took
    // behind the surface forms (whatever input_stream holds now) and behind the forward that last read this slot
    HIP_TRY(hipEventRecord(h->plan_fork, (hipStream_t)input_stream));
    HIP_TRY(hipStreamWaitEvent(h->plan_stream, h->plan_fork, 0));
    if (ps.released) HIP_TRY(hipStreamWaitEvent(h->plan_stream, ps.released, 0));
    if (int rc = enqueue_plan(h, ps, nullptr, surface_forms, n_rows, seq, h->plan_stream)) return rc;
    ps.pending = true;
    return 0;
}

// (ABI 8) the hoisted table shared between ranks (SURVEY 8e's optional second exchange): the distinct ids of a whole vocabulary
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
    PlanSlot& ps = h->table_plan;
    if (int rc = enqueue_plan(h, ps, nullptr, surface_forms, n_rows, seq, st)) return rc;          // (this plan numbers the ids itself)
    HIP_TRY(hipEventSynchronize(ps.done));
    const int32_t* hoff = ps.host.p;
    if (int rc = plan_error(h, hoff[n_rows + 2])) return rc;
    const int D = hoff[n_rows + 1];
    const PlanLayout L = plan_layout(h, &ps, n_rows, seq);
    HIP_TRY(hipMemcpyAsync(id_slot_out, L.p.id_slot, ((size_t)V + 1) * 4, hipMemcpyDeviceToDevice, st));
    if (D > 0) HIP_TRY(hipMemcpyAsync(id_list_out, L.p.id_list, (size_t)D * 4, hipMemcpyDeviceToDevice, st));
    *n_ids_out = D;
    return 0;
}

}  // extern "C"
