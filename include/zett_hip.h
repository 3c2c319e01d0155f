/*
 * zett_hip.h — C ABI of libzett_hip.so, the MI355X (gfx950) implementation of
 * ZeTT's embedding-prediction hot path.
 *
 * The reference (bminixhofer/zett) has no C ABI on this path: its boundary is a
 * Python class and a Python function.  Each entry point below names the
 * reference interface it stands behind; INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add to hf_hypernet/modeling_hypernet.py and
 * zett/utils.py.
 *
 * Conventions
 *   - plain C types only; no torch / HIP types in any signature.  `stream` is a
 *     hipStream_t passed as void* (NULL = default stream).
 *   - every function returns 0 on success or a negative ZETT_E_* code;
 *     zett_last_error() returns the message of the calling thread's last failure.
 *   - unless a parameter says "host", pointers are device pointers on the
 *     handle's device, owned by the caller (e.g. PyTorch-ROCm tensors).
 *   - a handle is bound to one device; calls on one handle must not overlap.
 */
#ifndef ZETT_HIP_H
#define ZETT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZETT_ABI_VERSION 8      /* 2: zett_stats gained distinct_positions; 3: ZETT_E_RANGE, zett_check_range;
                                   4: ZETT_RETOK_WORDPIECE (zett_retok_model gained piece_continuing, max_input_chars_per_word);
                                   5: zett_forward_prepare, zett_retokenize_async / zett_retok_result;
                                   6: zett_retokenize_async takes NUL-separated text (offsets == NULL); options gemm_tail_split;
                                   7: zett_retok_set_option;
                                   8: zett_table_plan, zett_table_rows, zett_forward_table (the hoisted table shared between ranks);
                                      additive, ABI 8: zett_forward_into, zett_forward_table_into, struct zett_dest, ZETT_RANGE_DEST;
                                      additive, ABI 8: zett_lexical_create / _destroy / _plan / _rows_into, enum zett_lexical_mode */

enum zett_status {
    ZETT_OK = 0,
    ZETT_E_INVALID = -1,      /* bad argument / unsupported shape                 */
    ZETT_E_HIP = -2,          /* a HIP runtime call failed                        */
    ZETT_E_STATE = -3,        /* weights missing, handle not finalized, ...       */
    ZETT_E_INDEX = -4,        /* surface-form id outside [0, V0 + n_extra)        */
    ZETT_E_NOT_IMPLEMENTED = -5,
    ZETT_E_KEY = -6,          /* character outside the byte table (KeyError)      */
    ZETT_E_RANGE = -7         /* a value left the range of the 16-bit operand type, or an output is not finite
                                 (zett_finalize: a weight; zett_check_range: the last forward)              */
};

/* Bits of the range word (zett_check_range). */
enum zett_range_bits {
    ZETT_RANGE_SOURCE = 1,      /* in_scaler(source_embeddings[id]) of a referenced id does not fit the operand type */
    ZETT_RANGE_ACTIVATION = 2,  /* a 16-bit GEMM output (Q/K/V, FFN intermediate, the operand copy of the residual sum) */
    ZETT_RANGE_OUTPUT = 4,      /* a predicted embedding is inf / NaN                                                */
    ZETT_RANGE_WEIGHT = 8,      /* a GEMM weight (or a LayerNorm-folded weight) does not fit: reported by zett_finalize */
    ZETT_RANGE_DEST = 16        /* zett_forward_into: a finite value did not fit an f16 destination; stored as inf.  Repeating the
                                   call in bf16 arithmetic would not help: the destination's type is the caller's choice     */
};

enum zett_dtype { ZETT_F32 = 0, ZETT_F16 = 1, ZETT_BF16 = 2 };

/* Arithmetic of the dense contractions.
 *   BF16: bf16 operands, fp32 accumulate (v_mfma_f32_32x32x16_bf16); LayerNorm,
 *         softmax, GELU, residual stream and outputs in fp32.  (The reference CLI
 *         defaults to bf16 end to end: scripts/transfer.py:41,145-151.)
 *   F32 : exact fp32 (v_mfma_f32_32x32x2_f32), the hf_hypernet arithmetic.
 *   F16 : IEEE-half operands, fp32 accumulate (v_mfma_f32_*_f16): 8x smaller operand rounding
 *         than BF16 (11 instead of 8 significand bits) at the same MFMA rate; ~4 % slower end to
 *         end, because the GEMMs are power-limited and wider significands cost energy.  Operands
 *         must stay inside the half range (|x| < 65504), which LayerNorm'd activations and
 *         embedding-scale weights do.
 *         The default of the Python layer (zett_amd/hypernet.py DEFAULT_PRECISION): bf16 sits on the edge
 *         of the 1e-2 parity tolerance at the 4096-wide shapes (tests/test_full_size_gpu.py). */
enum zett_precision { ZETT_PREC_BF16 = 0, ZETT_PREC_F32 = 1, ZETT_PREC_F16 = 2 };

/* Shape / flag block.  Mirrors the fields of ZettHypernetConfig that the forward
 * reads (hf_hypernet/configuration_hypernet.py:3-56 plus the fields train.py
 * injects: pad_token_id, original_vocab_size, separate_out_embeddings,
 * hn_n_extra_tokens — SURVEY.md §8a A11). */
typedef struct zett_config {
    int32_t n_embd;               /* E                                             */
    int32_t n_in_embd;            /* E_in = 2E if separate_out_embeddings else E   */
    int32_t hidden;               /* hn_hidden_size                                */
    int32_t intermediate;         /* hn_intermediate_size                          */
    int32_t heads;                /* hn_num_attention_heads                        */
    int32_t layers;               /* hn_n_layers                                   */
    int32_t n_extra;              /* rows of fallback_embeddings = max(X, 1)       */
    int32_t original_vocab_size;  /* V0                                            */
    int32_t pad_token_id;
    int32_t separate_out;         /* separate_out_embeddings                       */
    int32_t single_head;          /* hn_single_head                                */
    int32_t rescale;              /* hn_rescale_embeddings                         */
    int32_t predict_bias;         /* hn_predict_bias                               */
    int32_t embed_lang;           /* hn_embed_lang_id                              */
    int32_t n_langs;
    int32_t max_positions;        /* rows of position_embeddings (514)             */
    float ln_eps_encoder;         /* 1e-5 (roberta-base layer_norm_eps)            */
    float ln_eps_projector;       /* 1e-6 (ProjectorBlock.ln)                      */
} zett_config;

/* Counters of the most recent zett_forward on a handle. */
typedef struct zett_stats {
    int64_t rows;                 /* N                                             */
    int64_t packed_tokens;        /* positions that entered the encoder            */
    int64_t distinct_ids;         /* rows of the hoisted input-projection table    */
    int64_t chunks;               /* encoder row chunks                            */
    double executed_flops;        /* 2*M*N*K summed over every GEMM launch         */
    double gemm_ms;               /* sum of GEMM launch durations (timing on)      */
    int64_t gemm_launches;
    double gemm_flops_timed;      /* flops of the launches counted in gemm_ms      */
    int64_t distinct_positions;   /* rows of layer 0's Q/K/V launch: distinct (source id, position) pairs when that
                                     lever is taken (one chunk, >= 15 % repeats), else packed_tokens            */
} zett_stats;

typedef struct zett_hypernet zett_hypernet;
typedef struct zett_retok zett_retok;
typedef struct zett_lexical zett_lexical;

const char* zett_last_error(void);
int zett_abi_version(void);

/* ---- hypernetwork forward -------------------------------------------------
 * Replaces: ZettHypernet.__init__ / load_state_dict / __call__
 *           (hf_hypernet/modeling_hypernet.py:46-154, 156-267). */

int zett_create(const zett_config* cfg, int device, int precision, zett_hypernet** out);
int zett_destroy(zett_hypernet* h);

/* Upload one checkpoint tensor under its PyTorch state_dict name
 * (scripts/convert_to_pt.py:35-49).  `data` may be a host or a
 * device pointer; the library keeps its own repacked copy.  Unknown names and the
 * never-read model.embeddings.word_embeddings.weight are accepted and ignored
 * (returns 0). */
int zett_load_weight(zett_hypernet* h, const char* name, const void* data, int dtype,
                     const int64_t* shape, int ndim);

/* Check that every tensor the config needs was loaded; build fused operands. */
int zett_finalize(zett_hypernet* h);

/* ZettHypernet.__call__(target_surface_forms, source_embeddings=..., lang_index=...)
 *   surface_forms  int32 [n_rows, seq] row-major (what get_surface_form_matrix emits)
 *   source_embeddings [v_src, n_in_embd] row-major, dtype src_dtype
 *   lang_index     -1 = None
 *   out_in  fp32 [n_rows, n_embd]; out_out fp32 [n_rows, n_embd] or NULL when the
 *   config has no second output; out_bias fp32 [n_rows] (zeros when !predict_bias).
 * Returns ZETT_E_INDEX where the reference's F.embedding would raise IndexError. */
int zett_forward(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq,
                 const void* source_embeddings, int src_dtype, int64_t v_src, int32_t lang_index,
                 float* out_in, float* out_out, float* out_bias, void* stream);

/* ---- predicted rows straight into a destination matrix (additive, ABI 8) ------------------------------------------------
 * Replaces: what every caller of the reference's hypernet(...) does next — resize the model's embedding matrix, then copy the
 * predicted rows in with index_put_ and cast them to the model's dtype (README `hypernet(sfm, source_embeddings=...)`), or
 * accumulate them into [V, E] matrices with index_add_ (scripts/transfer.py:96-111).
 * zett_forward_into / zett_forward_table_into are zett_forward / zett_forward_table whose three outputs go to the caller's
 * matrices: input row i goes to row rows[i] (< 0: not written; rows == NULL: row i) of `in` / `out` / `bias`, with the
 * destination's own leading dimension (elements) and type.  The stored value is the fp32 value zett_forward stores: bit for bit
 * in an fp32 destination, rounded to nearest even in a bf16 / f16 one (what torch's .to(dtype) gives, inf included).
 *   in / out      [n_dest_rows, >= ld] of `dtype`; out is NULL iff the config has no second output
 *   bias          [n_dest_rows] of `bias_dtype`, or NULL: the bias is not written
 *   rows          device int64 [n_rows], or NULL (then n_dest_rows >= n_rows).  Checked against n_dest_rows on the device with the
 *                 plan's error word: ZETT_E_INDEX at the point where zett_forward reports a bad id, before any output is written.
 *                 (The check runs on `stream`, behind whatever wrote the map: with a prepared plan the host waits for `stream`
 *                 too.)  Two input rows with the same destination row: undefined which one lands.
 * ld_in / ld_out < n_embd, an unknown dtype, a NULL `in` or a NULL / non-NULL `out` that does not match the config: ZETT_E_INVALID.
 * Everything else as zett_forward: zett_forward_prepare, chunking, "concurrent_lanes", the pair plan, zett_stream_wait_output
 * (ZETT_OUT_IN: the destination's `in` rows are written; ZETT_OUT_BIAS: its bias).  ZETT_RANGE_OUTPUT is tested on the fp32
 * value, ZETT_RANGE_DEST on the destination's.
 * Where the conversion happens: in the 16-bit arithmetic modes the output heads' GEMM epilogues store into the destination
 * themselves (gemm4d's F32_SCALE / F32_SCALE_FOLD epilogues, 256x256 and 128x256 tiles; gemm log bit 10), and the position-0
 * readout stores the bias.  These launches instead write fp32 rows to the handle's workspace and a converting scatter
 * (the counterpart of zett_scatter_rows) moves them (gemm log bit 11): every head of the F32 arithmetic mode; hn_single_head with
 * separate outputs (one launch, two destinations); head launches that take another tile than gemm4d (M or N <= 128, K below
 * "gemm4d_min_k", a forced "gemm_variant"); heads without the Rescaler and without the LayerNorm fold (plain F32 epilogue); a
 * destination whose base or leading dimension is not a multiple of four values.  Same bits either way. */
typedef struct zett_dest {
    void* in; void* out; void* bias;      /* out: NULL iff the config has no second output; bias: NULL = not written */
    int32_t dtype; int32_t bias_dtype;    /* zett_dtype: ZETT_F32 / ZETT_F16 / ZETT_BF16 */
    int64_t ld_in; int64_t ld_out;        /* elements between destination rows, >= n_embd */
    const int64_t* rows;                  /* [n_rows] destination row of each input row, < 0 = skip; NULL = identity */
    int64_t n_dest_rows;                  /* rows in the destination (bounds of `rows`) */
} zett_dest;
int zett_forward_into(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq,
                      const void* source_embeddings, int src_dtype, int64_t v_src, int32_t lang_index,
                      const zett_dest* dest, void* stream);

/* How asynchronous zett_forward is.  The launches of a forward are sized by its PLAN (packed positions, distinct source ids,
 * distinct (id, position) pairs: integers computed on the device from the surface forms), so zett_forward enqueues the plan
 * (six small kernels), waits on the HOST for it and for its error word (ZETT_E_INDEX is returned synchronously, as the
 * reference's IndexError is raised), enqueues the ~60 launches of the forward and returns while they run.  Made on `stream`
 * itself, the plan sits behind whatever that stream still holds — a second zett_forward on the same stream waits for the
 * whole first one before it can enqueue anything.  zett_forward_prepare removes that wait: it enqueues the plan of the NEXT
 * zett_forward (same surface_forms pointer, n_rows, seq) on a stream the handle owns, behind the work `input_stream` holds NOW
 * (the stream the surface forms were produced on — pass one that is not busy with an earlier forward, e.g. the stream the
 * retokenizer ran on before the first forward was enqueued) and returns at once; plans live in two slots that forwards take
 * in turn, so the plan of forward k+1 runs while the kernels of forward k read theirs (it waits for forward k-1 to release
 * its slot).  The matching zett_forward then waits on the host for the plan only.  A prepared plan that the next
 * zett_forward does not match is discarded.  The reference has no counterpart (XLA sizes nothing from data). */
int zett_forward_prepare(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq, void* input_stream);

int zett_get_stats(const zett_hypernet* h, zett_stats* out);

/* Rows of the most recent forward that had a single kept position and whose query / key GEMM rows were skipped (the
 * "single_rows" option below); 0 when the forward did not take the lever.  (A getter of its own: zett_stats keeps its layout.) */
int zett_single_rows(const zett_hypernet* h, int64_t* out);

/* Table rows layer 0's Q/K/V GEMM of the most recent forward ran on — one per distinct source id instead of one per (id, position)
 * pair or packed position (the "id_qkv" option below); 0 when the forward did not take the lever.  (A getter of its own, as above.) */
int zett_id_qkv(const zett_hypernet* h, int64_t* out);

/* Per-launch record of the GEMMs of the most recent zett_forward ("time_gemm" on: durations from HIP events recorded on
 * the launch stream around every launch).  What bench.py prices its roofline on, launch class by launch class. */
typedef struct zett_gemm_record {
    int32_t m, n, k;
    int32_t variant;              /* tile kernel that ran: the "gemm_variant" numbering                          */
    int32_t epilogue;             /* bit 0 16-bit output, 1 fp32 output, 2 residual, 3 Rescaler, 4 LayerNorm-fold producer
                                     (16-bit copy + partial statistics), 5 LayerNorm-fold consumer, 6 residual read from the
                                     16-bit stream; bits 8-9 activation
                                     (0 none, 1 tanh-GELU, 2 erf-GELU); 10 zett_forward_into: the epilogue stores into
                                     the destination, 11 zett_forward_into: fp32 rows staged for the converting scatter */
    float ms;                     /* launch duration (0 when "time_gemm" is off)                                  */
    double flops;                 /* 2*m*n*k                                                                      */
    double bytes;                 /* algorithmic HBM bytes of the launch: A and W read once, every output written
                                     once, the residual rows read once                                            */
} zett_gemm_record;
/* Copies up to `capacity` records into `out` (may be NULL with capacity 0) and stores the number of launches in *count. */
int zett_get_gemm_log(const zett_hypernet* h, zett_gemm_record* out, int64_t capacity, int64_t* count);

/* Range guard of the 16-bit arithmetic modes.  ZETT_PREC_F16 operands overflow to inf above 65504; LayerNorm'd
 * activations and embedding-scale weights stay far inside, but with the LayerNorm fold the operand copy of the RAW
 * residual sum is rounded to half, and a checkpoint with massive activations can leave the range.  Nothing is silent:
 *   - zett_finalize returns ZETT_E_RANGE when a weight (or gamma-folded weight) does not fit the operand type;
 *   - every kernel that writes a 16-bit operand, and the epilogues that write the predicted embeddings, OR a bit of
 *     `zett_range_bits` into a device word that zett_forward clears when it starts.  An inf anywhere upstream reaches
 *     the outputs of its row (inf / NaN propagate through every residual add), so ZETT_RANGE_OUTPUT is the catch-all
 *     and the other bits say where it started;
 *   - zett_check_range waits for `stream`, reads the word of the most recent zett_forward on the handle and returns
 *     ZETT_E_RANGE if it is non-zero (0 otherwise); *flags (may be NULL) receives the word.  zett_forward itself does not
 *     wait for its kernels (see zett_forward_prepare for what it does wait for).  What to do on a hit is the caller's policy: the Python layer (zett_amd/hypernet.py)
 *     re-runs the call with bf16 operands (fp32's exponent range, same MFMA rate) and warns; a hit in BF16 / F32
 *     mode means the outputs are non-finite in the reference's own arithmetic too (non-finite inputs or weights).
 *     With zett_set_option("range_accumulate", 1) zett_forward no longer clears the word and zett_check_range clears it
 *     after reading: several asynchronous forwards, one question at the end (zett_amd/sharding.py, the CLI under torchrun).
 * The reference has no counterpart: its bf16 / fp32 arithmetic cannot leave the range short of inf in fp32. */
int zett_check_range(zett_hypernet* h, void* stream, int32_t* flags);

/* Completion of individual outputs inside a forward, for callers that start moving an output while the rest of the
 * forward still runs (the vocabulary-sharded path starts the all-gather of pred_in under the second head's GEMMs:
 * zett_amd/sharding.py).  zett_forward records an event on its stream when out_bias is complete (after the position-0
 * readout of the last encoder chunk) and when out_in is complete (after the first head's final GEMM of the last chunk);
 * out_out is complete when the forward is, i.e. in stream order.  zett_stream_wait_output makes `stream` (another
 * hipStream_t) wait for that point of the MOST RECENT zett_forward on the handle; it returns at once on the host.
 * The reference has no counterpart (its outputs appear together when XLA's executable returns). */
enum zett_output { ZETT_OUT_IN = 0, ZETT_OUT_BIAS = 1 };
int zett_stream_wait_output(zett_hypernet* h, int which, void* stream);

/* Upper bound of the device bytes zett_forward reserves (and keeps until zett_destroy)
 * for a [n_rows, seq] batch at the current options: the plan's worst case, no pad
 * position and every position a different source id.  The reference has no counterpart
 * (torch's caching allocator owns its activations); callers use it to size --batch_size
 * against free HBM before the first forward. */
int zett_workspace_bytes(const zett_hypernet* h, int64_t n_rows, int32_t seq, int64_t* out_bytes);

/* Options: "max_chunk_tokens" (packed positions per encoder chunk, >= 1024; default: 12 GiB of per-position
 * workspace, at least 131072 positions: 131072 at H = 4096, ~640 k at H = 768), "time_gemm" (0/1: bracket every
 * GEMM launch with HIP events on the launch stream and report the sum in
 * zett_stats.gemm_ms), "cls_only_last_layer" (0/1, default 1), "residual_lo" (0/1/2, default 1: with the LayerNorm fold on, the
 * encoder's hidden state travels as the 16-bit copy of its pre-LayerNorm sum only — the residual GEMMs read their residual rows
 * from it and write no fp32 sum; 1 = in F16 mode (the stream is rounded to 11 significand bits per layer: inside the f16
 * tolerance), 2 = in BF16 mode too (8 bits: outside the bf16 tolerance, A/B only), 0 = fp32 residual stream),
 * "concurrent_lanes" (0/1/2, default 0, A/B only: a call that is one chunk runs as two half-vocabulary chunks on two streams
 * at once — the caller's and one the handle owns, forked behind the hoisted table and joined before zett_forward's work on
 * `stream` ends — so that the partly filled last round of one chain's GEMMs can be filled by the other's; 1 = when the narrowest
 * launches would leave > 8 % of fewer than four CU-rounds idle, the pair lever is not taken and "time_gemm" is off, 2 = always.
 * Measured: 4 096-row shard of the 4096-wide hypernet (2.375 rounds) 8.85 -> 8.82 ms, every larger call slower: each 256x256
 * tile owns its CU, the dispatcher gains only the partial rounds.  Same bits),
 * "attention_fast" (0/1, default 1, A/B only: rows of at most 8 packed positions
 * take the attention kernel's register-resident path), "pair_dedupe" (0/1, default 1: layer 0's
 * Q/K/V once per distinct (source id, position) pair; same bits either way), "ln_fold" (0/1/2, default 1: in the 16-bit
 * modes the LayerNorms inside the encoder AND the ProjectorBlock LayerNorm in front of each output head's final Linear are
 * folded into the GEMMs around them instead of launched; 2 = the encoder's only (A/B); same values to the rounding of the
 * arithmetic, not the same bits; off whenever a tile variant is forced), "gemm_variant"
 * (0 = choose per launch, 1 = 128x128, 2 = 256x256 register-staged eight-wave,
 * 3 = 384x256 LDS-DMA, 7 = 256x256 four-wave direct-to-LDS (the choice for 16-bit
 * operands and K >= "gemm4d_min_k", default 512), 8 = as 7 with the generic epilogue drain; all produce
 * identical bits; a forced variant falls back to 2 where its preconditions do not
 * hold), "gemm_tile_order" (A/B only: 0 = the order in which gemm4d walks column
 * tiles first, default; 1 = row tiles first; same bits), "gemm_group" (A/B only: column — or, order 1, row — tiles per group of that
 * walk, 0 = the default of 4; same bits), "gemm_tail_split" (0/1/2/3, default 1: a 256x256-tile launch whose
 * tiles fill R whole rounds of the 256 CUs and part of one more is cut into 256x256 tiles on the rows of the whole rounds and
 * 128x256 tiles — twice as many workgroups of half the work — on the rest, when that is cheaper (a rank's 4 096-row shard at
 * 8 GPUs: M = 9 682, N = 4096 is 2.375 rounds); 0 = never, 2 = cut every launch in the middle, 3 = 128x256 tiles only (tests);
 * same bits), "table_lo" (0/1, default 1, round 6: with the 16-bit residual stream the hoisted input-projection table is kept as
 * the 16-bit copy of its pre-LayerNorm sum + (mean, rstd) per distinct id and normalised by the embeddings' kernel as it reads a
 * row; 0 = the fp32 table; one 16-bit rounding apart), "ln_rows8" (0/1, default 1, round 6: LayerNorm launches of the 16-bit
 * modes at hidden sizes of 256 k <= 1024 / 512 k <= 2048 give a lane eight columns and a row 32 / 64 lanes; 0 = the float4
 * kernel; the row sums are added in another order, results differ by rounding), "attention_pack" (0/1, default 1, round 6: a
 * last group of 256 / 128 / 64 hidden columns of the attention kernel — hidden size 768 — takes 2 / 4 / 8 rows per wave instead
 * of leaving lanes idle; same bits), "single_rows" (0/1/2, default 1: a vocabulary row with ONE kept position attends to exactly
 * one key — softmax weight exactly 1, context = its value row — so its query and key are never needed: such rows are put first
 * in the position-0 block of the hidden-state buffers and the Q|K launches of the layers behind the per-pair one skip them
 * with a pointer offset; the outputs are stored through the inverse row map; same bits.  1 = for a call that is one chunk on
 * one lane with seq + language token > 1, when floor(singles / 256) * (2 * hidden / 256) tiles fill at least one round of
 * the 256 CUs; 2 = for every such call with a single row; 0 = never.  Not taken: nothing differs, launch for launch),
 * "id_qkv" (0/1/2, default 1: layer 0's fused Q/K/V as ONE LayerNorm-fold GEMM over the distinct source ids' table rows, followed
 * by a row kernel that applies each position's additive term and the row's LayerNorm statistics — the position enters the
 * embeddings additively and the LayerNorm's centring is linear.  Possible with the folded 16-bit table, at least two encoder layers
 * and no language position; decided from the configuration and options alone, never from a call's counts, so every call shape of a
 * handle computes layer 0 the same way: 1 = when possible and hidden >= 4096, 2 = whenever possible, 0 = never.  Taken, the outputs
 * differ from "id_qkv" 0 by one 16-bit rounding placed elsewhere; zett_id_qkv reports it). */
int zett_set_option(zett_hypernet* h, const char* key, int64_t value);

/* ---- id-affinity row partition (ABI 6) ----------------------------------------------
 * Replaces: the ORDER in which the reference hands target-vocabulary rows to its devices — a random permutation cut into
 * device shards (scripts/transfer.py:54-67, 90-91; zett/utils.py:26).  Rows are independent, so which rank computes which row
 * is free; it decides how many DISTINCT source ids (hoisted input projection) and distinct (id, position) pairs (layer 0's
 * Q/K/V) a rank's shard holds.  zett_partition_rows assigns the n_rows rows of a device-resident surface-form matrix to
 * `world` <= 8 ranks with the given capacities (caps: host array, sum = n_rows) so that rows sharing ids share a rank, and
 * writes to perm_out (device, int32 [n_rows]) the row indices grouped by rank — rank r's rows at [sum(caps[:r]), + caps[r]),
 * ascending.  Deterministic: every rank runs it on the same matrix and gets the same permutation (no communication).  One
 * workgroup, ~2 us per 1024 rows, enqueued on `stream`; `workspace` = zett_partition_workspace_bytes(n_rows, n_ids) device
 * bytes, n_ids = the exclusive upper bound of the ids that count (original_vocab_size + n_extra; others and pad_id are ignored).
 * csrc/partition.hip.h has the algorithm. */
int zett_partition_workspace_bytes(int64_t n_rows, int32_t n_ids, int64_t* out_bytes);
int zett_partition_rows(const int32_t* surface_forms, int64_t n_rows, int32_t seq, int32_t pad_id, int32_t n_ids, int32_t world,
                        const int32_t* caps, int32_t* perm_out, void* workspace, int64_t workspace_bytes, int32_t device, void* stream);
/* dst[order[i]] = src[i] for i < n_rows, rows of row_bytes bytes (4, or a multiple of 16; device pointers; order: int64, < 0 =
 * skip): puts an exchanged block of predicted rows back into vocabulary order — the counterpart of the reference's
 * `preds[indices] += ...` scatter (scripts/transfer.py:96-111).  An HBM stream on `stream`. */
int zett_scatter_rows(const void* src, void* dst, const int64_t* order, int64_t n_rows, int64_t row_bytes, int32_t device, void* stream);

/* ---- the hoisted table shared between ranks (ABI 8) ---------------------------------------
 * Replaces: nothing the reference has — it is SURVEY.md 8e's optional second exchange of the row-sharded prediction
 * (scripts/transfer.py:90-91, zett/utils.py:26): input_projection(in_scaler(source_embeddings[id])) depends on the source id
 * only, so instead of every rank computing it for the distinct ids of ITS rows (8 340 of the 29 187 ids of the whole vocabulary on
 * each of 8 ranks of the headline workload: 2.3 x the work in all), the ranks agree on the distinct ids of the WHOLE vocabulary,
 * each computes 1/P of the table, and the slices are exchanged (the folded 16-bit table: 2 bytes per element + 8 per row).  A table
 * row's bits do not depend on which rank or tile computed it, so the predicted matrices are those of zett_forward bit for bit.
 * f16 arithmetic with the LayerNorm fold, the 16-bit residual stream and "table_lo" on (the defaults); ZETT_E_INVALID otherwise.
 *
 * zett_table_plan: the distinct source ids a forward over `surface_forms` [n_rows, seq] (device int32: every rank passes the WHOLE
 * vocabulary's matrix) would reference, in ascending id order: id_list_out (device int32, capacity original_vocab_size +
 * n_extra) receives them, id_slot_out (device int32 [original_vocab_size + n_extra + 1]) the table slot of every id (exclusive
 * scan of the reference flags), *n_ids_out their number.  Waits for `stream` (one host round trip); ZETT_E_INDEX on an id outside
 * the vocabulary, as zett_forward.
 * zett_table_rows: table rows [first, first + count) of that list — gather + in_scaler + fallback, input_projection.0, the
 * ProjectorBlock up to its pre-LayerNorm sum — into table_out (rows of `hidden` values of the handle's 16-bit type; the buffer
 * holds the WHOLE table, row i at table_out + i * hidden) and stats_out (float [*, 2]: mean, rstd of row i at stats_out + 2 i).
 * Asynchronous on `stream`.  Overflows of the 16-bit type are OR-ed into the handle's range word (zett_check_range), which the next
 * forward clears unless "range_accumulate" is on: ask after building the table, not after the forwards on it.  Whether the handle
 * builds table rows at all (precision, fold, "table_lo") is decided BEFORE the empty slice: a call with count == 0 gives that
 * ZETT_E_INVALID too, so that ranks with and without rows of a small table agree; behind that check count == 0 returns ZETT_OK
 * without reading a pointer, so `zett_table_rows(h, NULL, 0, 0, NULL, ZETT_F32, 0, NULL, NULL, NULL)` is the probe "does this handle
 * have the folded table".
 * zett_forward_table: zett_forward on that table (complete: this rank's rows and its peers') instead of source embeddings.  Every
 * id the call references (position 0, visible positions, every position of a row without a visible key) must own a row of the
 * table, i.e. id_slot[id + 1] != id_slot[id]: id_slot is an exclusive scan, so an id the planned matrix never referenced carries its
 * successor's slot.  Otherwise ZETT_E_INDEX ("... not in the table", with the number of the last offending row; an id outside
 * the vocabulary is reported first, with zett_forward's message), at the plan's host read: no output or destination row is written. */
int zett_table_plan(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq, int32_t* id_slot_out, int32_t* id_list_out,
                    int64_t* n_ids_out, void* stream);
int zett_table_rows(zett_hypernet* h, const int32_t* id_list, int64_t first, int64_t count, const void* source_embeddings, int src_dtype,
                    int64_t v_src, void* table_out, float* stats_out, void* stream);
int zett_forward_table(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq, const void* table, const float* table_stats,
                       const int32_t* id_slot, int32_t lang_index, float* out_in, float* out_out, float* out_bias, void* stream);
/* zett_forward_table storing into a destination (additive, ABI 8): see zett_forward_into */
int zett_forward_table_into(zett_hypernet* h, const int32_t* surface_forms, int64_t n_rows, int32_t seq, const void* table,
                            const float* table_stats, const int32_t* id_slot, int32_t lang_index, const zett_dest* dest, void* stream);

/* ---- retokenizer ------------------------------------------------------------
 * Replaces: zett.utils.get_surface_form_matrix (zett/utils.py:651-689) and the
 * tokenizers-library Model.tokenize it calls per token (zett/utils.py:681): BPE, Unigram and WordPiece models. */

enum zett_retok_kind { ZETT_RETOK_BPE = 0, ZETT_RETOK_UNIGRAM = 1, ZETT_RETOK_WORDPIECE = 2 };

/* Host-side description of the hn tokenizer's bare model.  Pieces are given as RAW
 * BYTES (byte-level token strings already mapped through the reference's
 * CHARS_TO_BYTES table, zett/utils.py:351-609); pieces that contain a character
 * outside that table can never match a byte-level token and must be omitted. */
typedef struct zett_retok_model {
    int32_t kind;                  /* zett_retok_kind                              */
    int32_t n_pieces;
    const uint8_t* piece_bytes;    /* host: concatenated piece bytes               */
    const int32_t* piece_offsets;  /* host: n_pieces + 1                           */
    const int32_t* piece_ids;      /* host: vocabulary id of each piece            */
    const double* piece_scores;    /* host: Unigram log-probs (NULL for BPE)       */
    double unigram_min_score;      /* Unigram: min score over the WHOLE vocabulary (also pieces
                                      omitted above); unknown pieces score min - 10 */
    int32_t n_merges;              /* BPE                                          */
    const int32_t* merges;         /* host: n_merges x 3 (left id, right id, new id), rank = row */
    int32_t unk_id;                /* -1 = none                                    */
    int32_t fuse_unk;              /* BPE fuse_unk (Unigram always fuses)          */
    int32_t byte_fallback;         /* BPE/Unigram byte_fallback                    */
    const int32_t* byte_fallback_ids; /* host: 256 ids of "<0xXX>" tokens, -1 = absent (may be NULL) */
    int32_t ignore_merges;         /* BPE ignore_merges                            */
    int32_t n_special;
    const uint8_t* special_bytes;  /* host: hn tokenizer all_special_tokens, raw bytes */
    const int32_t* special_offsets;/* host: n_special + 1                          */
    const int32_t* special_ids;    /* host                                          */
    /* WordPiece (tokenizers WordPiece::tokenize; zett/tokenizer_converters.py:370-373 carries such hn tokenizers through).
     * A lookup at the start of a word matches a vocabulary entry as listed; a lookup further in matches
     * continuing_subword_prefix + substring.  The caller lists every entry once as it is (piece_continuing 0) and every
     * entry that starts with the prefix once more with the prefix stripped (piece_continuing 1) — with the empty prefix
     * that convert_to_byte_level leaves, each entry twice.  unk_id = id of unk_token, -1 when it is not in the vocabulary
     * (a word that needs it then fails the call with ZETT_E_STATE, as the library raises). */
    const uint8_t* piece_continuing;   /* host: n_pieces flags (may be NULL: no continuing pieces); WordPiece only */
    int32_t max_input_chars_per_word;  /* WordPiece: longer words are [UNK] (library default 100)                  */
} zett_retok_model;

int zett_retok_create(const zett_retok_model* model, int device, zett_retok** out);
int zett_retok_destroy(zett_retok* r);
/* A/B switches of a retokenizer handle (as zett_set_option for the forward): "unigram_workgroup" — which stage-2 kernel Unigram
 * models run: the workgroup-per-64-tokens kernel (all piece lookups of 64 tokens in flight at once, then the Viterbi walk on
 * LDS) or the lane-per-token kernel every model kind used before.  1 (default) = by size (the workgroup kernel for calls of up to
 * 32 768 tokens), 2 = always the workgroup kernel, 0 = never.  Same ids either way (tests/test_retok_gpu.py).  Unknown key:
 * ZETT_E_INVALID.  No counterpart in the reference (tokenizers' Unigram::tokenize has one code path). */
int zett_retok_set_option(zett_retok* r, const char* key, int64_t value);

/* get_surface_form_matrix(tokens, maxlen, tokenizer_to_use)
 *   token_chars   device: UTF-8 text of the byte-level target tokens, concatenated
 *   offsets       device: int32 [n_tokens + 1] byte offsets into token_chars
 *   out           device: int32 [n_tokens, maxlen], pre-filled here with pad_id
 *   n_truncated   host out: number of tokens cut to maxlen
 * The byte-table lookup (CHARS_TO_BYTES) runs on the device; a character outside
 * the table returns ZETT_E_KEY with the offending token index in *bad_token
 * (reference: KeyError at zett/utils.py:675). */
int zett_retokenize(zett_retok* r, const uint8_t* token_chars, const int32_t* offsets,
                    int64_t n_tokens, int32_t maxlen, int32_t pad_id, int32_t* out,
                    int64_t* n_truncated, int64_t* bad_token, void* stream);

/* The same without the two host round trips of zett_retokenize (which reads the text length, offsets[n_tokens], back before it
 * launches, and the counts after): the caller passes n_text — it built the text — and the call returns as soon as its six
 * kernels are enqueued on `stream`.  Counts and errors are collected by zett_retok_result, ONCE for all asynchronous calls
 * since the previous query: it waits for the last of them, sums their truncated tokens into *n_truncated, and on a failure
 * returns what zett_retokenize would (ZETT_E_KEY / ZETT_E_STATE) for the EARLIEST failing call, whose ordinal since the
 * previous query goes to *bad_call and whose token index to *bad_token (both nullable; -1 when nothing failed).  The id
 * matrices of the calls before the failing one are complete.  A synchronous zett_retokenize in between discards what the
 * asynchronous calls before it reported; at most 2^20 calls may be outstanding between two queries (ZETT_E_STATE beyond).
 * offsets == NULL (ABI 6): token_chars holds the n_tokens tokens NUL-SEPARATED (n_text bytes, n_tokens - 1 of them NUL — exactly
 * what "\0".join(tokens).encode() gives; no byte-level token holds a NUL, byte 0 being written U+0100): the token boundaries
 * are found on the device by the scan that numbers the characters, so the host does no per-token work at all.  A text with
 * another number of separators is reported as ZETT_E_INVALID by zett_retok_result.
 * LIFETIME: `offsets` of every outstanding call must stay allocated and unchanged until zett_retok_result returns — on a
 * ZETT_E_KEY it is read back to name the failing token (zett_amd.surface_forms.DeviceRetokenizer holds the tensors).  A call
 * that fails while it enqueues is taken back (it does not count as outstanding).  The reference has no counterpart (its loop is host code). */
int zett_retokenize_async(zett_retok* r, const uint8_t* token_chars, const int32_t* offsets, int64_t n_tokens, int64_t n_text,
                          int32_t maxlen, int32_t pad_id, int32_t* out, void* stream);
int zett_retok_result(zett_retok* r, int64_t* n_truncated, int64_t* bad_call, int64_t* bad_token);

/* ---- lexical (FVT / BFVT) embedding transfer (additive, ABI 8) ------------------------------------------------------------
 * Replaces: the per-token loop of the reference's lexical baseline (scripts/transfer_lexical.py:50-91): for every target token
 * the row of the same string in the source vocabulary, else the mean of the source rows of its decomposition under the source
 * tokenizer's bare model, else a fallback row.  S = the source matrix of R rows (R is the MATRIX's row count, not the
 * tokenizer's length: the two differ in both directions in practice).
 *
 * THE MEAN: add the rows in `ids` order in fp32, then one IEEE (correctly rounded) division by float(n); n = 1 is a plain copy.
 * Every row of the reference's output with n <= 16 constituents has exactly these bits (torch's CPU mean(0) adds in order up to
 * there; beyond, its sum cascades in blocks and the reference's bits are another rounding of the same sum). */
enum zett_lexical_mode { ZETT_LEXICAL_NO = 0, ZETT_LEXICAL_FVT = 1, ZETT_LEXICAL_BFVT = 2 };      /* fvt_mode "no" / "fvt" / "bfvt" */

/* The lexicon of a source tokenizer (transfer_lexical.py:27-34, 65, 77): `model` is its bare model as for zett_retok_create; its
 * n_special / special_* fields are IGNORED — the decomposition never matches special tokens by string (a special token whose id
 * is >= R is tokenized by the reference like any other text).  vocab_*: the WHOLE source_tokenizer.get_vocab() dictionary, added
 * and special tokens included, as raw bytes / offsets [n_vocab + 1] / ids (host arrays, the layout of the pieces; entries with
 * a character outside the byte table can never equal a byte-level token and must be omitted).  It becomes an exact-match table
 * on the device (the retokenizer's whole-token table: open addressing, load <= 1/8). */
int zett_lexical_create(const zett_retok_model* model, int32_t n_vocab, const uint8_t* vocab_bytes, const int32_t* vocab_offsets,
                        const int32_t* vocab_ids, int device, zett_lexical** out);
int zett_lexical_destroy(zett_lexical* h);

/* transfer_lexical.py:65-86 without the arithmetic: for each of the n_tokens target tokens (token_chars: NUL-separated byte-level
 * text of n_text bytes, as zett_retokenize_async with offsets == NULL; boundaries found on the device) what its row is a mean of.
 *   ids    device int32 [n_tokens, width]; count device int32 [n_tokens]
 *   exact match (get_vocab().get(t) exists and is < n_source_rows, :65-67): count = 1, ids[i, 0] = that id;
 *   else, unless fvt_mode is NO, the ids of model.tokenize(t) (:77), filtered against n_source_rows — FVT (:78-81): any id >=
 *   n_source_rows, or no id at all, gives count = 0; BFVT (:82-86): such ids are removed and the others close up in order;
 *   count = 0 means "fallback row".  The empty token has count = 0.
 * count[i] is the TRUE number of ids even when it exceeds `width` (then only the first `width` are stored; ids[i, count[i]:] is
 * unspecified otherwise): *n_wide receives the number of such rows, which the caller plans again at the width they need, so no
 * decomposition is ever cut.  *n_overlap = rows with count > 0 (the reference's "Overlapping tokens", :88-91), *n_ids = the
 * sum of the counts; all three reduced on the device, all nullable.  Waits for `stream`.
 * A character outside the byte table: ZETT_E_KEY with the token index in *bad_token, as zett_retokenize (the reference would
 * hand such a string to the model as it is: a deliberate deviation).  A token that needs an unk id the model lacks:
 * ZETT_E_STATE, where tokenizers raises. */
int zett_lexical_plan(zett_lexical* h, const uint8_t* token_chars, int64_t n_tokens, int64_t n_text, int64_t n_source_rows, int32_t fvt_mode,
                      int32_t width, int32_t* ids, int32_t* count, int64_t* n_overlap, int64_t* n_wide, int64_t* n_ids, int64_t* bad_token,
                      void* stream);

/* transfer_lexical.py:50-63, 67, 81, 86, 93-103 (the arithmetic): destination row dest->rows[i] (< 0: skipped; NULL: i) =
 * the mean (above) of source rows ids[i, :count[i]]; count[i] == 0: source row fallback_id (fallback_mode "unk": the source
 * tokenizer's unk_token_id), or with fallback_id == -1 the row is left untouched (fallback_mode "random": the caller has put its
 * draws there).  The reference's cat([in, out], dim=1) is never materialised: src_in [R, >= ld_src_in] feeds dest->in, src_out
 * (NULL iff dest->out is NULL: tied embeddings) feeds dest->out, n_embd columns each, src_dtype F32 / F16 / BF16 upcast to fp32 on
 * load.  Stored as zett_forward_into stores: the fp32 value bit for bit in an fp32 destination, round-to-nearest-even in a 16-bit
 * one.  dest->bias must be NULL.  Nothing is trusted: every id in use is checked against n_source_rows and every dest->rows[i]
 * against dest->n_dest_rows on the device through an error word — ZETT_E_INDEX BEFORE anything is written (one host round trip on
 * `stream`); a count outside [0, width] (a row that was not planned again) is ZETT_E_INVALID.  The stores are asynchronous on `stream`. */
int zett_lexical_rows_into(zett_lexical* h, const int32_t* ids, const int32_t* count, int64_t n_tokens, int32_t width, const void* src_in,
                           int64_t ld_src_in, const void* src_out, int64_t ld_src_out, int32_t src_dtype, int64_t n_source_rows, int32_t n_embd,
                           int64_t fallback_id, const zett_dest* dest, void* stream);

/* ---- training use of the forward ---------------------------------------------------------
 * Replaces: the hypernetwork forward inside the loss of the reference's train_step / eval_step (train.py:1007-1013,
 * 1191-1197: state.apply_fn({"params": params["hypernet"]}, target_surface_forms, target_priors, source_embeddings,
 * lang_index) under jax.value_and_grad) — i.e. the same forward, differentiable with respect to every hypernetwork
 * parameter.  First slice: fp32 arithmetic in the reference's as-written dense [N, L', H] layout.  The primitives below
 * are what zett_amd/autograd.py (a torch.autograd.Function: torch holds the tensors and the tape, nothing else) builds
 * the forward that keeps its activations and the backward from.  All pointers are device pointers, fp32, row-major;
 * `stream` is a hipStream_t.  Dense contractions — forward, dgrad, wgrad — are ONE entry point on the library's TN
 * GEMM family (fp32 MFMA): dgrad is the same contraction against the transposed weight, wgrad the same contraction of
 * the two transposed activations (zett_op_transpose_f32 zero-pads the row count to the 32-wide K step).
 * One unit per family under zett_amd/csrc/, each with its kernels, its launch and its entry points: train_gemm.hip (the
 * contractions), train_operands.hip (conversions, transposes, sums, element-wise forms, the GELUs), train_layernorm.hip,
 * train_attention.hip, train_gather.hip (indexed rows, the source-embedding gather). */
/* out[m, n] = act(a[m, :] . w[n, :] + bias[n]) + residual[m, n]   (bias, residual nullable; act: 0 none, 1 tanh-GELU, 2 erf-GELU;
 * k % 32 == 0, lda / ldw % 4 == 0)
 * Pointers (this entry point and zett_op_gemm_lo): every tile fetches the operands as 16-byte pieces of a row, so `a` and `w` must be
 * 16-byte aligned (with the leading dimensions above, every row then is); bias, residual and out are fp32 and must be 4-byte
 * aligned.  Anything else is ZETT_E_INVALID before any launch.  ld_out and ld_res may be any value >= n.  The 256x256 tiles move
 * bias, residual and out as float4: they are taken for m > 128 and n > 128 when n % 8 == 0, ld_out % 4 == 0, ld_res % 4 == 0 and
 * out, residual and bias are 16-byte aligned; every other call runs on the 128x128 tile, which reads and writes them one float at
 * a time.  The choice does not change a bit of the result. */
int zett_op_gemm_f32(const float* a, int32_t lda, const float* w, int32_t ldw, int64_t m, int32_t n, int32_t k, const float* bias, int32_t act,
                     const float* residual, int32_t ld_res, float* out, int32_t ld_out, void* stream);
/* The same contraction on 16-bit MFMA operands (prec = ZETT_PREC_BF16 | ZETT_PREC_F16), fp32 accumulate, fp32 epilogue and output
 * (k % 64 == 0, lda / ldw % 8 == 0; pointer alignment as above): the tile kernels of the inference path.  Operands are made by zett_op_convert_lo
 * (out[r, c] = lo(in[r, c]), columns zero-padded to cols_padded) and zett_op_transpose_lo (out[c, r] = lo(in[r, c]), rows
 * zero-padded to rows_padded): the conversion is fused with the layout change dgrad / wgrad need anyway. */
int zett_op_gemm_lo(int32_t prec, const void* a, int32_t lda, const void* w, int32_t ldw, int64_t m, int32_t n, int32_t k, const float* bias, int32_t act,
                    const float* residual, int32_t ld_res, float* out, int32_t ld_out, void* stream);
/* Alignment of the conversions and 16-bit transposes: `in` of zett_op_transpose_lo / zett_op_grad_operands_lo (and act_z) 16-byte aligned,
 * 16-bit buffers (out, dy_lo, dy_t, a 16-bit `in`) 8-byte aligned, or ZETT_E_INVALID; zett_op_convert_lo takes any pointer.  Leading
 * dimensions may be any value >= the width (ld_out >= rows_padded / cols_padded): multiples of 4 elements move four values per access, any
 * other value one value at a time, with the same bits.  zett_op_transpose_f32 has no alignment requirement. */
int zett_op_convert_lo(int32_t prec, const float* in, int32_t ld_in, void* out, int32_t ld_out, int64_t rows, int32_t cols, int32_t cols_padded, void* stream);
int zett_op_transpose_lo(int32_t prec, const float* in, int32_t ld_in, void* out, int32_t ld_out, int64_t rows, int32_t cols, int64_t rows_padded, void* stream);
/* The transposed operand of an activation that is already stored as a 16-bit operand of type prec (no conversion). */
int zett_op_transpose_lo16(int32_t prec, const void* in, int32_t ld_in, void* out, int32_t ld_out, int64_t rows, int32_t cols, int64_t rows_padded, void* stream);
/* Everything a Linear's backward needs from its output gradient dy [rows, cols], in one read: dy_lo = lo(dy) (dgrad's A operand),
 * dy_t [cols, rows_padded] = lo(dy)^T (wgrad's A operand, rows zero-padded), colsum_part [ceil(rows / 64), cols] = the column sums
 * of each 64-row band (their sum over the bands is the bias gradient).  act_z (nullable): the Linear's output went through a GELU
 * (act_kind 1 tanh, 2 erf) and dy is the gradient of the GELU's OUTPUT: dy * gelu'(act_z) is formed on the fly and used for
 * all three results (the activation's backward costs no pass of its own). */
int zett_op_grad_operands_lo(int32_t prec, const float* dy, int32_t ld, const float* act_z, int32_t ld_z, int32_t act_kind, int64_t rows, int32_t cols,
                             int64_t rows_padded, void* dy_lo, int32_t ld_lo, void* dy_t, int32_t ld_t, float* colsum_part, void* stream);
/* out[c, r] = in[r, c] (r < rows), 0 for rows <= r < rows_padded */
int zett_op_transpose_f32(const float* in, int32_t ld_in, float* out, int32_t ld_out, int64_t rows, int32_t cols, int64_t rows_padded, void* stream);
/* out[c] (+)= sum_r in[r, c] */
int zett_op_colsum_f32(const float* in, int32_t ld, int64_t rows, int32_t cols, float* out, int32_t accumulate, void* stream);
/* op 0: a + b; 1: a * b; 2: a * vec[col] + vec2[col] (vec NULL: 1, vec2 NULL: 0); 3: a + s[row] * vec[col]; 4: a * s[row] (a NULL: s[row] * vec[col]).
 * a, b, out are [n / cols, cols] without padding; any 4-byte aligned pointers (16-byte aligned with cols % 4 == 0: four values per access, same bits).
 * The GELU entry points below likewise. */
int zett_op_elementwise_f32(int32_t op, const float* a, const float* b, const float* vec, const float* vec2, const float* s, float* out,
                            int64_t n, int32_t cols, void* stream);
/* out[r] = a[r, :] . w + b[0] (b nullable) */
int zett_op_rowdot_f32(const float* a, int32_t ld, const float* w, const float* b, float* out, int64_t rows, int32_t cols, void* stream);
/* y = LayerNorm(x) (two-pass variance); stats[r] = (mean, rstd); y_lo (nullable, type prec): the same values as the 16-bit
 * operand of the next contraction.  4 <= h <= 8192, h % 4 == 0.  x has leading dimension ld (ld % 4 == 0: x may be a column slice of a
 * wider matrix); y, y_lo (and dy, dy2, dx of the backward) have leading dimension h.  x, gamma, beta, y 16-byte aligned, y_lo 8-byte. */
int zett_op_layernorm_fwd_f32(const float* x, int32_t ld, const float* gamma, const float* beta, float eps, float* y, float* stats,
                              int64_t rows, int32_t h, void* y_lo, int32_t prec, void* stream);
/* dx for the gradient dy (+ dy2, nullable: the part arriving over the residual branch), and the parameter gradients as
 * n_part partial sums: partials [n_part, 2, h] — partials[:, 0].sum(0) = dgamma, partials[:, 1].sum(0) = dbeta (workgroup b
 * walks rows b, b + n_part, ...: deterministic for a given n_part; any n_part >= 1, a workgroup without rows writes zeros).
 * 4 <= h <= 8192, h % 4 == 0; dy, dy2, x, gamma, dx and partials 16-byte aligned. */
int zett_op_layernorm_bwd_f32(const float* dy, const float* dy2, const float* x, int32_t ld, const float* stats, const float* gamma, float* dx,
                              float* partials, int32_t n_part, int64_t rows, int32_t h, void* stream);
int zett_op_gelu_fwd_f32(const float* z, float* h, int64_t n, int32_t kind, void* stream);
int zett_op_gelu_bwd_f32(const float* z, const float* dh, float* dz, int64_t n, int32_t kind, void* stream);
/* h_lo = lo(gelu(z)): the activation as the next contraction's 16-bit operand (its fp32 value is never stored) */
int zett_op_gelu_fwd_lo(int32_t prec, const float* z, void* h_lo, int64_t n, int32_t kind, void* stream);
/* softmax(q k^T / sqrt(d) + finfo.min * !mask) v per vocabulary row and head (eager semantics: a row whose keys are all
 * masked attends uniformly).  The positions of row n are rows [row_offset[n], row_offset[n+1]) of k / v (packed: only the
 * positions the row keeps) or [n*seq, (n+1)*seq) when row_offset is NULL (the reference's dense layout); at most seq <= 32
 * positions per row; mask[t] = position t is visible as a key.  cls_only: one query per row (position 0), q and ctx hold
 * one row per vocabulary row (the position-0-only last layer).  probs [n_rows, heads, seq, seq] is kept for the backward: of a row with
 * L positions only the [L, L] block (cls_only: its first line) is written and read, the rest of the buffer is unspecified; a masked key
 * holds exactly 0 unless every key of the row is masked.  ld_ctx, ld_dq, ld_d may be any value >= heads * head_dim; no alignment beyond
 * the element's.
 * ctx_lo (nullable, type prec, same leading dimension): the context is written as the 16-bit operand of the contraction behind it
 * INSTEAD of fp32 (ctx may then be NULL).
 * Head dims up to 256 (the backward: above 128 for rows of up to 16 positions — the row's keys, values and their gradients
 * live in registers). */
int zett_op_attention_fwd_f32(const float* q, int32_t ldq, const float* k, const float* v, int32_t ld, const uint8_t* mask, const int32_t* row_offset,
                              int64_t n_rows, int32_t seq, int32_t heads, int32_t head_dim, int32_t cls_only, float* ctx, int32_t ld_ctx, float* probs,
                              void* ctx_lo, int32_t prec, void* stream);
int zett_op_attention_bwd_f32(const float* dctx, int32_t ld_ctx, const float* q, int32_t ldq, const float* k, const float* v, int32_t ld, const float* probs,
                              const int32_t* row_offset, int64_t n_rows, int32_t seq, int32_t heads, int32_t head_dim, int32_t cls_only, float* dq, int32_t ld_dq,
                              float* dk, float* dv, int32_t ld_d, void* stream);
/* out[r, :] = a[r, :] + src[idx[r], :] (a NULL: 0);   dst[idx[r], :] += src[r, :] (float atomics: a sum in NO fixed order, a row hit three
 * or more times can differ in its last bits from run to run).  a, out and scatter's src are [rows, cols] without padding. */
int zett_op_gather_rows_f32(const float* a, const float* src, int32_t ld_src, const int32_t* idx, float* out, int64_t rows, int32_t cols, void* stream);
int zett_op_scatter_add_rows_f32(float* dst, int32_t ld_dst, const int32_t* idx, const float* src, int64_t rows, int32_t cols, void* stream);
/* A2 + A3 (modeling_hypernet.py:170-188) per position (ids < v0: source rows, v0 <= id < v0 + fallback rows: fallback[id - v0]; sw NULL: no
 * rescaler, sb is then not read), and its backward: dfallback accumulated in place with float atomics (zero it first; like
 * zett_op_scatter_add_rows_f32 a sum in no fixed order),
 * prod = dx * source row and keep = dx on source rows (0 on fallback rows): their column sums are d in_scaler.w / d in_scaler.b */
int zett_op_gather_fwd_f32(const int32_t* ids, int64_t n_tokens, const void* src, int32_t src_dtype, int32_t e_in, int32_t v0, const float* fallback,
                           const float* sw, const float* sb, float* x, void* stream);
int zett_op_gather_bwd_f32(const int32_t* ids, int64_t n_tokens, const void* src, int32_t src_dtype, int32_t e_in, int32_t v0, const float* dx,
                           float* dfallback, float* prod, float* keep, void* stream);
/* The order-stable form of the gather's backward (ZettHypernet.train_deterministic): prod and keep exactly as zett_op_gather_bwd_f32
 * writes them — the same kernel with the fallback branch compiled out, the same bits for fp32 / f16 / bf16 sources — and NO fallback sum:
 * no dfallback argument, no atomic.  d fallback is then zett_op_embed_lookup_bwd(g = dx) over the plan
 * zett_op_embed_lookup_plan_base(ids, id_base = v0, v = fallback rows), i.e. per fallback row the sum that entry point defines
 * (ascending positions, fp32 partials of ZETT_EMBED_BWD_CHUNK positions added left to right, the partials added in ascending chunk
 * order, a row with no position zeros).  A null pointer, an unknown dtype, n_tokens < 0, e_in <= 0 or v0 < 0: ZETT_E_INVALID. */
int zett_op_gather_bwd_rows_f32(const int32_t* ids, int64_t n_tokens, const void* src, int32_t src_dtype, int32_t e_in, int32_t v0, const float* dx, float* prod,
                                float* keep, void* stream);

/* ---- the forward's row kernels, one launch at a time (csrc/rowops_entry.hip; additive, the ABI version does not move) -------------
 * Everything in the inference forward that is not a GEMM, callable on its own so that one launch can be checked element by element
 * (tests/test_rowops_direct_gpu.py).  Each call goes through the launcher the forward itself calls (csrc/rowops_launch.hip.h): the
 * kernel, lanes per row, grid and flags are the forward's for the same width and options.  Raw device pointers, asynchronous on
 * `stream`, nothing is allocated, every argument is validated before any launch (ZETT_E_INVALID with a zett_last_error text).
 * prec is a zett_precision: the operand type T of out_lo / q / k / v / ctx / tables (float with ZETT_PREC_F32).  Common rules: widths
 * are multiples of 8, base pointers 16-byte aligned, leading dimensions multiples of 8 and at least the width; a row count of 0
 * launches nothing. */
enum zett_ln_kernel {            /* what *kernel_id receives: the kernel a LayerNorm launch went to */
    ZETT_LN_ROWS8_32 = 0,        /* eight columns per lane, 32 lanes per row (16-bit modes, ln_rows8, h % 256 == 0, h <= 1024) */
    ZETT_LN_ROWS8_64 = 1,        /* eight columns per lane, 64 lanes per row (16-bit modes, ln_rows8, h % 512 == 0, h <= 2048) */
    ZETT_LN_WAVE = 2,            /* float4 per lane, one wave per row (h <= 2048) */
    ZETT_LN_WORKGROUP = 3        /* float4 per lane, one workgroup per row; rows wider than 8192 are read three times */
};
/* LayerNorm over h of rows [rows, ld_in]: fp32 `in`, or 16-bit `in_lo` (readout only, not with ZETT_PREC_F32).  Outputs, each nullable:
 * out_f32 [rows, h], out_lo [rows, h] of T, stats [rows, 2] = (mean, rstd).  out_bias != NULL selects the readout instantiations:
 * bias[r] = sum_c y[r, c] bias_w[c] + bias_b[0] (bias_w NULL: exactly 0); bias_dtype -1: out_bias is float [rows]; a zett_dtype: out_bias
 * is the caller's destination of that type and row r goes to element bias_rows[r] (< 0: not written; NULL: r); a finite bias that
 * becomes inf in an f16 destination ORs ZETT_RANGE_DEST's bit (16) into *range_flag (nullable). */
int zett_op_fwd_layernorm(int32_t prec, const float* in, const void* in_lo, int32_t ld_in, int32_t rows, int32_t h, const float* gamma, const float* beta,
                          float eps, int32_t ln_rows8, float* out_f32, void* out_lo, float* stats, const float* bias_w, const float* bias_b, void* out_bias,
                          const int64_t* bias_rows, int32_t bias_dtype, int32_t* range_flag, int32_t* kernel_id, void* stream);
/* The embeddings' LayerNorm over packed positions [tok0, tok0 + m): x = table[tok_slot] (fp32 `table`, or — not with ZETT_PREC_F32 — the
 * 16-bit table_lo normalised on the fly with table_stats (mean, rstd per table row), table_gamma, table_beta), or, tok_slot < 0,
 * lang - (type0 + pos_emb[lang_pos]); sum = (x + type0) + pos_emb[tok_pos]; out_lo / stats = LayerNorm(sum).  tok_row != NULL: the
 * position goes to its buffer row of the chunk (row0, rows, row_offset; position 0 of a vocabulary row first); NULL: written in place
 * (row t - tok0).  out_lo, stats, sum: each nullable. */
int zett_op_fwd_embed_layernorm(int32_t prec, const float* table, const void* table_lo, const float* table_stats, const float* table_gamma, const float* table_beta,
                                const int32_t* tok_slot, const int32_t* tok_pos, const float* type0, const float* pos_emb, const float* lang, int32_t lang_pos,
                                const int32_t* tok_row, const int32_t* row_offset, int64_t row0, int32_t rows, int32_t tok0, int32_t m, int32_t h, const float* gamma,
                                const float* beta, float eps, int32_t ln_rows8, void* out_lo, float* stats, float* sum, int32_t* kernel_id, void* stream);
/* attention_rows_kernel over vocabulary rows [row0, row0 + rows) = packed positions from tok0: q / k / v / ctx are BUFFER rows of
 * the chunk (position 0 first), or — tok_pair != NULL — q / k / v are indexed by pair slot.  flags: bit 0 cls_only (q [rows, ldq],
 * ctx [rows, h]), bit 1 the fast path for rows of at most 8 positions (16-bit), bit 2 pack a narrow last column group.  head_dim: a
 * power of two in [8, 512] that divides h. */
int zett_op_fwd_attention(int32_t prec, const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, int32_t h, int32_t head_dim,
                          const int32_t* row_offset, const uint8_t* row_uniform, const uint8_t* tok_key, int64_t row0, int32_t rows, int32_t tok0, float scaling,
                          int32_t flags, const int32_t* tok_pair, void* ctx, void* stream);
/* out[s] (T, [n_slots, e_in]) = id < v0 ? sc_w * src[id] + sc_b : fallback[id - v0], id = id_list[slot0 + s] (sc_w NULL: no rescaler).
 * A value beyond the f16 range (or NaN) ORs ZETT_RANGE_SOURCE's bit (1) into *range_flag (nullable), with ZETT_PREC_F16 only. */
int zett_op_fwd_gather_src(int32_t prec, const int32_t* id_list, int32_t slot0, int32_t n_slots, const void* src, int32_t src_dtype, int32_t e_in, int32_t v0,
                           const float* fallback, const float* sc_w, const float* sc_b, void* out, int32_t* range_flag, void* stream);
/* stats[r] = (mean, rstd) from the h / 128 partials (sum, sum of squares) of row r: parts is float2 [h / 128, ld_part], added in order;
 * var = max(q / h - mean^2, 0).  prec is checked and otherwise unused. */
int zett_op_fwd_ln_stats(int32_t prec, const float* parts, int32_t ld_part, int32_t rows, int32_t h, float eps, float* stats, void* stream);
/* w_fold[n, k] = T(w[n, k] * gamma[k]), c_out[n] = sum_k w_fold[n, k], b_out[n] = bias[n] + sum_k w[n, k] beta[k] (16-bit T only).  A
 * product beyond the f16 range ORs ZETT_RANGE_WEIGHT's bit (8) into *range_flag (nullable). */
int zett_op_fwd_fold_weight(int32_t prec, const float* w, int32_t n, int32_t k, const float* gamma, const float* beta, const float* bias, void* w_fold,
                            float* c_out, float* b_out, int32_t* range_flag, void* stream);
/* Layer 0's [q | k | v] rows from the id-level product U (lever 6, "id_qkv"; 16-bit T only):
 *   out[row, col] = T( fma(r_x, (U[slot, col] + c_pos[pos, col]) - mu_x * c_w[col], b_q[col]) ),  (mu_x, r_x) = stats[row],
 * in exactly this order of fp32 operations.  u is [*, n_cols] of T, c_pos float [n_pos, n_cols] (every pos < n_pos), c_w / b_q float
 * [n_cols].  Output row j of n: tok_row NULL: slot[t0 + j], pos[t0 + j], stats and out row j (pair rows); tok_row != NULL: packed
 * position t0 + j goes to its buffer row of the chunk (row0, rows, row_offset, cls_slot; position 0 of a vocabulary row first), where
 * its statistics lie too.  |value| beyond the f16 range (or NaN) ORs ZETT_RANGE_ACTIVATION's bit (2) into *range_flag (nullable),
 * with ZETT_PREC_F16 only. */
int zett_op_fwd_pair_qkv(int32_t prec, const void* u, const int32_t* slot, const int32_t* pos, int32_t t0, int32_t n, const int32_t* tok_row,
                         const int32_t* row_offset, int64_t row0, int32_t rows, const int32_t* cls_slot, const float* stats, const float* c_pos, int32_t n_pos,
                         const float* c_w, const float* b_q, int32_t n_cols, void* out, int64_t ld_out, int32_t* range_flag, void* stream);

/* ---- one GEMM launch of the forward (csrc/gemm_entry.hip; additive, the ABI version does not move) ------------------------------
 * C[m, n] = epilogue(a[m, k] . w[n, k]^T) exactly as the forward launches it: the tile variant and gemm4d's tail cut come from the rule
 * the forward's own launches use (csrc/gemm_launch.hip.h gemm_variant_for / gemm_row0_for), the kernel from launch_gemm_variant, so
 * that ONE launch with any epilogue can be checked element by element (tests/test_gemm_fwd_direct_gpu.py).  The descriptor mirrors
 * GemmArgs / GemmEpilogue of csrc/gemm.hip.h field for field (T = the operand type of prec; every pointer a raw device pointer,
 * nullable unless noted; leading dimensions in elements):
 *   v = acc + bias[col]  (fold_stats: acc <- rstd_row * (acc - mean_row * fold_c[col]) first);  v = act(v);  v += r[row, col];
 *   v = scale[col] * v + shift[col];   r = residual (fp32) or residual_lo (T) at row res_index[row] (NULL: row), with res_stats
 *   LayerNorm'd on the fly: ((r - mean) * rstd) * res_gamma[col] + res_beta[col], (mean, rstd) = res_stats[2 * that row ..];
 *   columns < split_col -> out_f32 / out_lo, columns >= split_col -> out_f32_b (split_col <= 0 or >= n: no split);
 *   dst: row m goes to row dst_rows[m] (NULL: m; < 0: not written) of the caller's matrix of zett_dtype dst_dtype, instead of out_f32;
 *   stats_part [n / 128][ld_part] float2: (sum, sum of squares) of v over each 128-column slice of a row (LayerNorm-fold producer);
 *   range_flag: where the range guard ORs its zett_range_bits; range_final: the fp32 outputs are checked for inf / NaN.
 * The entry validates everything before any launch, allocates nothing and is asynchronous on `stream`; a refusal is ZETT_E_INVALID with
 * a zett_last_error text: an unknown precision / act / dst_dtype / option value, k not a positive multiple of 128 bytes, lda / ldw
 * below k or rows that are not multiples of 16 bytes, base pointers that are not 16-byte aligned (statistics and partials 8, index
 * arrays and range_flag their element size, dst what its type's four-value store needs), a leading dimension below its width, no output,
 * 16-bit features (stats_part, fold_stats, residual_lo, dst) with ZETT_PREC_F32, res_stats without gamma / beta or a residual,
 * residual with residual_lo, scale without shift, fold_stats without fold_c, a LayerNorm-fold or destination launch no gemm4d
 * instantiation carries, dst together with another output.  res_index and dst_rows are trusted, as in the forward.  The 384-row tile
 * (variant 3) does not clamp rows: it runs only when a_rows_readable >= ceil(m / 384) * 384, otherwise the launch takes variant 2.
 * m == 0 or n == 0 launches nothing.  *variant_out (nullable): the tile variant that ran (1, 2, 3, 7, 8; -1: nothing launched);
 * *mode_out (nullable): for variants 7 / 8 the epilogue instantiation (0 generic, 1 LO, 2 F32, 3 F32_SCALE, 4 BOTH, 5 F32_LN,
 * 6 LO_FOLD, 7 LO_LN, 8 F32_SCALE_FOLD, 9 LN16: G4D_EPI_* of csrc/gemm4d.hip.h), -1 otherwise. */
typedef struct zett_fwd_gemm_desc {
    int64_t size;                     /* sizeof(zett_fwd_gemm_desc): any other value is refused */
    const void* a; const void* w;     /* T [m, lda], T [n, ldw]; required */
    const float* bias;                /* [n] */
    const float* residual;            /* [*, ld_res] */
    const void* residual_lo;          /* T [*, ld_res_lo]: the 16-bit residual stream (with stats_part only) */
    const float* res_stats;           /* [*, 2] */
    const float* res_gamma; const float* res_beta;      /* [n] */
    const int32_t* res_index;         /* [m] */
    float* stats_part;                /* float2 [n / 128][ld_part] */
    const float* fold_stats;          /* [m, 2] (mean, rstd) of the A rows */
    const float* fold_c;              /* [n] */
    const float* scale; const float* shift;             /* [n] */
    float* out_f32; void* out_lo; float* out_f32_b;
    int32_t* range_flag;
    void* dst; const int64_t* dst_rows;
    int64_t ld_dst;
    int64_t a_rows_readable;          /* rows of `a` that may be read (>= m) */
    int32_t lda, ldw, m, n, k, act;   /* act: 0 none, 1 tanh-GELU, 2 erf-GELU */
    int32_t ld_res, ld_res_lo, ld_part, ld_f32, ld_lo, split_col;
    int32_t range_final, dst_dtype;
    /* the options Runner::gemm reads from the handle (zett_set_option names and ranges) */
    int32_t gemm_variant, gemm4d_min_k, gemm_tail_split, gemm_tile_order, gemm_group;
    int32_t reserved;                 /* 0 */
} zett_fwd_gemm_desc;
int zett_op_fwd_gemm(int32_t prec, const zett_fwd_gemm_desc* desc, int32_t* variant_out, int32_t* mode_out, void* stream);

/* ---- the losses and the parameter update of a training step (zett_amd/training.py) ----------------------------------------------
 * What the reference's trainer puts around the hypernetwork forward: the squared-error loss of the identity warm-up
 * (identity_train_step, train.py:914-975), the lexical loss (train.py:1074-1141) and optax.chain(clip_by_global_norm,
 * multi_transform({train: adamw, freeze: set_to_zero})) (train.py:591-656).  All pointers are device pointers unless said
 * otherwise; everything is asynchronous on `stream` and none of these calls waits for the host.  Every reduction is per-workgroup partials
 * summed in a fixed order (no float atomics): the same inputs give the same bits on every run. */
enum zett_distance { ZETT_DIST_MSE = 0, ZETT_DIST_RMSE = 1, ZETT_DIST_HUBER = 2 };      /* lexical_loss_kind, train.py:1096-1115 */
enum zett_loss_mode { ZETT_LOSS_MEAN = 0, ZETT_LOSS_LEXICAL = 1 };
enum zett_adamw_flags { ZETT_ADAMW_DECAY = 1, ZETT_ADAMW_FROZEN = 2 };
#define ZETT_MT_CHUNK 65536      /* elements per work item of the multi-tensor kernels: zett_op_grad_norm needs one float of `partials`
                                    per started chunk of every tensor */
/* mask[r] = 1.0 where ids[r, 1:] are all pad_token_id, else 0.0 (lexical_overlap_mask, train.py:1092-1094).  ids is int32
 * (ids_bytes 4) or int64 (8), [n, width] with leading dimension ld. */
int zett_op_single_token_mask(const void* ids, int32_t ids_bytes, int64_t n, int32_t width, int64_t ld, int64_t pad_token_id, float* mask, void* stream);
/* Rows pass of an embedding distance.  The target of row r is src[clamp(ids[r * ids_stride], 0, src_rows - 1), col0 : col0 + e]
 * (src: zett_dtype src_dtype, leading dimension ld_src; the clamp is JAX's gather rule for train.py:941 / 1086).
 * row_dist[r] = distance(pred[r], target) * mask[r] (mask NULL: 1), row_tnorm[r] = ||target||_2.  kind: ZETT_DIST_MSE sum (x-y)^2
 * (train.py:943-944, 1099), ZETT_DIST_RMSE ||x-y||_2 (:1104), ZETT_DIST_HUBER sum huber(x-y; 1e-3) / 1e-3 / 30 (:1107-1115). */
int zett_op_embed_dist_rows(const float* pred, int64_t ld_pred, const void* src, int32_t src_dtype, int64_t ld_src, int64_t src_rows, int32_t col0, const void* ids,
                            int32_t ids_bytes, int64_t ids_stride, const float* mask, int64_t n, int32_t e, int32_t kind, float* row_dist, float* row_tnorm,
                            void* stream);
/* record[0..3] = { loss, gradient scale, sum(mask) / n, 0 }.  ZETT_LOSS_MEAN: loss = sum(row_dist) / n (train.py:942-946);
 * ZETT_LOSS_LEXICAL: loss = sum(row_dist) / (sum(mask) + 1e-8) / mean(row_tnorm), the mean over ALL rows (train.py:1121-1125;
 * 1e-8 is EPSILON of zett/utils.py).  The gradient scale is d loss / d sum(row_dist). */
int zett_op_embed_dist_finalize(const float* row_dist, const float* row_tnorm, const float* mask, int64_t n, int32_t mode, float* record, void* stream);
/* dpred[r, :] = (accumulate ? dpred[r, :] : 0) + upstream[0] * record[1] * mask[r] * d distance / d pred[r, :] — what
 * jax.value_and_grad (train.py:964) yields for these terms.  row_dist and record are the outputs of the two calls above;
 * upstream is a device scalar.  ZETT_DIST_RMSE at distance 0: gradient 0 (the reference's is NaN there). */
int zett_op_embed_dist_grad(const float* pred, int64_t ld_pred, const void* src, int32_t src_dtype, int64_t ld_src, int64_t src_rows, int32_t col0, const void* ids,
                            int32_t ids_bytes, int64_t ids_stride, const float* mask, const float* row_dist, int64_t n, int32_t e, int32_t kind, const float* record,
                            const float* upstream, float* dpred, int64_t ld_dpred, int32_t accumulate, void* stream);
/* optax.clip_by_global_norm (train.py:653-654) over n_tensors fp32 tensors.  grads / numel are HOST arrays of device pointers and
 * element counts: they travel to the kernels as launch arguments, so the caller's arrays are free again when the call returns.
 * record (8 words, zeroed once by the caller and then owned by these two calls):
 *   [0] norm  [1] coef = 1 if norm < max_norm else max_norm / norm  [2] int32 skip = the norm is not finite
 *   [3] int32 step count, advanced unless skip  [4] 1 - b1^step  [5] 1 - b2^step. */
int zett_op_grad_norm(const void* const* grads, const int64_t* numel, int32_t n_tensors, double max_norm, double b1, double b2, float* partials,
                      int64_t partials_capacity, float* record, void* stream);
/* optax.adamw with a decay mask inside multi_transform (train.py:638-650), one pass over all tensors:
 *   g' = coef g;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= lr ((m / c1) / (sqrt(v / c2) + eps) + decay ? weight_decay p : 0)
 * coef, c1, c2 and skip come from `record` (zett_op_grad_norm); with skip set no parameter and no moment is written.  flags[i]:
 * ZETT_ADAMW_DECAY, ZETT_ADAMW_FROZEN (set_to_zero: the tensor is left alone; params / moments may be NULL).  zero_grad: gradients are
 * zeroed in the same pass — those of frozen tensors and, on a skipped step, all of them too, so that a non-finite gradient does not
 * stay behind for the next backward to accumulate into.  The pointer and count arrays are HOST arrays, as above.  Any element count and any 4-byte-aligned pointer. */
int zett_op_adamw(void* const* params, void* const* grads, void* const* exp_avg, void* const* exp_avg_sq, const int64_t* numel, const uint8_t* flags, int32_t n_tensors,
                  double lr, double b1, double b2, double eps, double weight_decay, int32_t zero_grad, const float* record, void* stream);
/* The other branch of the reference's optimizer (train.py:631-656, use_adafactor): optax.chain(clip_by_global_norm(max_norm),
 * multi_transform({train: optax.adafactor(lr, weight_decay_rate, weight_decay_mask), freeze: set_to_zero})) with every other argument of
 * optax.adafactor (optax/_src/alias.py, adafactor) at its default: scale_by_factored_rms(factored, decay_rate 0.8, step offset 0,
 * min_dim_size_to_factor 128, eps 1e-30), clip_by_block_rms(1.0), scale_by_learning_rate, scale_by_param_block_rms (eps 1e-3),
 * add_decayed_weights, no momentum (optax/_src/factorized.py scale_by_factored_rms; clipping.py clip_by_block_rms; transform.py
 * scale_by_param_block_rms, add_decayed_weights).  Tensor i is [rows[i], cols[i]] fp32, contiguous (1-D: rows 1); flags[i] as for
 * zett_op_adamw.  With t = record[3], the updates applied so far:
 *   norm, coef, skip: as zett_op_grad_norm, over every tensor of the list, frozen ones included;  g' = coef g;  q = g'^2 + 1e-30
 *   beta = 1 - (t + 1)^-0.8 (float64 power, rounded to fp32 once)
 *   FACTORED, not frozen and min(rows, cols) >= 128: with d0 the larger and d1 the smaller dimension by numpy.argsort(shape) (a square
 *     matrix: d1 = 0, d0 = 1), v_row[shape[d1]] = beta v_row + (1 - beta) mean(q, axis d0), v_col[shape[d0]] = beta v_col + (1 - beta)
 *     mean(q, axis d1), u = g' (v_row / mean(v_row))^-1/2 (along d0) v_col^-1/2 (along d1);  v[i] is not read
 *   every other tensor that is not frozen: v[rows, cols] = beta v + (1 - beta) q, u = g' v^-1/2;  v_row[i], v_col[i] are not read
 *   s = max(sqrt(mean p^2), 1e-3) of the parameter before the update;  p -= lr s u / max(1, sqrt(mean u^2)) + (decay ? weight_decay p : 0)
 *     — the decay is NOT multiplied by lr: optax adds the decayed weights after the learning-rate scaling.
 * record: 8 words as zett_op_grad_norm's, [4] beta, [5] 1 - beta.  A norm that is not finite sets skip: no parameter, no statistic and
 * not the count is written.  zero_grad: as zett_op_adamw.  A frozen tensor needs its gradient only.  The arrays are HOST arrays; the
 * workspace is device memory, 16-byte aligned, of at least zett_op_adafactor_workspace_floats floats, free again when the stream has
 * run the call.  A factored tensor is worked on in tiles of ZETT_ADAFACTOR_TILE_ROWS x ZETT_ADAFACTOR_TILE_COLS, the others in chunks of
 * ZETT_MT_CHUNK, ZETT_ADAFACTOR_GROUP tensors per launch; every sum is taken in a fixed order (csrc/train_adafactor.hip states it). */
#define ZETT_ADAFACTOR_TILE_ROWS 64
#define ZETT_ADAFACTOR_TILE_COLS 256
#define ZETT_ADAFACTOR_GROUP 40
int zett_op_adafactor_workspace_floats(const int64_t* rows, const int64_t* cols, const uint8_t* flags, int32_t n_tensors, int64_t* floats);
int zett_op_adafactor_step(void* const* params, void* const* grads, void* const* v_row, void* const* v_col, void* const* v, const int64_t* rows, const int64_t* cols,
                           const uint8_t* flags, int32_t n_tensors, double lr, double weight_decay, double max_norm, int32_t zero_grad, float* workspace,
                           int64_t workspace_floats, float* record, void* stream);

/* ---- the language-model loss over predicted output embeddings (zett_amd/training.py lm_head_loss) --------------------------------
 * train_step / eval_step of the reference (train.py:1039-1056, 874-912, 1226-1255):
 *     logits = hidden . pred_out^T + where(vocab_mask, 0, -100000) + bias + priors           [T, V]
 *     loss   = sum_t w_t (logsumexp(logits[t]) - logits[t, label_t]) / sum_t w_t
 * The contractions are zett_op_gemm_lo / zett_op_gemm_f32 (the column addend enters through the bias epilogue); the calls below
 * are the kernels between them (csrc/train_loss.hip).  Asynchronous on `stream`, no float atomics, nothing waits for the host. */
enum zett_ce_path { ZETT_CE_AUTO = 0, ZETT_CE_ONCE = 1, ZETT_CE_TWICE = 2 };
#define ZETT_CE_ONCE_MAX_COLS 32768      /* the longest (padded) row the rows pass reads once and keeps in registers */
/* out[c] = (vocab_mask ? (vocab_mask[c] ? 0 : -100000) : 0) + bias[c] + priors[c] for c < v, 0 for v <= c < v_padded (all three
 * nullable; vocab_mask: one byte per column, nonzero = the column is in the vocabulary). */
int zett_op_ce_addend(const float* bias, const float* priors, const uint8_t* vocab_mask, int32_t v, int32_t v_padded, float* out, void* stream);
/* Softmax cross-entropy rows pass over fp32 logits [rows, v] (leading dimension ld_z >= v_padded, rows 16-byte aligned).  Per row t:
 *   argmax[t] = the FIRST maximum (jnp.argmax);  lse[t] = max + log sum exp(z - max);  row_loss[t] = w_t (lse[t] - z[label_t]).
 * A label outside [0, v) is an all-zero one-hot (jax.nn.one_hot; -100 included): row_loss = w_t lse, and the label is never an
 * index.  weight NULL: 1.  A row with w_t == 0 has row_loss 0 whatever its label.
 * g (nullable; zett_dtype g_dtype, leading dimension ld_g >= v_padded): the gradient operand
 *   g[t, c] = w_t (exp(z[t, c] - lse[t]) - [c == label_t]),  0 for v <= c < v_padded,  all zero for w_t == 0,
 * NOT scaled by 1 / sum(w) or an upstream gradient (zett_op_ce_scale applies both to the fp32 results of the contractions).  An
 * fp32 g may be the logits themselves (ld_g == ld_z).  v_padded % 4 == 0.
 * path: ZETT_CE_ONCE reads a row once and keeps it in registers (v_padded <= ZETT_CE_ONCE_MAX_COLS), ZETT_CE_TWICE reads it
 * twice (any v), ZETT_CE_AUTO takes the first where it applies.  Both give the same bits. */
int zett_op_ce_rows(float* logits, int64_t ld_z, const int32_t* labels, const float* weight, int64_t rows, int32_t v, int32_t v_padded, void* g, int32_t g_dtype,
                    int64_t ld_g, float* row_loss, float* lse, int32_t* argmax, int32_t path, void* stream);
/* record (8 words) = { loss = sum(row_loss) / sum(w), sum(w), 1 / sum(w), int32 n_correct, int32 n_counted, 0, 0, 0 } over all n
 * rows: n_counted = rows with w > 0, n_correct = those whose argmax equals their label.  sum(w) == 0: loss 0 and 1 / sum(w) = 0,
 * so every gradient is 0 (the reference's are NaN). */
int zett_op_ce_finalize(const float* row_loss, const float* weight, const int32_t* labels, const int32_t* argmax, int64_t n, float* record, void* stream);
/* out[c] = (accumulate ? out[c] : 0) + sum_t g[t, c], c < v: the (unscaled) bias gradient */
int zett_op_ce_colsum(const void* g, int32_t g_dtype, int64_t ld_g, int64_t rows, int32_t v, float* out, int32_t accumulate, void* stream);
/* out[i] = (out_dtype) (in[i] * upstream[0] * record[2]): an unscaled gradient times upstream / sum(w), both read on the device */
int zett_op_ce_scale(const float* in, int64_t n, const float* record, const float* upstream, void* out, int32_t out_dtype, void* stream);
/* out[r, c] = (out_dtype) in[r, c] for c < cols, 0 for cols <= c < cols_padded (zett_dtype both): an operand of the contractions */
int zett_op_ce_cast(const void* in, int32_t in_dtype, int64_t ld_in, void* out, int32_t out_dtype, int64_t ld_out, int64_t rows, int32_t cols, int32_t cols_padded,
                    void* stream);

/* ---- the input side of a training step (zett_amd/training.py splice_special_rows, token_embeddings) ------------------------------
 * train_step of the reference (train.py:998-1037): the special rows of the predicted matrices are overwritten with source rows, and
 * the backbone looks input_ids up in the spliced input matrix; the backward of that lookup is where pred_in gets its gradient.
 * The calls below are csrc/train_embed.hip.  Asynchronous on `stream`, nothing waits for the host, no float atomics: the same
 * inputs give the same bits on every run. */
#define ZETT_SPLICE_MAX_ROWS 256       /* the longest splice list: the lists travel as kernel arguments (tokenizer.all_special_ids is far shorter) */
#define ZETT_EMBED_BWD_CHUNK 64        /* positions of one partial sum of the lookup's backward: part of the definition of the result */
/* out[rows[i], 0:e] = (float) src[ref_rows[i], col0 : col0 + e] for i < n (src: zett_dtype src_dtype, leading dimension ld_src,
 * src_rows rows; src NULL: the listed rows become 0 and ref_rows is not read).  in != NULL: every other row of out [v, e] is a copy
 * of in's, in ONE pass over the matrix; in NULL: no other row of out is touched.  rows / ref_rows are HOST arrays, validated before
 * any launch: a row outside [0, v) or a source row outside [0, src_rows) is ZETT_E_INDEX, a row listed twice or more than
 * ZETT_SPLICE_MAX_ROWS rows ZETT_E_INVALID.  They travel to the kernel as launch arguments, so the caller's arrays are free again
 * when the call returns.  Any e and any 4-byte aligned pointers; 16-byte accesses where pointers and leading dimensions allow them. */
int zett_op_splice_rows(const float* in, int64_t ld_in, float* out, int64_t ld_out, int64_t v, int32_t e, const void* src, int32_t src_dtype, int64_t ld_src,
                        int64_t src_rows, int32_t col0, const int32_t* rows, const int32_t* ref_rows, int32_t n, void* stream);
/* out[p, 0:e] = (out_dtype) table[ids[p], 0:e] for p < t (zett_dtype both; out contiguous [t, e]; ids int32 (ids_bytes 4) or int64
 * (8)).  fp32 -> 16 bits rounds to nearest even, equal types copy the bits.  An id outside [0, v) gives a zero row, is never used as
 * an address, and ORs 1 into *error_word (device, nullable, zeroed by the caller). */
int zett_op_embed_lookup(const void* table, int32_t table_dtype, int64_t ld_table, int64_t v, int32_t e, const void* ids, int32_t ids_bytes, int64_t t, void* out,
                         int32_t out_dtype, int32_t* error_word, void* stream);
/* bytes of the plan of t positions over v rows (what the backward reads: keep it until then), of the scratch buffer that only the plan
 * call itself uses (free once that call's work on the stream is done), and of the partial-sum rows the backward needs for e columns */
int zett_op_embed_lookup_workspace_bytes(int64_t t, int64_t v, int32_t e, int64_t* plan_bytes, int64_t* scratch_bytes, int64_t* partial_bytes);
/* The inverted index of ids: per id in [0, v) its positions in ASCENDING order, and the chunk table of the ids that hold more than
 * ZETT_EMBED_BWD_CHUNK positions.  Ids outside [0, v) are in no list.  Integers only (a histogram, a scan, a placement that depends
 * on tile indices and counts alone): the plan is a pure function of ids.  `plan`, `scratch`: device, 4-byte aligned, sizes as queried. */
int zett_op_embed_lookup_plan(const void* ids, int32_t ids_bytes, int64_t t, int64_t v, void* plan, int64_t plan_bytes, void* scratch, int64_t scratch_bytes,
                              void* stream);
/* The same plan over SHIFTED ids: the inverted index of ids[p] - id_base over [0, v) — row r lists the positions that hold the id
 * id_base + r, ascending; an id outside [id_base, id_base + v) is in no list.  The same kernels with one more integer argument;
 * zett_op_embed_lookup_plan is the id_base = 0 case and writes the same plan words as ever.  Sizes as queried for (t, v).  With
 * zett_op_embed_lookup_bwd this is "sum the rows of g that share an index" for any index array, in the order defined there: the
 * fallback rows of the hypernetwork take ids in [v0, v0 + F) to rows [0, F) with id_base = v0.  id_base and id_base + v must be
 * 32-bit values (rows are indexed with 32 bits): otherwise ZETT_E_INVALID, as for ids_bytes outside {4, 8}, t < 0, v <= 0, a null,
 * misaligned or too small plan or scratch.  Everything is checked before the first launch. */
int zett_op_embed_lookup_plan_base(const void* ids, int32_t ids_bytes, int64_t t, int64_t id_base, int64_t v, void* plan, int64_t plan_bytes, void* scratch,
                                   int64_t scratch_bytes, void* stream);
/* d_table[id, 0:e] for EVERY id in [0, v), each row written exactly once (no memset, no read-modify-write): with p_0 < p_1 < ... the
 * positions of id and C = ZETT_EMBED_BWD_CHUNK,
 *     partial_j = ((g[p_jC] + g[p_jC+1]) + ...) + g[p_jC+C-1]        fp32, ascending positions, the last chunk ragged
 *     d_table[id] = ((partial_0 + partial_1) + ...) + partial_last   fp32, ascending chunks; no position: zeros
 * g: [t, e] contiguous, zett_dtype g_dtype, converted exactly to fp32.  plan: what the plan call wrote for the same t and v. */
int zett_op_embed_lookup_bwd(const void* g, int32_t g_dtype, int64_t t, int64_t v, int32_t e, const void* plan, int64_t plan_bytes, float* partials,
                             int64_t partial_bytes, float* d_table, int64_t ld_d, void* stream);

/* ---- the batch's sub-vocabulary (zett_amd/training.py subsample_batch_vocabulary) --------------------------------------------------
 * The n_token_subsample branch of the reference's collator (collator.py:207-282) on arrays that are already on the device
 * (csrc/train_batch.hip).  With S = special_ids in the given order and N = n:
 *   positives       = ascending, the ids of [0, v) that occur in input_ids or in labels != -100 and are not in S
 *   tokens_in_batch = S ++ positives;   *n_positive = their number (> n: ZETT_BATCH_OVERFLOW)
 *   negatives       = n - *n_positive ids: ZETT_BATCH_POSITIVES_ONLY: id 0 repeated;  ZETT_BATCH_RANDOM: the first entries of
 *                     negative_order (a permutation of [0, v)) that are not in tokens_in_batch, in negative_order's order
 *   ids_to_embed    = tokens_in_batch ++ negatives, then move m = 0 .. n_special - 1 in turn: the row move_from[m] is taken out and
 *                     inserted at row move_to[m] (Python's del / insert; the collator's "for special in sorted(all_special_ids)" loop —
 *                     the moves depend on special_ids and n alone and are computed by the caller)
 *   inv[id]         = the LARGEST row r with ids_to_embed[r] == id
 *   out_input_ids   = inv[input_ids];   out_labels = labels == -100 ? -100 : inv[labels]
 *   out_surface_forms[r, 0:l] = surface_forms[ids_to_embed[r], 0:l];  out_priors[r] = priors[ids_to_embed[r]];  mask[r] = 1
 * input_ids / labels: t elements of ids_bytes / labels_bytes (4 or 8), the outputs have the widths of their inputs and ids_to_embed
 * that of input_ids; surface_forms: [v, l] of sf_bytes (4 or 8) with leading dimension ld_sf >= l elements, out_surface_forms [n, l]
 * contiguous; negative_order: v elements of order_bytes, read in ZETT_BATCH_RANDOM only.  special_ids / move_from / move_to are
 * HOST arrays of n_special <= ZETT_SPLICE_MAX_ROWS entries (distinct ids of [0, v), rows of [0, n)), validated before any launch;
 * they travel to the kernels as launch arguments.
 * *status (device) is written by the call: an OR of zett_batch_status bits, 0 when all is well.  With a bit set the outputs are
 * unspecified, but every write stays inside the output buffers and no id outside [0, v) is ever used as an address.
 * Integers only; the only atomics are integer OR and max, so the same inputs give the same bits.  Asynchronous on `stream`, no
 * allocation: `workspace` (device, 4-byte aligned, zett_op_batch_vocab_workspace_bytes) is free once the call's work is done. */
enum zett_batch_mode { ZETT_BATCH_POSITIVES_ONLY = 0, ZETT_BATCH_RANDOM = 1 };
enum zett_batch_status {
    ZETT_BATCH_BAD_ID = 1,         /* an id of input_ids / labels (other than a label of -100) is outside [0, v) */
    ZETT_BATCH_OVERFLOW = 2,       /* *n_positive > n */
    ZETT_BATCH_BAD_ORDER = 4,      /* an entry of negative_order is outside [0, v) */
    ZETT_BATCH_REPEAT = 8          /* ZETT_BATCH_RANDOM: an id is listed twice (inv saw a previous owner), or negative_order holds fewer
                                    * absent ids than rows to fill: negative_order is not a permutation */
};
int zett_op_batch_vocab_workspace_bytes(int64_t t, int64_t v, int64_t n, int64_t* bytes);
int zett_op_batch_vocab(const void* input_ids, int32_t ids_bytes, const void* labels, int32_t labels_bytes, int64_t t, int64_t v, int64_t n, const void* surface_forms,
                        int32_t sf_bytes, int64_t ld_sf, int32_t l, const float* priors, const void* negative_order, int32_t order_bytes, int32_t mode,
                        const int32_t* special_ids, const int32_t* move_from, const int32_t* move_to, int32_t n_special, void* out_input_ids, void* out_labels,
                        void* ids_to_embed, void* out_surface_forms, float* out_priors, uint8_t* mask, int32_t* n_positive, int32_t* status, void* workspace,
                        int64_t workspace_bytes, void* stream);

/* ---- labelling a batch (zett_amd/collate.py label_batch; additive, ABI 8) --------------------------------------------------------------
 * What the reference's Collator.encode does between the tokenizer call and the vocabulary (collator.py:180-205): the inner collator
 * (MLM: the arithmetic of transformers' DataCollatorForLanguageModeling.numpy_mask_tokens; CLM: labels = input_ids), then byte_lengths
 * and the two metrics, taken on the ids AFTER masking (csrc/train_batch.hip).  input_ids: [b, s] of ids_bytes (4 or 8) with leading
 * dimension ld_in >= s; position p = row * s + column is the logical index whatever ld_in is.  "special" = the id is one of special_ids
 * (HOST array, n_special <= ZETT_SPLICE_MAX_ROWS ids of [0, v)).  byte_lengths_per_token: v elements of table_bytes (4 or 8).
 * ZETT_LABEL_MLM, with mix64 the finalizer of splitmix64 and all arithmetic mod 2^64:
 *   key_i  = mix64(seed + (i + 1) * 0x9E3779B97F4A7C15)   i = 0 .. 3;     h_i(p) = mix64(key_i ^ p);     k_i(p) = h_i(p) >> 11   (53 bits)
 *   masked   = not special and k_0 < t_mask;   replaced = masked and k_1 < t_replace;   random = masked, not replaced and k_2 < t_random
 *   labels   = masked ? id : -100;   out_input_ids = replaced ? mask_token_id : random ? h_3(p) mod vocab_len : id
 * A threshold is ceil(probability * 2^53), so that k < t <=> k * 2^-53 < probability; at most 2^53.  1 <= vocab_len <= v.
 * ZETT_LABEL_CLM: labels = out_input_ids = input_ids; thresholds, seed and mask_token_id are not read.
 *   byte_lengths[p] = byte_lengths_per_token[out_input_ids[p]]     int64, [b, s] contiguous, like labels (width of input_ids)
 *   record   = { t, n_non_special, byte_sum_non_special, n_unk, n_masked, n_replaced, n_random, status }   8 int64 on the device;
 *              non-special and unk (out_input_ids == unk_token_id; -1: none) are counted on out_input_ids
 *   metrics  = { byte_sum_non_special / n_non_special, n_unk / t }   2 doubles on the device: quotients of exact integers, numpy's
 *              mean bit for bit; 0 / 0 is NaN
 * out_input_ids ([b, s], leading dimension ld_out >= s) may be input_ids itself.  An id outside [0, v) sets ZETT_LABEL_BAD_ID in
 * status; it is never used as an address, is never masked, counts as non-special and has byte length 0.  Integers only, added in a
 * fixed order (lanes, waves, workgroups): the same inputs give the same bits.  Positions and ids are indexed with 32 bits: b, b * s and v
 * above 0x7fffff00 are ZETT_E_INVALID.  Two launches on `stream`, no allocation, no host read;
 * `workspace`: ZETT_LABEL_WORKSPACE_BYTES on the device, 8-byte aligned, free once the call's work is done. */
#define ZETT_LABEL_WORKSPACE_BYTES 16384
enum zett_label_mode { ZETT_LABEL_CLM = 0, ZETT_LABEL_MLM = 1 };
enum zett_label_status { ZETT_LABEL_BAD_ID = 1 };
int zett_op_label_batch(const void* input_ids, int32_t ids_bytes, int64_t ld_in, int64_t b, int32_t s, const int32_t* special_ids, int32_t n_special,
                        const void* byte_lengths_per_token, int32_t table_bytes, int64_t v, int64_t vocab_len, int64_t mask_token_id, int64_t unk_token_id, int32_t mode,
                        uint64_t t_mask, uint64_t t_replace, uint64_t t_random, uint64_t seed, void* out_input_ids, int64_t ld_out, void* labels, int64_t* byte_lengths,
                        int64_t* record, double* metrics, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- the padded vocabulary (zett_amd/collate.py pad_vocabulary; additive, ABI 8) ----------------------------------------------------------
 * The branch of Collator.encode without n_token_subsample (collator.py:283-337): the whole vocabulary, padded to r >= v rows.
 *   out_surface_forms[i, 0:l] = i < v ? surface_forms[i, 0:l] : 0        [r, l] contiguous, sf_bytes (4 or 8) like the input (ld_sf >= l)
 *   out_priors[i] = i < v ? (float)priors[i] : -100000                   priors: v elements of priors_bytes (4: float, 8: double, rounded
 *                                                                        once to nearest even)
 *   mask[i] = i < v;     ids_to_embed[i] = i < v ? i : 0                 (int64)
 * Limits, ZETT_E_INVALID beyond them: 0 < l <= 65536 columns, r <= 0x7fffff00 rows.  One launch on `stream`; nothing is read back. */
int zett_op_pad_vocabulary(const void* surface_forms, int32_t sf_bytes, int64_t ld_sf, int32_t l, int64_t v, int64_t r, const void* priors, int32_t priors_bytes,
                           void* out_surface_forms, float* out_priors, uint8_t* mask, int64_t* ids_to_embed, void* stream);

/* ---- text encoding (zett_amd/text_encode.py DeviceTextEncoder, training.encode_texts; additive, ABI 8) ----------------------------
 * The tokenizer call of the reference's Collator.encode (collator.py:166-175: tokenizer(texts, max_length=block_size, truncation=True,
 * padding="max_length", add_special_tokens=True)) and its special_ids_map patch (collator.py:177-178), on UTF-8 text that is already on
 * the device (csrc/text_encode.hip).  `r` holds the tokenizer's bare model (BPE or Unigram; WordPiece is ZETT_E_NOT_IMPLEMENTED).
 *   text          n_text bytes: the UTF-8 of the n_texts texts back to back;  text_offsets: DEVICE, n_texts + 1 int64, non-decreasing from 0
 *                 to n_text (anything else sets ZETT_ENCODE_BAD_OFFSETS; every offset is clamped before it is used)
 *   prefix        zett_encode_prefix: a U+0020 in front of a NON-EMPTY text — always (normalizers.Prepend(" ")), or unless the text
 *                 starts with one (pre_tokenizers.ByteLevel(add_prefix_space=True)).  An empty text gets none in any mode.
 *   words         the leftmost-first matches of 's|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+ (zett/utils.py:29;
 *                 with ZETT_ENCODE_MARKS_ARE_LETTERS the letter class is [\p{L}\p{M}]), per text.  class_table: DEVICE, 4 bits per code
 *                 point (code point c in bits 4 * (c & 1) .. of byte c >> 1), n_code_points <= 0x110000 of them: 0 other, 1 \p{L},
 *                 2 \p{M}, 3 \p{N}, 4 \s; a code point beyond the table and a byte sequence that is not UTF-8 are class 0.
 *   ids of a word what stage 2 of zett_retokenize gives for the word's bytes as raw bytes (no special-token lookup)
 *   row           prefix_ids ++ the text's ids cut to block_size - n_prefix - n_suffix from the right ++ suffix_ids ++ pad_id ...;
 *                 attention_mask 1 on everything but the pads; then for m = 0 .. n_map - 1 in turn every id equal to map_from[m]
 *                 becomes map_to[m].  input_ids / attention_mask: [n_texts, block_size] of out_bytes (4 or 8) with leading
 *                 dimension ld_out >= block_size elements.
 * prefix_ids / suffix_ids (at most ZETT_ENCODE_MAX_TEMPLATE each, n_prefix + n_suffix < block_size <= 8192) and map_from / map_to (at
 * most ZETT_SPLICE_MAX_ROWS pairs) are HOST arrays, validated before any launch; they travel to the kernels as launch arguments.
 * *status (device) is written by the call: an OR of zett_encode_status bits, 0 when all is well.  With a bit set the outputs are
 * unspecified, but every write stays inside them.  Integers only, the only atomic is the OR into *status: the same inputs give the same
 * bits.  Asynchronous on `stream`, no allocation: `workspace` (device, 16-byte aligned, zett_encode_workspace_bytes: about 180 bytes per
 * byte of text, most of it the worst-case state of words too long for LDS) is free once the call's work is done.  n_texts == 0 is a no-op.
 *
 * zett_encode_texts_added: the same call with the tokenizer's ADDED TOKENS split out of the texts, as the library's added vocabulary does
 * for tokens with normalized = false and no lstrip / rstrip / single_word.  The table is DEVICE memory: n_added
 * tokens, token k the bytes added_bytes[added_offsets[k] .. added_offsets[k + 1]) (int32 offsets from 0 to n_added_bytes), each of 2 to 64
 * bytes, in strictly ascending byte order (a token before every longer one that starts with it), with the id added_ids[k]; at most 512
 * tokens.  A table that breaks this sets ZETT_ENCODE_BAD_TABLE (its offsets are clamped like the texts').
 *   matches       leftmost-longest and non-overlapping on the raw bytes of every text: from byte i the first byte m >= i where a token
 *                 matches is taken with the longest token that matches there; the search goes on behind the match.  A match lies wholly
 *                 inside one text.
 *   sections      what lies between two matches (or a text's end) is encoded as a text of its own — its own prefix decision, the
 *                 pattern sees its end as a text's end —, an empty section gives nothing.
 *   a match       gives exactly one id, added_ids[k]; it counts towards the cut at block_size and map_from / map_to apply to it.
 * n_added == 0 writes exactly what zett_encode_texts writes (the table pointers may be null) and needs the same workspace;
 * zett_encode_added_workspace_bytes is a few bytes per position more otherwise.  No atomic beyond the OR into *status. */
#define ZETT_ENCODE_MAX_TEMPLATE 8
enum zett_encode_flags {
    ZETT_ENCODE_MARKS_ARE_LETTERS = 1,   /* the letter class is [\p{L}\p{M}] (zett/utils.py:29) */
    ZETT_ENCODE_RESPLIT = 2              /* every word is split once more, on its own, with the pattern WITHOUT \p{M}: what a ByteLevel with use_regex behind
                                          * the Split of collator.py:408-411 does to it ("e" + U+0301 becomes two words; U+0301 + "." stays two) */
};
enum zett_encode_prefix { ZETT_ENCODE_PREFIX_NONE = 0, ZETT_ENCODE_PREFIX_ALWAYS = 1, ZETT_ENCODE_PREFIX_UNLESS_SPACE = 2 };
enum zett_encode_status {
    ZETT_ENCODE_NO_UNK = 1,        /* a word needs an unk id the model does not have (the library raises) */
    ZETT_ENCODE_BAD_OFFSETS = 2,   /* text_offsets is not non-decreasing from 0 to n_text */
    ZETT_ENCODE_BAD_TABLE = 4      /* zett_encode_texts_added: the token table's offsets, lengths or order */
};
int zett_encode_workspace_bytes(int64_t n_text, int64_t n_texts, int64_t* bytes);
int zett_encode_texts(zett_retok* r, const uint8_t* text, const int64_t* text_offsets, int64_t n_texts, int64_t n_text, const uint8_t* class_table,
                      int64_t n_code_points, int32_t flags, int32_t prefix_mode, int32_t block_size, const int32_t* prefix_ids, int32_t n_prefix,
                      const int32_t* suffix_ids, int32_t n_suffix, const int32_t* map_from, const int32_t* map_to, int32_t n_map, int32_t pad_id, void* input_ids,
                      void* attention_mask, int32_t out_bytes, int64_t ld_out, void* workspace, int64_t workspace_bytes, int32_t* status, void* stream);
int zett_encode_added_workspace_bytes(int64_t n_text, int64_t n_texts, int32_t n_added, int64_t* bytes);
int zett_encode_texts_added(zett_retok* r, const uint8_t* text, const int64_t* text_offsets, int64_t n_texts, int64_t n_text, const uint8_t* class_table,
                            int64_t n_code_points, int32_t flags, int32_t prefix_mode, int32_t block_size, const int32_t* prefix_ids, int32_t n_prefix,
                            const int32_t* suffix_ids, int32_t n_suffix, const int32_t* map_from, const int32_t* map_to, int32_t n_map, int32_t pad_id, void* input_ids,
                            void* attention_mask, int32_t out_bytes, int64_t ld_out, const uint8_t* added_bytes, const int32_t* added_offsets, const int32_t* added_ids,
                            int32_t n_added, int32_t n_added_bytes, void* workspace, int64_t workspace_bytes, int32_t* status, void* stream);

/* ---- tokenizer sampling (zett_amd/tokenizer_sampling.py DeviceTokenizerSampler; additive, ABI 8) -----------------------------------
 * What rust_utils.TokenizerSampler.sample_tokenizer computes for a batch of texts (rust_utils/src/lib.rs:70-249; restated in
 * tests/sampler_ref.py, the definition this code is tested against), on the device (csrc/tokenizer_sample.hip).
 * A sampler owns the queue of the earlier batches' substring tables and all scratch that depends on its capacities:
 *   max_depth       batches the queue may hold            list_capacity   distinct substrings kept of one batch
 *   table_capacity  slots of the open-addressing table (this call's substrings, then the queue's merged)
 *   max_pieces      the most pieces of the table one call may ask for (seed_size - 256 - 9 * (max_length - 1))
 * zett_sampler_sample: text / text_offsets / class_table as zett_encode_texts takes them; the texts must be distinct (the reference
 * takes them as dictionary keys).  Every text gets a U+0020 in front, the words are the matches of the split pattern without \p{M}.
 * A key is a run of 1 .. max_length - 1 (max_length <= 16) raw bytes of a word from every stride-th entry of the reference's start
 * list; its score grows by the UTF-8 length of its byte-level string.  Then, in the reference's order: with pop_prev the oldest batch
 * leaves the queue; this batch enters at the front; with pop_prev the queue's tables are summed and the outputs written; with
 * push_current == 0 this batch leaves again and the popped one returns.  Outputs (device; written with pop_prev only, else *n_out = 0):
 *   pieces [out_capacity, 16] key bytes, zero padded; piece_lengths [out_capacity] (a separate array: the whitespace runs reach 16
 *   bytes); scores [out_capacity] float64; *n_out.  First the 256 single bytes in byte order at log(min / sum), then for c1 in
 *   (0x20, 0x0A, 0x09), i in 1 .. max_length - 1, c2 in the same three: c2 c1^i at 0.0, then the max(1, seed_size - those) best keys of
 *   two or more bytes with fewer than two of the three whitespace bytes, by p = v / sum + noise_std * z(seed, key) descending, shorter
 *   key first, smaller bytes first; log(p), or -100000.0 for p <= 0 (those keys tie on p).  p is float64 with every operation rounded
 *   on its own; z is standard normal and a function of seed and key bytes alone.
 * *status (device): an OR of zett_sample_status bits; with a bit set the outputs are unspecified but every write stays in bounds.
 * Asynchronous on `stream` (one stream per sampler), no allocation after zett_sampler_create; `workspace` (16-byte aligned,
 * zett_sampler_workspace_bytes) is free once the call's work is done, and so is the text.  No loop waits for another lane and every
 * probe loop ends after table_capacity slots.  zett_sampler_table reads out the merged table of the last call with pop_prev, in no
 * particular order: keys [capacity, 16], key_lengths, counts, z (of that call's seed) and *n (which may exceed capacity: the rest is
 * dropped); ZETT_E_STATE after a call without pop_prev.  A full queue (pop_prev == 0, push_current != 0 at max_depth): ZETT_E_STATE. */
typedef struct zett_sampler zett_sampler;
enum zett_sample_status {
    ZETT_SAMPLE_BAD_OFFSETS = 2,    /* text_offsets is not non-decreasing from 0 to n_text (the bit of ZETT_ENCODE_BAD_OFFSETS) */
    ZETT_SAMPLE_TABLE_FULL = 4,     /* a key found no slot within table_capacity probes: it is not counted */
    ZETT_SAMPLE_LIST_FULL = 8,      /* the batch has more than list_capacity distinct keys: the rest is dropped */
    ZETT_SAMPLE_SUM_OVERFLOW = 16,  /* the sum of the merged scores reached 2^32, where the reference's u32 wraps (it is held in 64 bits here) */
    ZETT_SAMPLE_OUT_FULL = 32       /* more pieces than out_capacity: the rest is dropped */
};
int zett_sampler_create(int device, int32_t max_depth, int64_t list_capacity, int64_t table_capacity, int64_t max_pieces, zett_sampler** out);
int zett_sampler_destroy(zett_sampler* s);
int zett_sampler_depth(const zett_sampler* s, int32_t* depth);
int zett_sampler_workspace_bytes(int64_t n_text, int64_t n_texts, int64_t* bytes);
int zett_sampler_sample(zett_sampler* s, const uint8_t* text, const int64_t* text_offsets, int64_t n_texts, int64_t n_text, const uint8_t* class_table,
                        int64_t n_code_points, int64_t seed_size, int32_t max_length, int32_t stride, double noise_std, uint64_t seed, int32_t pop_prev,
                        int32_t push_current, uint8_t* pieces, uint8_t* piece_lengths, double* scores, int64_t out_capacity, int32_t* n_out, void* workspace,
                        int64_t workspace_bytes, int32_t* status, void* stream);
int zett_sampler_table(zett_sampler* s, uint8_t* keys, uint8_t* key_lengths, uint32_t* counts, double* z, int64_t capacity, int32_t* n, void* stream);

/* ---- sampled vocabulary (zett_amd/sampled_vocab.py DeviceSampledVocabulary; additive, ABI 8) ----------------------------------------
 * From the sampler's piece list, as zett_sampler_sample leaves it on the device, to the step's vocabulary and the tables zett_encode_texts
 * segments with: what zett/collator.py:371-400 does with Python lists and DeviceTextEncoder.from_tokenizer with a host Tokenizer
 * (csrc/sampled_vocab.hip; zett_amd/sampled_vocab.py holds the definition the kernels are tested against).
 * zett_retok_create_unigram_device makes a retokenizer handle whose piece table, bitmap, blob and single-byte ids are allocated for
 * max_vocab entries and empty: a Unigram model without unk id, byte fallback, merges or special table.  zett_retok_destroy frees it.
 * zett_sampled_vocab_build fills it.  pieces / piece_lengths / scores / n: the outputs of zett_sampler_sample (pieces 16-byte aligned,
 * rows [0, min(*n, piece_capacity, seed_size)) are read; seed_size is the caller's upper bound of *n, seed_size + n_special <=
 * max_vocab).  The reference tokenizer's special tokens, n_special <= ZETT_SPLICE_MAX_ROWS of them SORTED BY ID, are DEVICE arrays:
 * special_ids (distinct, >= 0), special_raw_offsets [n_special + 1] into special_raw (the raw bytes of the byte-level strings; an
 * empty range for a string that is not byte-level; at most max_special_raw <= ZETT_SAMPLED_VOCAB_KEY_BYTES bytes each and
 * special_raw_bytes in all, both known to the host), special_char_lengths (characters of the string) and special_hn_ids (the id to put
 * into the token's surface-form row, or -1).  With m the number of pieces that equal no special token's raw bytes, special k gets id
 * min(special_ids[k], m + k) and the kept pieces fill the other ids of [0, m + n_special) in their order.  Outputs (device):
 *   priors [vocab_capacity] the scores bit for bit, 0.0 for a special;  byte_lengths [vocab_capacity] int64: bytes of a piece,
 *   characters of a special;  token_text [text_capacity] / text_offsets [vocab_capacity + 1]: the UTF-8 of every id's byte-level
 *   string back to back, what zett_retokenize_async takes (a special with an hn id has an empty text);
 *   record: 32 bytes, zett_sampled_vocab_record; status is an OR of zett_vocab_status bits, 0 when all is well.
 * The table holds every id with raw bytes under its id and score.  With a status bit set the outputs are unspecified, but every write
 * stays inside them.  Integers and bit copies, and for ZETT_VOCAB_SCORES_THROUGH_JSON one conversion and one correctly rounded division per score: the same inputs give the same bits.  Asynchronous on `stream` (one stream per
 * handle), no allocation; `workspace` (16-byte aligned, zett_sampled_vocab_workspace_bytes) is free once the call's work is done.
 * zett_sampled_vocab_commit takes the record as the caller read it back (HOST memory) and sets what the kernels take by value: the
 * masks, the longest piece and the unknown score table_min_score - 10.  Between build and commit zett_encode_texts and zett_retokenize*
 * return ZETT_E_STATE; a record whose n_vocab is beyond the build's bound is ZETT_E_INVALID.
 * zett_sampled_vocab_table reads out the occupied slots in no particular order: keys [capacity, ZETT_SAMPLED_VOCAB_KEY_BYTES] zero
 * padded, key_lengths, ids, scores, *n (which may exceed capacity: the rest is dropped) and, unless null, single_id [256]: the id of
 * every one-byte piece or -1.  zett_sampled_vocab_patch_rows writes
 * surface_forms [n_rows, maxlen] row min(special_ids[k], record.n_vocab - n_special + k) = special_hn_ids[k], pad_id ... for every k
 * with an hn id (zett/utils.py:671-673); record and the arrays are DEVICE memory. */
#define ZETT_SAMPLED_VOCAB_KEY_BYTES 64
enum zett_vocab_status {
    ZETT_VOCAB_NOT_A_SAMPLE = 1,   /* *n < 256: the list does not hold the alphabet pieces (the reference would prepend the missing characters) */
    ZETT_VOCAB_DUPLICATE = 2,      /* two ids have the same bytes: the second is not in the table */
    ZETT_VOCAB_TABLE_FULL = 4,     /* an id found no slot within the capacity: it is not in the table */
    ZETT_VOCAB_OUT_FULL = 8        /* *n beyond min(piece_capacity, seed_size), or more ids / text than vocab_capacity / text_capacity: the rest is dropped */
};
enum zett_vocab_flags {
    ZETT_VOCAB_SCORES_THROUGH_JSON = 1   /* a slot's score is the sampler's as the tokenizers library reads it back from its own JSON: (double)digits / 10^places
                                          * of the shortest decimal, one ulp off for about one score in nine.  The model of a tokenizer that transformers
                                          * rebuilt from JSON holds these values; priors stay the sampler's bit for bit */
};
typedef struct zett_sampled_vocab_record {
    int32_t n_vocab;      /* m + n_special */
    int32_t n_removed;    /* pieces that were a special token's string */
    int32_t n_text;       /* bytes of token_text */
    int32_t status;
    double min_score;     /* over all n_vocab scores, the specials' 0.0 included */
    double table_min_score; /* over the scores as the table holds them (zett_vocab_flags): the unknown score is this - 10 */
} zett_sampled_vocab_record;
int zett_retok_create_unigram_device(int device, int64_t max_vocab, zett_retok** out);
int zett_sampled_vocab_workspace_bytes(int64_t max_vocab, int32_t n_special, int64_t* bytes);
int zett_sampled_vocab_build(zett_retok* r, const uint8_t* pieces, const uint8_t* piece_lengths, const double* scores, const int32_t* n, int64_t piece_capacity,
                             int64_t seed_size, const int32_t* special_ids, const int32_t* special_raw_offsets, const uint8_t* special_raw,
                             const int32_t* special_char_lengths, const int32_t* special_hn_ids, int32_t n_special, int32_t special_raw_bytes, int32_t max_special_raw,
                             double* priors, int64_t* byte_lengths, int32_t* text_offsets, int64_t vocab_capacity, uint8_t* token_text, int64_t text_capacity,
                             void* record, int32_t flags, void* workspace, int64_t workspace_bytes, void* stream);
int zett_sampled_vocab_commit(zett_retok* r, const void* host_record);
int zett_sampled_vocab_table(zett_retok* r, uint8_t* keys, int32_t* key_lengths, int32_t* ids, double* scores, int32_t* single_id, int64_t capacity, int32_t* n,
                             void* stream);
int zett_sampled_vocab_patch_rows(zett_retok* r, const void* record, const int32_t* special_ids, const int32_t* special_hn_ids, int32_t n_special,
                                  int32_t* surface_forms, int64_t n_rows, int32_t maxlen, int32_t pad_id, void* stream);

/* ---- fitting a fresh hypernetwork's Rescalers (zett_amd/training.py column_moments, rescaler_fit) -----------------------------------
 * Hypernet.init_rescaler of the reference (zett/model/__init__.py:348-385) through Rescaler.scale_to (zett/utils.py:165-175): per
 * column, w = t_std / (std(x) + 1e-8) and b = t_mean - mean(x * w), with the population std (ddof = 0).  The calls below are
 * csrc/train_init.hip.  No float atomics and a partition that depends on (rows, cols) alone: the same call gives the same bits on
 * every run and every device.
 *
 * The STATE of `cols` columns is cols triples of doubles, column c at state[3 c .. 3 c + 2]:
 *     count (an integer value), mean, M2 = sum (x - mean)^2
 * 24 bytes per column, 8-byte aligned, on the device.  Interleaved, so that the state of a column range [c0, c1) of a matrix is the
 * contiguous slice state + 3 c0 of the matrix's state: no second pass for a range.  fp64, because a state is merged into (below)
 * and read back by a fit whose quotient t_std / (std + 1e-8) amplifies what the state lost; it is 24 bytes per column either way. */
#define ZETT_COL_MOMENTS_CHUNK 256     /* rows of one partial: part of the definition of the result */
/* bytes of the workspace of a call over `rows` rows and `cols` columns: two doubles per (chunk, column), at least 16 */
int zett_op_col_moments_workspace_bytes(int64_t rows, int32_t cols, int64_t* bytes);
/* The moments of columns [col0, col0 + cols) of the row-major matrix x (zett_dtype dtype, leading dimension ld elements, `rows` rows),
 * every element read exactly once and converted exactly.  With R = ZETT_COL_MOMENTS_CHUNK the rows are cut into the chunks
 * [j R, min(rows, (j + 1) R)).  Within a chunk a column is one Welford recurrence in fp64 over ascending rows,
 *     d = x - mean;  mean = fma(d, 1 / k, mean);  M2 = fma(d, x - mean, M2)          k = 1, 2, ... the rows so far
 * whose (mean, M2) goes to the workspace; a second kernel then merges the chunks in ascending order with Chan's update
 *     n = na + nb;  d = mean_b - mean_a;  r = nb / n;  mean = mean_a + d r;  M2 = M2_a + M2_b + d d (na r)
 * starting from the empty state (accumulate = 0) or from what `state` holds (accumulate = 1: rows fed call by call).  The result
 * does not depend on col0, ld or the alignment of x: 16-byte reads per lane where the address of a row's column and ld allow them,
 * element reads for the columns in front of the first aligned one, behind the last whole vector, or for all of them — the recurrence
 * of a column is the same on both paths.  It DOES depend on how a caller cuts the rows into calls.
 * rows = 0: accumulate = 1 leaves the state untouched, accumulate = 0 writes the empty state (0, 0, 0), which the fit refuses.
 * ZETT_E_INVALID, before any launch: a null or misaligned x / state / workspace (8 bytes), rows < 0, cols < 1, col0 < 0, col0 + cols > ld,
 * an unknown dtype, a workspace below the queried size. */
int zett_op_col_moments(const void* x, int32_t dtype, int64_t ld, int64_t rows, int32_t col0, int32_t cols, void* state, int32_t accumulate, void* workspace,
                        int64_t workspace_bytes, void* stream);
/* w[c] = t_std / (std_x + 1e-8), b[c] = t_mean - w[c] mean_x for c < cols, fp32 (computed in fp64, rounded once each), with
 * std = sqrt(M2 / count) of a state.  The target's std and mean come from target_state (a state of the same number of columns), or,
 * with target_state NULL, from the two scalars target_std / target_mean for every column.  (The reference takes the mean of x * w;
 * w mean(x) is the same quantity.)  The call reads the count of both states back — it waits for `stream` once — and a state of
 * count 0 is ZETT_E_INVALID, as are null x_state / w / b, a misaligned state and cols < 1; nothing is launched then. */
int zett_op_rescaler_fit(const void* x_state, int32_t cols, const void* target_state, double target_std, double target_mean, float* w, float* b, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZETT_HIP_H */
