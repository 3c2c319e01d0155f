"""The cases of tests/golden/forward_launch_log.json: what tests/golden/make_golden_forward_launch_log.py records on a library built
from the commit BEFORE a change of the forward's host orchestration, and tests/test_forward_launch_log_gpu.py asserts on the library
under test.  Per case: the GEMM launch sequence (m, n, k, variant, epilogue), stats() without its timing fields, workspace_bytes()
and the sha256 of every output's bytes.  The shapes are the smallest that reach each branch of the orchestration (csrc/zett_hip.hip):
the LayerNorm launcher's four kernels, every ForwardMode, one and two chunks, two lanes, the pair lever, both head layouts, every
destination store, the shared table, a prepared plan, the single-rows lever, layer 0's Q/K/V per source id and the options of a GEMM launch."""
import hashlib

import numpy as np
import torch

from zett_amd import synth
from zett_amd.dims import HypernetDims

SEED = 11
LANG = 3


def _cfg(hidden, heads, inter, layers, **extra):
    return dict(synth.workload("tiny")[0], n_embd=128, hn_hidden_size=hidden, hn_num_attention_heads=heads, hn_intermediate_size=inter, hn_n_layers=layers, **extra)


CONFIGS = {
    "tiny": (synth.workload("tiny")[0], 700),                  # H = 128: no fold, layernorm_rows_kernel TPR 64, language position
    "h512": (_cfg(512, 8, 1024, 2), 600),                      # fold on, layernorm_rows8_kernel TPR 32
    "h512_norescale": (_cfg(512, 8, 1024, 2, hn_rescale_embeddings=False), 600),      # the head_one / head_zero epilogue
    "h512_nobias": (_cfg(512, 8, 1024, 2, hn_predict_bias=False), 600),
    "h512_oneout": (_cfg(512, 8, 1024, 2, separate_out_embeddings=False), 600),
    "h512_split": (_cfg(512, 8, 1024, 2, hn_single_head=True), 600),                  # single_head + separate_out: the split head, unfolded
    "h512_nolang": (_cfg(512, 8, 1024, 2, hn_embed_lang_id=False), 600),              # no language position: rows that keep ONE position exist
    "h1536": (_cfg(1536, 24, 512, 2), 300),                    # rows8 TPR 64
    "h2560": (_cfg(2560, 20, 512, 1), 300),                    # TPR 256; the only layer is the position-0-only one; no pair plan
}

# name -> (config, precision, options, kind); kind: "forward", or one of the special runs of run_case
CASES = {}
for _prec in ("f32", "f16", "bf16"):
    for _tag, _opt in (("default", {}), ("chunks", {"max_chunk_tokens": 1024}), ("nopairs", {"pair_dedupe": 0}), ("all_positions", {"cls_only_last_layer": 0})):
        CASES[f"tiny_{_prec}_{_tag}"] = ("tiny", _prec, _opt, "forward")
for _tag, _prec, _opt in (("default", "f16", {}), ("residual_lo0", "f16", {"residual_lo": 0}), ("table_lo0", "f16", {"table_lo": 0}), ("ln_fold0", "f16", {"ln_fold": 0}),
                          ("ln_fold2", "f16", {"ln_fold": 2}), ("ln_rows8_0", "f16", {"ln_rows8": 0}), ("bf16", "bf16", {}), ("bf16_residual_lo2", "bf16", {"residual_lo": 2}),
                          ("two_lanes", "f16", {"concurrent_lanes": 2}), ("chunks", "f16", {"max_chunk_tokens": 1024})):
    CASES[f"h512_{_tag}"] = ("h512", _prec, _opt, "forward")
for _name in ("h512_norescale", "h512_nobias", "h512_oneout", "h512_split", "h1536"):
    CASES[_name] = (_name, "f16", {}, "forward")
CASES["h2560_f16"] = ("h2560", "f16", {}, "forward")
CASES["h2560_f32"] = ("h2560", "f32", {}, "forward")
CASES["into_bf16_permuted"] = ("h512", "f16", {}, "into_bf16_permuted")      # fused destination store
CASES["into_f32_identity"] = ("h512", "f16", {}, "into_f32_identity")
CASES["into_split"] = ("h512_split", "f16", {}, "into_f32_identity")         # staged store, both halves
CASES["into_bias_f16"] = ("h512", "f16", {}, "into_bias_f16")
CASES["into_no_bias"] = ("h512", "f16", {}, "into_no_bias")                  # the sink path
CASES["shared_table"] = ("h512", "f16", {}, "shared_table")                  # table_plan -> table_rows -> forward_table
CASES["prepared"] = ("h512", "f16", {}, "prepared")                          # prepare(x) then forward(x)
CASES["prepared_other"] = ("h512", "f16", {}, "prepared_other")              # prepare(x) then forward(y): the plan is made again
# "single_rows": 2 (skip the query / key GEMM rows of single-position rows whenever possible).  On h512 every row also keeps the language
# position, so the forward asks and declines; h512_nolang takes it: Q|K launches from a row offset, outputs through cls_row
for _cfg_name, _tag in (("h512", "single_rows"), ("h512_nolang", "single_rows_taken")):
    CASES[_tag] = (_cfg_name, "f16", {"single_rows": 2}, "forward")
    CASES[_tag + "_into"] = (_cfg_name, "f16", {"single_rows": 2}, "into_bf16_permuted")
# "id_qkv": 2 (lever 6: layer 0's Q/K/V once per distinct source id, whenever possible — h512_nolang has no language position): alone, per
# buffer row instead of per pair, over two chunks, through the fused destination store, and on a caller's table (the table_gather path)
for _tag, _opt, _kind in (("id_qkv", {}, "forward"), ("id_qkv_nopairs", {"pair_dedupe": 0}, "forward"), ("id_qkv_chunks", {"max_chunk_tokens": 1024}, "forward"),
                          ("id_qkv_into", {}, "into_bf16_permuted"), ("id_qkv_shared_table", {}, "shared_table")):
    CASES[_tag] = ("h512_nolang", "f16", dict({"id_qkv": 2}, **_opt), _kind)
# the options of a GEMM launch, "attention_fast" and "time_gemm" (event pairs around the launches: the same log and outputs as h512_default)
for _tag, _opt in (("tail_split2", {"gemm_tail_split": 2}), ("tail_split3", {"gemm_tail_split": 3}), ("gemm_variant2", {"gemm_variant": 2}),
                   ("attention_fast0", {"attention_fast": 0}), ("time_gemm", {"time_gemm": 1})):
    CASES[f"h512_{_tag}"] = ("h512", "f16", _opt, "forward")

TIMING_FIELDS = ("gemm_ms", "gemm_flops_timed")


def _sha(t):
    return None if t is None else hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _engine(cfg, precision):
    from zett_amd.hypernet import HipEngine
    dev = torch.device("cuda:0")
    eng = HipEngine(HypernetDims.from_config(cfg), 1e-5, dev, precision)
    eng.load_weights({k: torch.from_numpy(v).to(dev) for k, v in synth.make_weights(cfg, SEED).items()})
    return eng


def _into(eng, ids, src, lang, dtype, permuted, bias):
    d, n = eng.dims, ids.shape[0]
    rows = torch.from_numpy(np.random.default_rng(SEED).permutation(n + 7)[:n].astype(np.int64)).cuda() if permuted else None
    n_dest = n + 7 if permuted else n
    out_in = torch.zeros((n_dest, d.n_embd), dtype=dtype, device=eng.device)
    out_out = torch.zeros((n_dest, d.n_embd), dtype=dtype, device=eng.device) if d.separate_out else None
    out_bias = None if bias is None else torch.zeros((n_dest,), dtype=bias, device=eng.device)
    eng.forward_into(ids, src, lang, out_in, out_out, out_bias, rows)
    return out_in, out_out, out_bias


def run_case(name):
    """Run a case on the library zett_amd._lib loads -> {"gemm_log", "stats", "workspace_bytes", "outputs"} (JSON-ready)."""
    cfg_name, precision, options, kind = CASES[name]
    cfg, n_rows = CONFIGS[cfg_name]
    lang = LANG if cfg.get("hn_embed_lang_id") else -1
    eng = _engine(cfg, precision)
    for key, value in options.items():
        eng.set_option(key, value)
    src = torch.from_numpy(synth.make_source_embeddings(cfg, SEED)).cuda()
    ids = torch.from_numpy(synth.make_surface_forms(cfg, n_rows, seed=SEED, n_special=2)).cuda()
    if kind == "forward":
        outs = eng.forward(ids, src, lang)
    elif kind == "into_bf16_permuted":
        outs = _into(eng, ids, src, lang, torch.bfloat16, True, torch.float32)
    elif kind == "into_f32_identity":
        outs = _into(eng, ids, src, lang, torch.float32, False, torch.float32)
    elif kind == "into_bias_f16":
        outs = _into(eng, ids, src, lang, torch.float32, False, torch.float16)
    elif kind == "into_no_bias":
        outs = _into(eng, ids, src, lang, torch.float32, False, None)
    elif kind == "shared_table":
        id_slot, id_list, n_ids = eng.table_plan(ids)
        table, stats = eng.table_buffers(n_ids)
        half = n_ids // 2
        eng.table_rows(id_list, half, n_ids - half, src, table, stats)       # (two slices, out of order)
        eng.table_rows(id_list, 0, half, src, table, stats)
        outs = eng.forward_table(ids, table, stats, id_slot, lang)
    elif kind in ("prepared", "prepared_other"):
        first = ids.to(torch.int32).contiguous()
        eng.prepare(first)
        if kind == "prepared_other":
            first = torch.from_numpy(synth.make_surface_forms(cfg, n_rows, seed=SEED + 1, n_special=2)).cuda().to(torch.int32).contiguous()
        outs = eng.forward(first, src, lang)
    else:
        raise KeyError(kind)
    torch.cuda.synchronize()
    record = {"gemm_log": [[r["m"], r["n"], r["k"], r["variant"], r["epilogue"]] for r in eng.gemm_log()],
              "stats": {k: v for k, v in eng.stats().items() if k not in TIMING_FIELDS},
              "workspace_bytes": eng.workspace_bytes(n_rows, ids.shape[1]),
              "outputs": [_sha(t) for t in outs]}
    eng.close()
    return record
