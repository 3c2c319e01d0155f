#!/usr/bin/env python
"""Time of the lexical (FVT / BFVT) transfer on the GPU, stage by stage, on a synthetic workload of zett_amd/synth.py.

    python tools/lexical_bench.py --workload xlmr_gpt2 [--exact_share 0.5] [--src_dtypes float32,bfloat16] [--iters 20]

The source tokenizer is the workload's synthetic hn model (make_hn_model), the target tokens are strings that retokenize to a
seeded surface-form matrix (tokens_for_surface_forms), the source matrix is make_source_embeddings (split into its input / output
halves where the workload has separate output embeddings: two pointers with a leading dimension of 2E).  The synthetic
vocabulary shares next to no exact strings with its targets, so --exact_share replaces that share of the targets by source
pieces.  Prints ONE JSON line.  Two yardsticks, measured in the same process, neither of them the code under test:

  zett_scatter_rows moving the same destination bytes   (the HBM write stream the rows kernel cannot beat)
  the retokenizer (zett_retokenize_async + result) on the same tokens at maxlen = width   (what the plan adds to it)

Times: the rows stage and the scatter with device events around `iters` back-to-back calls after a warm-up; the plan and the
retokenizer with a host clock around calls that end in a device synchronise (both include the same host work: one join /
encode of the tokens and one upload).  bytes moved = sum(count) * D * sizeof(src) + rows * D * sizeof(dst).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from zett_amd import _lib, synth  # noqa: E402
from zett_amd.lexical import LexicalTransfer  # noqa: E402
from zett_amd.surface_forms import DeviceRetokenizer, HnTokenizerSpec  # noqa: E402

PEAK_TBS = 8.0          # sanity only: an implied bandwidth above the HBM peak means the timing or the byte count is wrong


def event_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def wall_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="xlmr_gpt2")
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--exact_share", type=float, default=0.0)
    ap.add_argument("--fvt_mode", default="bfvt")
    ap.add_argument("--src_dtypes", default="float32,bfloat16")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu_restatement", type=int, default=0, help="no GPU: time tests/lexical_ref.py on this many rows (context figure) and exit")
    args = ap.parse_args()

    cfg, rows, _, hist = synth.workload(args.workload)
    rows = args.rows or rows
    model, piece_of_id = synth.make_hn_model(args.workload, cfg)
    vocab = dict(model["vocab"]) if isinstance(model["vocab"], dict) else {p: i for i, (p, _) in enumerate(model["vocab"])}
    sfm = synth.make_surface_forms(cfg, rows, seed=3, hist=hist)
    tokens = synth.tokens_for_surface_forms(cfg, sfm, piece_of_id)
    R = int(cfg["original_vocab_size"])
    if args.exact_share > 0:
        rng = np.random.default_rng(5)
        pieces = [p for p, i in vocab.items() if 3 <= i < R]
        for r in np.flatnonzero(rng.random(rows) < args.exact_share):
            tokens[r] = pieces[int(rng.integers(0, len(pieces)))]
    E = int(cfg["n_embd"])
    separate = bool(cfg.get("separate_out_embeddings"))
    D = 2 * E if separate else E

    if args.cpu_restatement:          # context only: the CPU restatement (one process), model construction not counted
        from tests import lexical_ref
        n = min(args.cpu_restatement, rows)
        host_S = synth.make_source_embeddings(cfg, seed=3, dtype="float32", rows=R)
        ref_model = lexical_ref.bare_model(model)
        t0 = time.perf_counter()
        lexical_ref.rows(host_S, lexical_ref.plan(ref_model, vocab, tokens[:n], R, args.fvt_mode), 0)
        print(json.dumps({"workload": args.workload, "cpu_restatement_rows": n, "columns": D,
                          "cpu_restatement_rows_per_s_one_process": n / (time.perf_counter() - t0)}))
        return
    assert torch.cuda.is_available(), "tools/lexical_bench.py needs an MI355X"
    dev = torch.device("cuda", 0)
    spec = HnTokenizerSpec.from_model_json(model, (), (), -1)
    lt = LexicalTransfer(spec, dev, vocab=vocab, unk_token_id=0)
    plan = lt.plan(tokens, R, args.fvt_mode)
    count = plan.count.cpu().numpy()
    classes = {"count_0_fallback": int((count == 0).sum()), "count_1_copy": int((count == 1).sum()), "count_gt_1_mean": int((count > 1).sum())}
    out = {"workload": args.workload, "rows": rows, "n_source_rows": R, "n_embd": E, "columns": D, "separate_out": separate, "fvt_mode": args.fvt_mode,
           "exact_share": args.exact_share, "width": plan.width, "rows_replanned": plan.n_replanned, "overlap": plan.overlap,
           "rows_by_class": classes, "mean_count": float(count.mean()), "sum_count": int(count.sum()), "iters": args.iters, "runs": []}

    # the plan against the retokenizer on the same tokens at maxlen = width
    rt = DeviceRetokenizer(HnTokenizerSpec.from_model_json(model, (), (), 0), dev)
    out["plan_ms"] = wall_ms(lambda: lt.plan(tokens, R, args.fvt_mode), max(3, args.iters // 4), 2)
    out["retokenize_ms"] = wall_ms(lambda: rt(tokens, plan.width), max(3, args.iters // 4), 2)
    out["plan_over_retokenize"] = out["plan_ms"] / out["retokenize_ms"]

    lib = _lib.load()
    host_S = synth.make_source_embeddings(cfg, seed=3, dtype="float32", rows=R)
    for name in args.src_dtypes.split(","):
        dtype = getattr(torch, name)
        S = torch.from_numpy(host_S).to(dev).to(dtype)
        src_in, src_out = (S[:, :E], S[:, E:]) if separate else (S, None)
        dst_in = torch.empty((rows, E), dtype=dtype, device=dev)
        dst_out = torch.empty_like(dst_in) if separate else None
        rows_ms = event_ms(lambda: lt.rows_into(plan, src_in, src_out, "unk", dest_in=dst_in, dest_out=dst_out), args.iters, args.warmup)
        esize = S.element_size()
        moved = float(count.sum()) * D * esize + float(rows) * D * esize
        # yardstick: the same destination bytes through zett_scatter_rows (identity order; one [rows, D] stream in, one out)
        stage = torch.empty((rows, D), dtype=dtype, device=dev)
        sink = torch.empty_like(stage)
        order = torch.arange(rows, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream

        def scatter():
            _lib.check(lib.zett_scatter_rows(C.c_void_p(stage.data_ptr()), C.c_void_p(sink.data_ptr()), C.c_void_p(order.data_ptr()), rows, D * esize, 0,
                                             C.c_void_p(stream)), "zett_scatter_rows")

        scatter_ms = event_ms(scatter, args.iters, args.warmup)
        run = {"src_dtype": name, "dst_dtype": name, "rows_ms": rows_ms, "bytes_moved": moved, "implied_TBps": moved / (rows_ms * 1e-3) / 1e12,
               "scatter_rows_ms": scatter_ms, "scatter_bytes": 2.0 * rows * D * esize, "scatter_TBps": 2.0 * rows * D * esize / (scatter_ms * 1e-3) / 1e12,
               "rows_over_scatter": rows_ms / scatter_ms}
        assert run["implied_TBps"] <= PEAK_TBS, f"implied {run['implied_TBps']:.2f} TB/s exceeds the HBM peak: timing or byte count is wrong"
        out["runs"].append(run)
        del S, src_in, src_out, dst_in, dst_out, stage, sink

    print(json.dumps(out))


if __name__ == "__main__":
    main()
