#!/usr/bin/env python
"""GPU box: what storing the predicted rows straight into a destination is worth (zett_forward_into).
  1. the engine step at the headline shape: forward() against forward_into() (bf16 destination, identity rows), f16 policy;
  2. predict_vocabulary on a workload walked in batches of 16 384 rows (default C5 = llama3_256k: 262 144 rows, 16 batches), the direct
     path (ZETT_DIRECT_OUT=1) against the accumulating one (=0): wall time and max_memory_allocated.
One JSON line per figure.

    python tools/dest_bench.py [--step-workload NAME] [--vocab-workload NAME] [--reps N]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import device_weights  # noqa: E402
from zett_amd import synth  # noqa: E402
from zett_amd.config import ZettHypernetConfig  # noqa: E402
from zett_amd.hypernet import ZettHypernet  # noqa: E402
from zett_amd.transfer import Args, predict_vocabulary  # noqa: E402


def _model(name, dev):
    cfg, rows, src_dtype, hist = synth.workload(name)
    model = ZettHypernet(ZettHypernetConfig(**cfg))
    model.load_state_dict({k: v.float().cpu() for k, v in device_weights(cfg, dev, seed=0).items()})
    model = model.to(dev).eval()
    g = torch.Generator(device=dev); g.manual_seed(1)
    src = (0.02 * torch.randn((cfg["original_vocab_size"], model.dims.n_in_embd), device=dev, generator=g)).to(getattr(torch, src_dtype))
    sfm = torch.from_numpy(synth.make_surface_forms(cfg, rows, seed=0, hist=hist)).to(dev)
    lang = 3 if model.dims.embed_lang else None
    return model, src, sfm, lang, rows


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step-workload", default="mistral_gpt2_32k")
    ap.add_argument("--vocab-workload", default="llama3_256k")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda:0")

    model, src, sfm, lang, rows = _model(a.step_workload, dev)
    eng = model.engine(dev, "f16")
    ids = sfm.to(torch.int32).contiguous()
    lg = lang if lang is not None else -1
    E = model.dims.n_embd
    d_in = torch.empty((rows, E), dtype=torch.bfloat16, device=dev)
    d_out = torch.empty_like(d_in) if model.dims.separate_out else None
    d_bias = torch.empty((rows,), dtype=torch.bfloat16, device=dev)
    for _ in range(2):
        eng.forward(ids, src, lg); eng.forward_into(ids, src, lg, d_in, d_out, d_bias)
    res = {"figure": "engine_step", "workload": a.step_workload, "rows": rows}
    for mode in ("forward", "forward_into_bf16"):
        fn = (lambda: eng.forward(ids, src, lg)) if mode == "forward" else (lambda: eng.forward_into(ids, src, lg, d_in, d_out, d_bias))
        res[mode + "_ms"], res[mode + "_all_ms"] = _median_ms(fn, a.reps)
    print(json.dumps(res), flush=True)
    del model, eng, src, sfm, d_in, d_out, d_bias
    torch.cuda.empty_cache()

    model, src, sfm, lang, rows = _model(a.vocab_workload, dev)
    res = {"figure": "predict_vocabulary", "workload": a.vocab_workload, "rows": rows, "batch_size": 16384, "batches": -(-rows // 16384)}
    args = Args(output="", batch_size=16384)
    for flag in ("0", "1"):
        os.environ["ZETT_DIRECT_OUT"] = flag
        predict_vocabulary(model, sfm, src, lang, args)          # (warm-up: engine, table, workspace)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        ms, ts = _median_ms(lambda: predict_vocabulary(model, sfm, src, lang, args), max(3, a.reps // 2))
        res[f"direct{flag}_ms"], res[f"direct{flag}_all_ms"] = ms, ts
        res[f"direct{flag}_max_memory_allocated"] = torch.cuda.max_memory_allocated(dev)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
