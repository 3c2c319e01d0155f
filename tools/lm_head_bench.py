#!/usr/bin/env python
"""The language-model loss over predicted output embeddings, forward + backward, timed two ways in one process with HIP events on the
same tensors (the reference's training shape: train_batch_size 128 x block_size 128 = 16 384 positions, a sampled vocabulary of 32 768
tokens, E = 4 096, bf16):

  torch : the glue a user writes without this module — a bf16 F.linear, a float cast, the mask add, F.cross_entropy, autograd
  hip   : zett_amd.training.lm_head_loss (csrc/train_loss.hip between the library's GEMMs), loss.backward()

    python tools/lm_head_bench.py [--t 16384] [--v 32768] [--e 4096] [--precision bf16] [--steps 10] [--warmup 3] [--only hip|torch]

Both produce d hidden (bf16) and d pred_out (fp32).  Reports the median milliseconds of a step and the peak of
torch.cuda.max_memory_allocated above what the inputs hold.  The three contractions are 6 T V E FLOP (13.2 TFLOP at the default shape).
Prints a table and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from zett_amd.training import lm_default_chunk_rows, lm_head_loss  # noqa: E402

MASK_FILL = -100000.0


def timed(fn, steps, warmup):
    """(median ms, all ms) of fn() between HIP events, one event pair per step; (peak bytes above the resident tensors)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), ms, torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--t", type=int, default=16384)
    ap.add_argument("--v", type=int, default=32768)
    ap.add_argument("--e", type=int, default=4096)
    ap.add_argument("--precision", default="bf16", choices=["bf16", "f16", "f32"])
    ap.add_argument("--chunk-rows", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="", choices=["", "hip", "torch"])
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    t, v, e = args.t, args.v, args.e
    lo = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}[args.precision]
    gen = torch.Generator(device=dev).manual_seed(1234)
    hidden = torch.randn(t, e, device=dev, generator=gen).to(lo).requires_grad_(True)
    w_out = (2.0 * torch.randn(v, e, device=dev, generator=gen) / e ** 0.5).requires_grad_(True)
    labels = torch.randint(0, v, (t,), device=dev, generator=gen)
    vocab_mask = torch.rand(v, device=dev, generator=gen) >= 0.05
    labels = torch.where(vocab_mask[labels], labels, torch.nonzero(vocab_mask)[0, 0].expand_as(labels))
    weight = (torch.rand(t, device=dev, generator=gen) >= 0.1).float()
    chunk = args.chunk_rows or None

    def clear():
        hidden.grad = None
        w_out.grad = None

    def torch_step():
        clear()
        logits = F.linear(hidden, w_out.to(lo)).float() + torch.where(vocab_mask, 0.0, MASK_FILL)
        loss = (F.cross_entropy(logits, labels, reduction="none") * weight).sum() / weight.sum()
        loss.backward()
        return loss

    def hip_step():
        clear()
        loss, _ = lm_head_loss(hidden, w_out, labels, weight=weight, vocab_mask=vocab_mask, precision=args.precision, chunk_rows=chunk)
        loss.backward()
        return loss

    out = {"metric": "lm head loss, forward + backward", "t": t, "v": v, "e": e, "precision": args.precision,
           "chunk_rows": chunk or min(t, lm_default_chunk_rows(v, args.precision)), "contraction_tflop": 6.0 * t * v * e / 1e12, "steps": args.steps, "warmup": args.warmup}
    losses = {}
    for name, fn in (("torch", torch_step), ("hip", hip_step)):
        if args.only and args.only != name:
            continue
        losses[name] = float(fn().detach())
        grads = (hidden.grad.float().clone(), w_out.grad.clone())
        med, ms, peak = timed(fn, args.steps, args.warmup)
        out[name] = {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "peak_bytes": peak, "loss": losses[name], "tflops": 6.0 * t * v * e / (med * 1e-3) / 1e12}
        out[name + "_grads"] = grads
        clear()
        torch.cuda.empty_cache()
    if "torch_grads" in out and "hip_grads" in out:
        for i, key in enumerate(("d_hidden", "d_pred_out")):
            a, b = out["hip_grads"][i].double(), out["torch_grads"][i].double()
            out[key + "_rel_diff"] = float((a - b).norm() / b.norm())
        out["loss_rel_diff"] = abs(losses["hip"] - losses["torch"]) / abs(losses["torch"])
    out.pop("torch_grads", None)
    out.pop("hip_grads", None)

    print(f"| T = {t}, V = {v}, E = {e}, {args.precision}, forward + backward | median ms | min | max | TFLOP/s | peak memory GB |")
    print("|---|---:|---:|---:|---:|---:|")
    for name, label in (("torch", "torch glue (F.linear, float, mask add, F.cross_entropy, autograd)"), ("hip", f"lm_head_loss (chunks of {out['chunk_rows']} rows)")):
        if name in out:
            r = out[name]
            print(f"| {label} | {r['median_ms']:.2f} | {r['min_ms']:.2f} | {r['max_ms']:.2f} | {r['tflops']:.0f} | {r['peak_bytes'] / 1e9:.2f} |")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
