#!/usr/bin/env python
"""The input side of a training step — special rows, token lookup, the lookup's backward — timed two ways in one process with HIP events
on the same tensors (the reference's training shape: 128 x 128 = 16 384 positions, a sampled vocabulary of 32 768 tokens, E = 4 096, fp32
pred_in, bf16 inputs_embeds, bf16 upstream gradient, 8 special rows):

  torch : the glue a user writes without this module — index_copy, F.embedding, .to(bfloat16), autograd backward
  hip   : zett_amd.training.splice_special_rows + token_embeddings (csrc/train_embed.hip), piece by piece and as their sum

    python tools/embed_lookup_bench.py [--t 16384] [--v 32768] [--e 4096] [--specials 8] [--steps 10] [--warmup 3] [--out FILE.md]

Two id distributions: "zipf" (ids = floor(V u^3), the recipe of tests/embed_lookup_ref.py) and "padded" (the same with 30 % of the
positions set to one pad id — a list of about 5 000 positions, the case the chunked sum exists for).  Per distribution the variants
ALTERNATE (one repetition of each, then the next repetition), 3 warm-up and 10 timed repetitions; medians and min-max are reported,
with each kernel's algorithmic bytes over its time as a fraction of the 6.29 TB/s copy rate of profiles/train_step.md, and
torch.cuda.max_memory_allocated above the resident tensors.  Prints a markdown table and one JSON line.
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

from zett_amd import training  # noqa: E402

COPY_RATE = 6.29e12          # bytes / s, profiles/train_step.md


def measure(variants, steps, warmup):
    """variants: name -> fn.  One repetition of every variant in turn, `warmup` + `steps` times; -> name -> list of ms (timed repetitions)."""
    ms = {name: [] for name in variants}
    for rep in range(warmup + steps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if rep >= warmup:
                ms[name].append(a.elapsed_time(b))
    return ms


def peak_of(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--t", type=int, default=16384)
    ap.add_argument("--v", type=int, default=32768)
    ap.add_argument("--e", type=int, default=4096)
    ap.add_argument("--specials", type=int, default=8)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    t, v, e = args.t, args.v, args.e
    gen = torch.Generator().manual_seed(1234)
    u = torch.rand(t, generator=gen)
    zipf = torch.floor(v * u ** 3).to(torch.int64).clamp_(max=v - 1)
    padded = zipf.clone()
    padded[torch.randperm(t, generator=gen)[:int(0.3 * t)]] = 1
    dgen = torch.Generator(device=dev).manual_seed(1234)
    pred = torch.randn(v, e, device=dev, generator=dgen)
    src = torch.randn(v, 2 * e, device=dev, generator=dgen).to(torch.bfloat16)
    upstream = torch.randn(t, e, device=dev, generator=dgen).to(torch.bfloat16)
    special = [int(x) for x in torch.randperm(v, generator=gen)[:args.specials]]
    in_reference = [int(x) for x in torch.randperm(v, generator=gen)[:args.specials]]
    idx, ref = torch.tensor(special, device=dev), torch.tensor(in_reference, device=dev)
    bf16 = torch.bfloat16

    def splice(matrix, inplace):          # (nothing requires grad: the kernel alone, behind the host-side validation of the lists)
        return training.splice_special_rows(matrix, None, src, special, in_reference, inplace=inplace)[0]

    result = {"metric": "special rows + token lookup, forward + backward", "t": t, "v": v, "e": e, "specials": args.specials, "steps": args.steps, "warmup": args.warmup}
    lines = []
    for dist, ids_cpu in (("zipf", zipf), ("padded", padded)):
        ids = ids_cpu.to(dev)
        counts = torch.bincount(ids_cpu, minlength=v)
        scratch = pred.clone()          # what the in-place splice writes to
        plan = training.embed_lookup_plan(ids, v)
        leaf = pred.clone().requires_grad_(True)

        def hip_pieces():          # the four calls in a row, the outputs held as autograd would hold them
            out = training.token_embeddings(splice(scratch, True), ids, dtype=bf16, check_ids=False)
            p = training.embed_lookup_plan(ids, v)
            return out, p, training.embed_lookup_backward(upstream, p, t, v, e)

        def torch_glue():
            x = leaf.index_copy(0, idx, src[ref, :e].float())
            F.embedding(ids, x).to(torch.bfloat16).backward(upstream)
            leaf.grad = None

        variants = {
            "splice, out of place": lambda: splice(pred, False),
            "splice, in place": lambda: splice(scratch, True),
            "lookup forward": lambda: training.token_embeddings(pred, ids, dtype=bf16, check_ids=False),
            "plan": lambda: training.embed_lookup_plan(ids, v),
            "lookup backward": lambda: training.embed_lookup_backward(upstream, plan, t, v, e),
            "torch glue": torch_glue,
        }
        ms = measure(variants, args.steps, args.warmup)
        pieces = ("splice, in place", "lookup forward", "plan", "lookup backward")
        ms["sum of splice (in place), forward, plan, backward"] = [sum(ms[p][i] for p in pieces) for i in range(args.steps)]
        # (no fraction for the in-place splice and the plan: a launch that moves 8 rows, and integer work, are not bandwidth-bound)
        nbytes = {"splice, out of place": 2 * 4 * v * e, "lookup forward": t * e * (4 + 2), "lookup backward": t * e * 2 + v * e * 4}
        peaks = {"torch glue": peak_of(torch_glue), "sum of splice (in place), forward, plan, backward": peak_of(hip_pieces)}
        res = {"max_count": int(counts.max()), "ids_used": int((counts > 0).sum())}
        lines.append(f"| {dist}: longest list {res['max_count']}, {res['ids_used']} ids used | median ms | min | max | bytes / time of 6.29 TB/s | peak memory GB |")
        lines.append("|---|---:|---:|---:|---:|---:|")
        for name, xs in ms.items():
            med = statistics.median(xs)
            res[name] = {"median_ms": med, "min_ms": min(xs), "max_ms": max(xs)}
            frac = f"{nbytes[name] / (med * 1e-3) / COPY_RATE:.2f}" if name in nbytes else ""
            peak = f"{peaks[name] / 1e9:.2f}" if name in peaks else ""
            if name in peaks:
                res[name]["peak_bytes"] = peaks[name]
            lines.append(f"| {name} | {med:.3f} | {min(xs):.3f} | {max(xs):.3f} | {frac} | {peak} |")
        ours, theirs = res["sum of splice (in place), forward, plan, backward"], res["torch glue"]
        overlap = ours["min_ms"] <= theirs["max_ms"] and theirs["min_ms"] <= ours["max_ms"]
        res["verdict"] = "tie (the min-max ranges overlap)" if overlap else ("ours faster" if ours["median_ms"] < theirs["median_ms"] else "torch faster")
        lines.append("")
        lines.append(f"{dist}: {res['verdict']}; sum / torch glue = {ours['median_ms'] / theirs['median_ms']:.3f}")
        lines.append("")
        result[dist] = res
        del scratch, plan, leaf
        torch.cuda.empty_cache()
    key = "sum of splice (in place), forward, plan, backward"
    result["padded_over_zipf"] = result["padded"][key]["median_ms"] / result["zipf"][key]["median_ms"]
    lines.append(f"padded / zipf (sum): {result['padded_over_zipf']:.3f} (the skew bound is 1.2)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
