#!/usr/bin/env python
"""The optimizer step of the hypernetwork three ways in one process, at a workload's parameter shapes, on the same gradients:

  adamw     : zett_amd.training.HypernetAdamW.step (csrc/train_step.hip; tools/train_step_bench.py's "hip step")
  adafactor : zett_amd.training.HypernetAdafactor.step (csrc/train_adafactor.hip)
  torch     : the glue a user writes without it — the optax-style clip in torch (_foreach_norm, a device-side coefficient,
              _foreach_mul_) and transformers.optimization.Adafactor(scale_parameter=True, relative_step=False) on the device

    python tools/adafactor_bench.py [--workload mistral_gpt2_32k] [--reps 10] [--warmup 3] [--arms adamw,adafactor,torch]

The arms ALTERNATE (one step of each per round), every step between its own pair of HIP events; min, median and max per arm are
printed, with the bytes of optimizer state each arm holds and the bytes the Adafactor passes move per step, from the shapes:

  pass 1  reads g and p                      8 B per updated parameter, 4 B per frozen one
  pass 2  reads g (flat: and v, writes v)    4 B per factored parameter, 12 B per flat one
  pass 3  reads g and p, writes p            12 B per factored parameter, 16 B per flat one (flat: v is read again)
          (+ 4 B per parameter with zero_grad; the partial sums between the passes are below 1 % of this)

`--arms adafactor` runs that arm alone: what a kernel trace is taken on.  Prints a table and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from zett_amd import synth  # noqa: E402
from zett_amd.config import ZettHypernetConfig  # noqa: E402
from zett_amd.hypernet import ZettHypernet  # noqa: E402
from zett_amd.training import HypernetAdafactor, HypernetAdamW, adafactor_state_shapes, param_labels  # noqa: E402

COPY_ROOF_TBS = 6.29          # measured float4-copy rate of the MI355X (profiles/train_step.md)


def state_bytes(state):
    return sum(t.numel() * t.element_size() for st in state.values() for t in st.values() if torch.is_tensor(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="mistral_gpt2_32k", choices=sorted(synth.WORKLOADS))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--arms", default="adamw,adafactor,torch")
    args = ap.parse_args()
    arms = [a for a in args.arms.split(",") if a]
    dev = torch.device("cuda", 0)
    cfg, _rows, _src_dtype, _hist = synth.workload(args.workload)
    lr, wd, max_norm = 6e-5, 0.01, 0.1
    gen = torch.Generator(device=dev).manual_seed(0)

    def fresh():
        model = ZettHypernet(ZettHypernetConfig(**cfg)).to(dev).requires_grad_(True).train()
        for p in model.parameters():
            p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
        return model

    steps, states = {}, {}
    labels = None
    if "adamw" in arms:
        m = fresh()
        labels = param_labels(m)
        opt = HypernetAdamW(m, lr=lr, weight_decay=wd, max_grad_norm=max_norm)
        steps["adamw"], states["adamw"] = opt.step, (lambda opt=opt: state_bytes(opt.state))
    if "adafactor" in arms:
        m = fresh()
        labels = param_labels(m)
        opt2 = HypernetAdafactor(m, lr=lr, weight_decay=wd, max_grad_norm=max_norm)
        steps["adafactor"], states["adafactor"] = opt2.step, (lambda: state_bytes(opt2.state))
    if "torch" in arms:
        from transformers.optimization import Adafactor
        m = fresh()
        labels = param_labels(m)
        named = dict(m.named_parameters())
        kw = dict(lr=lr, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, scale_parameter=True, relative_step=False, warmup_init=False)
        ref = Adafactor([{"params": [named[n] for n, l in labels.items() if l == "decay"], "weight_decay": wd},
                         {"params": [named[n] for n, l in labels.items() if l == "no_decay"], "weight_decay": 0.0}], **kw)
        grads = [p.grad for p in m.parameters()]

        def torch_step():
            norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(grads)))
            coef = torch.where(norm < max_norm, torch.ones_like(norm), max_norm / norm)          # optax.clip_by_global_norm, on the device
            torch._foreach_mul_(grads, coef)
            ref.step()

        steps["torch"], states["torch"] = torch_step, (lambda: state_bytes(ref.state))

    shapes = [(tuple(p.shape), labels[n]) for n, p in m.named_parameters()]
    count = {"factored": 0, "flat": 0, "frozen": 0}
    for shape, label in shapes:
        n = 1
        for s in shape:
            n *= s
        count["frozen" if label == "frozen" else ("factored" if "v_row" in adafactor_state_shapes(shape) else "flat")] += n
    pass_bytes = {"pass 1": 8 * (count["factored"] + count["flat"]) + 4 * count["frozen"], "pass 2": 4 * count["factored"] + 12 * count["flat"],
                  "pass 3": 12 * count["factored"] + 16 * count["flat"]}
    moved = sum(pass_bytes.values())

    for _ in range(args.warmup):
        for arm in arms:
            steps[arm]()
    torch.cuda.synchronize()
    ms = {arm: [] for arm in arms}
    for _ in range(args.reps):
        for arm in arms:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            steps[arm]()
            b.record()
            torch.cuda.synchronize()
            ms[arm].append(a.elapsed_time(b))
    summary = {arm: {"min_ms": min(v), "median_ms": statistics.median(v), "max_ms": max(v), "state_bytes": states[arm]()} for arm, v in ms.items()}
    n_params = sum(count.values())
    print(f"| {args.workload}: {n_params / 1e6:.1f} M parameters in {len(shapes)} tensors ({count['factored'] / 1e6:.1f} M factored, {count['flat'] / 1e6:.2f} M flat, "
          f"{count['frozen'] / 1e6:.3f} M frozen), {args.reps} alternating repetitions | min ms | median ms | max ms | optimizer state |")
    print("|---|---:|---:|---:|---:|")
    for arm, s in summary.items():
        print(f"| {arm} | {s['min_ms']:.3f} | {s['median_ms']:.3f} | {s['max_ms']:.3f} | {s['state_bytes'] / 1e6:.1f} MB |")
    out = {"metric": "optimizer step of the hypernetwork", "workload": args.workload, "parameters": n_params, "elements": count, "arms": summary, "reps": args.reps,
           "warmup": args.warmup, "adafactor_pass_bytes": pass_bytes, "adafactor_bytes_per_step": moved, "copy_roof_tb_per_s": COPY_ROOF_TBS,
           "adafactor_floor_ms": moved / (COPY_ROOF_TBS * 1e12) * 1e3}
    if "adafactor" in summary:
        out["adafactor_tb_per_s"] = moved / (summary["adafactor"]["median_ms"] * 1e-3) / 1e12
        print(f"| adafactor: {moved / 1e9:.2f} GB per step ({moved / max(n_params, 1):.1f} B per parameter) | | {out['adafactor_tb_per_s']:.2f} TB/s | | floor {out['adafactor_floor_ms']:.2f} ms at {COPY_ROOF_TBS} TB/s |")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
