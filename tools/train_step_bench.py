#!/usr/bin/env python
"""What zett_amd/training.py saves around the differentiable forward: one identity warm-up step's LOSS-AND-GRADIENT (from the
predicted embeddings to their gradients) and its OPTIMIZER STEP (clip by global norm + AdamW over every hypernetwork
parameter), each timed two ways in one process, with HIP events, on the same tensors:

  torch : the glue a user writes without this module — index_select of the target rows, torch element-wise loss, autograd,
          the optax-style clip in torch (_foreach_norm, a device-side coefficient, _foreach_mul_) and torch.optim.AdamW(fused=True)
  hip   : zett_amd.training.identity_loss (csrc/train_dist.hip) / zett_amd.optim.HypernetAdamW.step (csrc/train_step.hip)

    python tools/train_step_bench.py [--workload mistral_gpt2_32k] [--rows N] [--steps K] [--warmup W]

The hypernetwork's own forward and backward are the same in both and are not run (tools/train_bench.py times them): the
predictions and the parameter gradients are random tensors of the workload's shapes.  Prints a table and one JSON line.  The
AdamW pass moves 28 bytes per parameter (reads p, g, m, v; writes p, m, v), 32 with the fused zeroing of g.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from zett_amd import synth  # noqa: E402
from zett_amd.config import ZettHypernetConfig  # noqa: E402
from zett_amd.hypernet import ZettHypernet  # noqa: E402
from zett_amd.training import HypernetAdamW, identity_loss, param_labels  # noqa: E402

COPY_ROOF_TBS = 6.29          # measured float4-copy rate of the MI355X


def timed(fn, steps, warmup):
    """mean milliseconds of fn() between HIP events (all steps in one event pair: launch gaps are part of a step)"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="mistral_gpt2_32k", choices=sorted(synth.WORKLOADS))
    ap.add_argument("--rows", type=int, default=0)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg, rows, src_dtype, _hist = synth.workload(args.workload)
    rows = args.rows or rows
    e, lr, betas, eps, wd, max_norm = cfg["n_embd"], 6e-5, (0.9, 0.95), 1e-8, 0.01, 0.1
    gen = torch.Generator(device=dev).manual_seed(0)

    # ---- loss and gradient -------------------------------------------------------------------------------------------------
    separate = bool(cfg.get("separate_out_embeddings"))
    src = (torch.randn(cfg["original_vocab_size"], e * (2 if separate else 1), device=dev, generator=gen) * 0.02).to(getattr(torch, src_dtype))
    ids = torch.randint(0, cfg["original_vocab_size"], (rows,), device=dev, generator=gen)
    pred_in = (torch.randn(rows, e, device=dev, generator=gen) * 0.02).requires_grad_(True)
    pred_out = (torch.randn(rows, e, device=dev, generator=gen) * 0.02).requires_grad_(True) if separate else None

    def torch_loss():
        pred_in.grad = None
        if separate:
            pred_out.grad = None
        target = src.index_select(0, ids).float()
        loss = torch.square(pred_in - target[:, :e]).sum(-1).mean()
        if separate:
            loss = (loss + torch.square(pred_out - target[:, e:]).sum(-1).mean()) / 2.0
        loss.backward()
        return loss

    def hip_loss():
        pred_in.grad = None
        if separate:
            pred_out.grad = None
        loss = identity_loss(pred_in, pred_out, src, ids)
        loss.backward()
        return loss

    a, b = torch_loss(), hip_loss()
    loss_rel = abs(float(a.detach()) - float(b.detach())) / abs(float(a.detach()))
    loss_ms = {"torch": timed(torch_loss, args.steps, args.warmup), "hip": timed(hip_loss, args.steps, args.warmup)}

    # ---- optimizer step ----------------------------------------------------------------------------------------------------
    model = ZettHypernet(ZettHypernetConfig(**cfg)).to(dev).requires_grad_(True).train()
    labels = param_labels(model)
    n_params = sum(p.numel() for p in model.parameters())
    n_updated = sum(p.numel() for n, p in model.named_parameters() if labels[n] != "frozen")
    for p in model.parameters():
        p.grad = torch.randn(p.shape, device=dev, generator=gen) * 1e-3
    twin = {n: torch.nn.Parameter(p.detach().clone()) for n, p in model.named_parameters()}
    for n, p in model.named_parameters():
        twin[n].grad = p.grad.clone()
    ref = torch.optim.AdamW([{"params": [twin[n] for n, l in labels.items() if l == "decay"], "weight_decay": wd},
                             {"params": [twin[n] for n, l in labels.items() if l == "no_decay"], "weight_decay": 0.0}], lr=lr, betas=betas, eps=eps, fused=True)
    twin_grads = [p.grad for p in twin.values()]

    def torch_clip():
        norm = torch.linalg.vector_norm(torch.stack(torch._foreach_norm(twin_grads)))
        coef = torch.where(norm < max_norm, torch.ones_like(norm), max_norm / norm)          # optax.clip_by_global_norm, on the device
        torch._foreach_mul_(twin_grads, coef)

    def torch_step():
        torch_clip()
        ref.step()

    opt = HypernetAdamW(model, lr=lr, betas=betas, eps=eps, weight_decay=wd, max_grad_norm=max_norm)
    # the two launches of step() are timed one by one as well (HypernetAdamW.launch_norm, launch_adamw), on tensor lists collected
    # once (the pointers do not change here).  The bias corrections move with the device step count, the work per element does not.
    lists = opt.collect()
    opt_ms = {"torch clip": timed(torch_clip, args.steps, args.warmup), "torch adamw(fused)": timed(ref.step, args.steps, args.warmup),
              "torch clip + adamw": timed(torch_step, args.steps, args.warmup),
              "hip norm": timed(lambda: opt.launch_norm(lists), args.steps, args.warmup),
              "hip adamw": timed(lambda: opt.launch_adamw(lists), args.steps, args.warmup),
              "hip step": timed(opt.step, args.steps, args.warmup)}
    stats = opt.last_step_stats()
    stats.pop("step")          # (every timed call of the norm entry point advanced the device step count: not a count of real steps)
    opt_ms["hip adamw + zero_grad"] = timed(lambda: opt.launch_adamw(lists, zero_grad=True), args.steps, args.warmup)      # (last: it clears the gradients)
    tbs = {"hip adamw": 28.0 * n_updated / (opt_ms["hip adamw"] * 1e-3) / 1e12, "hip adamw + zero_grad": 32.0 * n_updated / (opt_ms["hip adamw + zero_grad"] * 1e-3) / 1e12,
           "hip norm": 4.0 * n_params / (opt_ms["hip norm"] * 1e-3) / 1e12, "torch adamw(fused)": 28.0 * n_updated / (opt_ms["torch adamw(fused)"] * 1e-3) / 1e12}

    print(f"| {args.workload}, {rows} rows x {e} columns ({src_dtype} source), {n_params / 1e6:.1f} M parameters | ms | TB/s |")
    print("|---|---:|---:|")
    print(f"| loss + gradient, torch glue | {loss_ms['torch']:.3f} | |")
    print(f"| loss + gradient, identity_loss | {loss_ms['hip']:.3f} | |")
    for k, v in opt_ms.items():
        print(f"| {k} | {v:.3f} | {('%.2f' % tbs[k]) if k in tbs else ''} |")
    print(json.dumps({"metric": "identity warm-up step outside the hypernetwork forward / backward", "workload": args.workload, "rows": rows, "n_embd": e,
                      "parameters": n_params, "updated_parameters": n_updated, "loss_grad_ms": loss_ms, "loss_rel_diff": loss_rel, "optimizer_ms": opt_ms,
                      "achieved_tb_per_s": tbs, "copy_roof_tb_per_s": COPY_ROOF_TBS, "adamw_floor_ms": 28.0 * n_updated / (COPY_ROOF_TBS * 1e12) * 1e3,
                      "last_step": stats, "steps": args.steps, "warmup": args.warmup}))


if __name__ == "__main__":
    main()
