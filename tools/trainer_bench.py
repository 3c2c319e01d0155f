#!/usr/bin/env python
"""What HypernetTrainer.fit costs per step over the same chain written out by hand: one process, the two arms alternating, one model and
one optimizer behind both.

  hand    : hypernet -> splice_special_rows -> token_embeddings -> toy backbone -> lm_head_loss + 0.5 lexical_loss -> backward -> step
  trainer : HypernetTrainer.fit over the same batches (the device window, its one read-back per repetition, the loader draw, the schedule)

    python tools/trainer_bench.py [--workload mistral_gpt2_32k] [--rows 16384] [--steps 4] [--reps 5] [--precision bf16]

A repetition is `--steps` updates between two synchronisations (wall clock; launch gaps and host work are part of a step).  Prints a table
(min - max over the repetitions, per arm) and one JSON line.  The yardstick is the hand-written chain."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from bench import device_weights  # noqa: E402
from zett_amd import synth  # noqa: E402
from zett_amd.config import ZettHypernetConfig  # noqa: E402
from zett_amd.hypernet import ZettHypernet  # noqa: E402
from zett_amd.trainer import HypernetTrainer  # noqa: E402
from zett_amd.training import HypernetAdamW, lexical_loss, lm_head_loss, splice_special_rows, token_embeddings  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="mistral_gpt2_32k", choices=sorted(synth.WORKLOADS))
    ap.add_argument("--rows", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=["f32", "bf16", "f16"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq", type=int, default=128)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg, _rows, src_dtype, hist = synth.workload(args.workload)
    rows, e = args.rows, cfg["n_embd"]
    model = ZettHypernet(ZettHypernetConfig(**cfg)).to(dev)
    with torch.no_grad():
        for name, w in device_weights(cfg, dev, seed=0).items():
            dict(model.named_parameters())[name].copy_(w)
    model.requires_grad_(True).train()
    model.train_precision = args.precision
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}[args.precision]
    src = torch.from_numpy(synth.make_source_embeddings(cfg, seed=0, dtype=src_dtype)).to(dev)
    pad = cfg["pad_token_id"]
    gen = torch.Generator(device=dev).manual_seed(0)
    mix = (torch.randn(e, e, device=dev, generator=gen) / e ** 0.5).to(dtype)

    def backbone(x, attention_mask=None):
        return x + torch.tanh(x @ mix)

    batches = []
    for i in range(2):
        ids = torch.randint(0, rows, (args.batch, args.seq), device=dev, generator=gen)
        batches.append({"target_surface_forms": torch.from_numpy(synth.make_surface_forms(cfg, rows, seed=i, hist=hist)).to(dev), "input_ids": ids, "labels": ids,
                        "attention_mask": torch.ones_like(ids), "target_priors": torch.zeros(rows, device=dev), "mask": torch.ones(rows, dtype=torch.bool, device=dev),
                        "special_indices": [0, 1, 2], "special_indices_in_reference": [0, 1, 2], "lang_index": torch.tensor(0), "lang_code": "en",
                        "metrics": {"avg_byte_length": torch.tensor(4.0, dtype=torch.float64, device=dev), "unk_ratio": torch.tensor(0.0, dtype=torch.float64, device=dev)}})
    training_args = dict(steps=args.steps, logging_steps=args.steps, warmup_steps=0, learning_rate=6e-5, learning_rate_alpha=1.0, lexical_loss_weight=0.5, loss="clm")
    opt = HypernetAdamW(model, lr=6e-5, betas=(0.9, 0.95), weight_decay=0.01, max_grad_norm=0.1)
    trainer = HypernetTrainer(model, backbone, src, training_args, hn_pad_token_id=pad, optimizer=opt, lm_precision=args.precision, embed_dtype=dtype, langs=["en"])
    logged = []

    def hand():
        for step in range(args.steps):
            batch = batches[step % len(batches)]
            pred_in, pred_out, _ = model(batch["target_surface_forms"], source_embeddings=src, lang_index=batch["lang_index"])
            pred_in, pred_out = splice_special_rows(pred_in, pred_out, src, batch["special_indices"], batch["special_indices_in_reference"], inplace=True)
            hidden = backbone(token_embeddings(pred_in, batch["input_ids"], dtype=dtype, check_ids=False))
            lm, _ = lm_head_loss(hidden, pred_out if pred_out is not None else pred_in, batch["labels"], batch["attention_mask"], mode="clm", priors=batch["target_priors"],
                                 vocab_mask=batch["mask"], precision=args.precision)
            lex, _ = lexical_loss(pred_in, pred_out, src, batch["target_surface_forms"], pad)
            (lm + 0.5 * lex).backward()
            opt.step(lr=6e-5, zero_grad=True)

    def fit():
        trainer.micro_step = 0
        trainer.fit([batches], [1.0], log=lambda metrics, step: logged.append(metrics))

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / args.steps * 1e3

    hand(), fit()          # warm-up: allocations, moments, engines
    ms = {"hand": [], "trainer": []}
    for _ in range(args.reps):
        ms["hand"].append(timed(hand))
        ms["trainer"].append(timed(fit))
    print(f"| {args.workload}, {rows} rows, {args.batch} x {args.seq} tokens, {args.precision}, {args.steps} updates per repetition, {args.reps} repetitions | ms per step (min - max) |")
    print("|---|---:|")
    for arm, values in ms.items():
        print(f"| {arm} | {min(values):.2f} - {max(values):.2f} |")
    print(json.dumps({"metric": "ms per training step, hand-written chain against HypernetTrainer.fit", "workload": args.workload, "rows": rows, "precision": args.precision,
                      "steps": args.steps, "reps": args.reps, "ms_per_step": ms, "last_window": logged[-1] if logged else None}))


if __name__ == "__main__":
    main()
