#!/usr/bin/env python
"""The batch's sub-vocabulary (collator.py:207-282 of the reference) timed three ways in one process on the same inputs (the reference's
training shape: 128 x 128 = 16 384 positions, N = n_token_subsample = 16 384, L = 7, Zipf-like ids, 8 special ids, mode "random"; a
vocabulary of 32 768 and of 262 144 ids):

  hip   : zett_amd.training.subsample_batch_vocabulary(check=False) (csrc/train_batch.hip) — no host read
  numpy : the restatement of tests/batch_vocab_ref.py on host arrays plus the host-to-device copies of its outputs (what the collator does today)
  torch : the most direct restatement with torch on the device — torch.unique, torch.isin, boolean indexing (each a host read of a size), index ops

    python tools/batch_vocab_bench.py [--t 16384] [--v 32768 262144] [--n 16384] [--l 7] [--steps 10] [--warmup 3] [--out FILE.md]

The three are first compared member by member (torch.equal).  Per vocabulary the variants ALTERNATE (one repetition of each in turn), 3
warm-up and 10 timed repetitions; every repetition is timed with a HIP event pair AND with the host clock around it (start after a
synchronize, stop after the next): the numpy path does its work on the host, so only the host clock sees it, and the torch path waits for
the host inside, so its event time contains those waits.  Prints a markdown table, the bytes each pass of the HIP path moves, and one
JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests.batch_vocab_ref import batch_vocab_ref  # noqa: E402
from zett_amd import training  # noqa: E402

MEMBERS = ("input_ids", "labels", "ids_to_embed", "target_surface_forms", "target_priors", "mask")


def measure(variants, steps, warmup):
    """One repetition of every variant in turn; -> name -> (event ms, host-clock ms) lists of the timed repetitions."""
    ev, wall = {k: [] for k in variants}, {k: [] for k in variants}
    for rep in range(warmup + steps):
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rep >= warmup:
                ev[name].append(a.elapsed_time(b))
                wall[name].append((t1 - t0) * 1e3)
    return ev, wall


def torch_glue(ids, labels, special, moves, n, sf, priors, order):
    """The definition with torch's own operators on the device: sizes come back to the host wherever a result's length depends on data."""
    flat = labels.reshape(-1)
    uniq = torch.unique(torch.cat([ids.reshape(-1), flat[flat != -100]]))
    tokens = torch.cat([special, uniq[~torch.isin(uniq, special)]])
    lst = torch.cat([tokens, order[~torch.isin(order, tokens)][:n - tokens.numel()]])
    for frm, to in moves:          # del / insert per special id
        x = lst[frm:frm + 1]
        lst = torch.cat([lst[:frm], lst[frm + 1:]])
        lst = torch.cat([lst[:to], x, lst[to:]])
    inv = torch.zeros(priors.numel(), dtype=torch.int64, device=ids.device)
    inv[lst] = torch.arange(n, device=ids.device)
    out_labels = torch.where(labels != -100, inv[labels.clamp(min=0)], labels)
    return inv[ids], out_labels, lst, sf[lst], priors[lst], torch.ones(n, dtype=torch.bool, device=ids.device)


def pass_bytes(t, v, n, l, ids_b=8, sf_b=8, order_b=8):
    """algorithmic bytes of each launch of the HIP path, mode "random" """
    return {
        "batch_init_kernel": 8 * v,                                                        # flags and inv written
        "batch_mark_kernel": 2 * ids_b * t + 2 * 4 * t,                                    # both id arrays read, a flag word read per id (an OR only where it is not set yet)
        "batch_count_kernel": 4 * v + order_b * v + 4 * v,                                 # flags in id order, negative_order, flags gathered through it
        "batch_scan_kernel": 4 * 4 * ((v + 1023) // 1024),
        "batch_place_kernel": 4 * v + order_b * v + 4 * v + 4 * n,                         # the same reads, the two lists written (n entries between them)
        "batch_rows_kernel": n * (4 + ids_b + 4 + 4 + 1 + 4) + 2 * n * l * sf_b,           # list entry, id, prior in and out, mask, inv max; the surface-form rows in and out
        "batch_remap_kernel": t * (4 * ids_b + 2 * 4),                                     # both arrays in and out, an inv word per id
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--t", type=int, default=16384)
    ap.add_argument("--v", type=int, nargs="+", default=[32768, 262144])
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--l", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    t, n, l = args.t, args.n, args.l
    result = {"metric": "batch sub-vocabulary, mode random", "t": t, "n": n, "l": l, "steps": args.steps, "warmup": args.warmup}
    lines = []
    for v in args.v:
        rng = np.random.default_rng(1234)
        ids_h = np.minimum(np.floor(v * rng.random(t) ** 3).astype(np.int64), v - 1).reshape((128, -1) if t % 128 == 0 else (-1,))
        labels_h = ids_h.copy()
        labels_h[rng.random(ids_h.shape) < 0.1] = -100
        special = [1, 0, 2, 3, 4, 5, 6, v - 1]          # the last one at the end of the vocabulary, as GPT-2's <|endoftext|>
        sf_h = rng.integers(0, 50000, (v, l)).astype(np.int64)
        priors_h = rng.standard_normal(v).astype(np.float32)
        order_h = rng.permutation(v).astype(np.int64)
        ids, labels, sf, priors, order = (torch.from_numpy(x).to(dev) for x in (ids_h, labels_h, sf_h, priors_h, order_h))
        special_t = torch.tensor(special, device=dev)
        moves, _ = training.special_row_moves(special, n)

        def hip(check=False, mode="random"):
            return training.subsample_batch_vocabulary(ids, labels, special, n, sf, priors, mode=mode, negative_order=order, check=check)

        def numpy_path():
            out = batch_vocab_ref(ids_h, labels_h, special, n, sf_h, priors_h, "random", order_h)
            return [torch.from_numpy(np.ascontiguousarray(out[k])).to(dev) for k in MEMBERS]

        def torch_path():
            return torch_glue(ids, labels, special_t, moves, n, sf, priors, order)

        bv = hip(check=True)
        for name, other in (("numpy", numpy_path()), ("torch", torch_path())):
            for key, x in zip(MEMBERS, other):
                assert torch.equal(getattr(bv, key), x), (v, name, key)
        variants = {"hip, check=False": hip, "hip, check=True (one host read)": lambda: hip(True), "hip, positives_only, check=False": lambda: hip(False, "positives_only"),
                    "numpy restatement + host-to-device copies": numpy_path, "torch on the device": torch_path}
        ev, wall = measure(variants, args.steps, args.warmup)
        res = {"n_positive": int(bv.n_positive)}
        lines.append(f"| V = {v}: {res['n_positive']} ids in the batch | events: median ms | min | max | host clock: median ms | min | max |")
        lines.append("|---|---:|---:|---:|---:|---:|---:|")
        for name in variants:
            e, w = ev[name], wall[name]
            res[name] = {"event_median_ms": statistics.median(e), "event_min_ms": min(e), "event_max_ms": max(e),
                         "wall_median_ms": statistics.median(w), "wall_min_ms": min(w), "wall_max_ms": max(w)}
            lines.append(f"| {name} | {statistics.median(e):.3f} | {min(e):.3f} | {max(e):.3f} | {statistics.median(w):.3f} | {min(w):.3f} | {max(w):.3f} |")
        ours, theirs = res["hip, check=False"], res["torch on the device"]
        overlap = ours["wall_min_ms"] <= theirs["wall_max_ms"] and theirs["wall_min_ms"] <= ours["wall_max_ms"]
        res["verdict"] = "tie (the min-max ranges overlap)" if overlap else ("hip faster" if ours["wall_median_ms"] < theirs["wall_median_ms"] else "torch faster")
        lines.append("")
        lines.append(f"V = {v}: {res['verdict']}; hip / torch = {ours['wall_median_ms'] / theirs['wall_median_ms']:.3f}, "
                     f"hip / numpy = {ours['wall_median_ms'] / res['numpy restatement + host-to-device copies']['wall_median_ms']:.4f} (host clock)")
        lines.append("")
        lines.append(f"| pass, V = {v} | algorithmic bytes |")
        lines.append("|---|---:|")
        for k, b in pass_bytes(t, v, n, l).items():
            lines.append(f"| `{k}` | {b} |")
        lines.append("")
        result[f"v{v}"] = res
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
