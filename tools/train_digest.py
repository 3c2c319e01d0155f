#!/usr/bin/env python
"""Digest of the differentiable forward (zett_amd/autograd.py): the bits of what a training step computes and the library calls it
makes, one line per item, to compare two trees on one machine with diff.  A change that only moves host code must leave every line
as it was (profiles/autograd_refactor.md).

    python tools/train_digest.py [--trace] > table.tsv        # case <tab> item <tab> sha256 of the item's bits
    python tools/train_digest.py --peak packed bf16           # torch.cuda.max_memory_allocated() of one forward + backward

Cases: the seven flag sets of tests/test_autograd_gpu.py x {packed, dense} x {f32, bf16, f16} x {deterministic, default} on two
batches of synth.workload("tiny") — 300 rows of L = 7 with fallback ids of 100 and 65 uses and one special row (the case of
tests/test_train_deterministic_gpu.py), and 8 rows of which one is all pads and one has a single position — with that test's cotangents.
deterministic: the three outputs and every parameter gradient.  default: the outputs (the forward has no atomics) and, on the dense
schedule, every gradient but the fallback rows' (its one sum of float atomics); the packed backward's default mode is covered by
--trace alone.  --trace adds one line per case: the number of zett_op_* calls of the step and the sha256 of the list of their names
with their integer and float arguments (no pointers), in call order.
"""
import argparse
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from zett_amd import _lib, synth  # noqa: E402
from zett_amd.config import ZettHypernetConfig  # noqa: E402
from zett_amd.hypernet import ZettHypernet  # noqa: E402

DEV = "cuda:0"
FLAGS = [dict(), dict(hn_embed_lang_id=False), dict(separate_out_embeddings=False), dict(hn_single_head=True), dict(hn_rescale_embeddings=False),
         dict(hn_predict_bias=False), dict(hn_single_head=True, separate_out_embeddings=False, hn_embed_lang_id=False)]
CALLS = []


class Traced:
    """the loaded library, every zett_op_* call appended to CALLS"""

    def __init__(self, lib):
        self.lib = lib

    def __getattr__(self, name):
        f = getattr(self.lib, name)
        if not name.startswith("zett_op_"):
            return f

        def call(*args):
            CALLS.append([name] + [a for a in args if isinstance(a, (int, float))])
            return f(*args)
        return call


def case(flags):
    cfg = dict(synth.workload("tiny")[0], **flags)
    ids = synth.make_surface_forms(cfg, 300, seed=61, n_special=1)
    v0, pad = cfg["original_vocab_size"], cfg["pad_token_id"]
    ids[50:150, 1] = v0 + 2
    ids[150:215, 0] = v0 + 3
    edge = ids[:8].copy()
    edge[0, :] = pad                    # an all-pad row: uniform attention when there is no language token
    edge[1, 1:] = pad                   # a row of length 1
    return cfg, synth.make_weights(cfg, seed=61), synth.make_source_embeddings(cfg, 61), {"rows300": ids, "edge8": edge}


def step(cfg, w, src, ids, packed, precision, deterministic):
    """one forward + backward -> {item: tensor}"""
    model = ZettHypernet(ZettHypernetConfig(**cfg))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    model = model.to(DEV).requires_grad_(True).train()
    model.train_packed, model.train_precision, model.train_deterministic = packed, precision, deterministic
    lang = torch.tensor(2) if cfg.get("hn_embed_lang_id") else None
    out = model(torch.from_numpy(ids).to(DEV), source_embeddings=torch.from_numpy(src).to(DEV), lang_index=lang)
    gen = torch.Generator().manual_seed(5)
    cot = [None if o is None else torch.randn(o.shape, generator=gen, dtype=torch.float64) for o in out]
    sum((o.double() * c.to(DEV)).sum() for o, c in zip(out, cot) if o is not None).backward()
    torch.cuda.synchronize()
    items = {f"out{i}": o.detach() for i, o in enumerate(out) if o is not None}
    if deterministic or not packed:
        items.update({n: p.grad for n, p in model.named_parameters() if p.grad is not None and (deterministic or n != "fallback_embeddings.weight")})
    return items


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--peak", nargs=2, metavar=("SCHEDULE", "PRECISION"))
    args = ap.parse_args()
    if args.peak:
        cfg, w, src, batches = case({})
        torch.cuda.reset_peak_memory_stats()
        step(cfg, w, src, batches["rows300"], args.peak[0] == "packed", args.peak[1], False)
        print(json.dumps({"schedule": args.peak[0], "precision": args.peak[1], "peak_bytes": torch.cuda.max_memory_allocated()}))
        return
    if args.trace:
        _lib._lib = Traced(_lib.load())
    sha = lambda b: hashlib.sha256(b).hexdigest()          # noqa: E731
    for fi, flags in enumerate(FLAGS):
        cfg, w, src, batches = case(flags)
        for batch, ids in batches.items():
            for packed in (True, False):
                for precision in ("f32", "bf16", "f16"):
                    for deterministic in (True, False):
                        name = f"flags{fi}/{batch}/{'packed' if packed else 'dense'}/{precision}/{'deterministic' if deterministic else 'default'}"
                        CALLS.clear()
                        for item, t in sorted(step(cfg, w, src, ids, packed, precision, deterministic).items()):
                            print(f"{name}\t{item}\t{sha(t.contiguous().cpu().numpy().tobytes())}")
                        if args.trace:
                            print(f"{name}\ttrace of {len(CALLS)} calls\t{sha(json.dumps(CALLS).encode())}", flush=True)


if __name__ == "__main__":
    main()
