#!/usr/bin/env python
"""Digest of the differentiable forward (zett_amd/autograd.py): the bits of what a training step computes and the library calls it
makes, one line per item, to compare two trees on one machine with diff.  A change that only moves host code must leave every line
as it was (profiles/autograd_refactor.md).

    python tools/train_digest.py [--trace] > table.tsv        # case <tab> item <tab> sha256 of the item's bits
    python tools/train_digest.py --peak packed bf16           # torch.cuda.max_memory_allocated() of one forward + backward
    python tools/train_digest.py --optimizer > table.tsv      # the optimizer step instead (zett_amd/optim.py): see optimizer_digest

The script imports the tree it lies in: to digest another tree (a parent commit with its own build), copy this file into that tree's
tools/ and run it there.  --optimizer needs only names that zett_amd.training has exported since Adafactor was added.

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


class Bag(torch.nn.Module):
    """parameters t000, t001, ... and the refresh_weights() an optimizer asks of its model"""

    def __init__(self, tensors):
        super().__init__()
        for i, t in enumerate(tensors):
            self.register_parameter(f"t{i:03d}", torch.nn.Parameter(t))

    def refresh_weights(self):
        pass


def optimizer_digest():
    """Both optimizers over three steps on the tensor lists of the direct GPU tests (tests/loss_step_check.mt_list, tests/adafactor_check
    mixed_list + single_cases: chunk and tile edges, pointers 4 bytes off a 16-byte boundary, frozen and empty tensors, more tensors than
    either unit's launch group), with zero_grad on and off.  Step 0 is clipped, step 1 has an infinite gradient and is skipped, step 2 is
    below max_grad_norm.  One line per parameter, state tensor and gradient after every step, and one for the record's eight words."""
    from tests import adafactor_check as ac
    from tests import loss_step_check as lc
    from zett_amd.training import HypernetAdafactor, HypernetAdamW, adafactor_state_shapes
    label = {lc.DECAY: "decay", 0: "no_decay", lc.FROZEN: "frozen"}
    entries = [((e["n"],), e["flags"], e["off"][:2], e["off"][2:]) for e in lc.mt_list()]
    entries += [(e["shape"], e["flags"], e["off"][:2], e["off"][2:] * 2) for e in ac.mixed_list() + ac.single_cases()]
    sha = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()          # noqa: E731

    def at(shape, off, gen=None, scale=1.0):
        """a contiguous device tensor of `shape` that starts `off` elements into its allocation"""
        n = 1
        for s in shape:
            n *= s
        buf = torch.zeros(n + off, device=DEV)
        if gen is not None:
            buf[off:] = (torch.randn(n, generator=gen) * scale).to(DEV)
        return buf[off:].view(shape)

    gen = torch.Generator().manual_seed(77)
    grads = [[torch.randn(shape, generator=gen) * scale for shape, *_ in entries] for scale in (0.1, 0.1, 1e-5)]
    poisoned = next(i for i, (shape, flags, *_) in enumerate(entries) if flags != lc.FROZEN and min(shape) >= 128)
    grads[1][poisoned].view(-1)[5] = float("inf")
    max_norm = 0.01 * float(torch.sqrt(sum((g.double() ** 2).sum() for g in grads[0])))
    for name, cls in (("adamw", HypernetAdamW), ("adafactor", HypernetAdafactor)):
        for zero_grad in (True, False):
            gen = torch.Generator().manual_seed(78)
            model = Bag([at(shape, off[0], gen, 0.5) for shape, _, off, _ in entries])
            names = [n for n, _ in model.named_parameters()]
            opt = cls(model, lr=1e-2, weight_decay=0.01, max_grad_norm=max_norm, labels={n: label[e[1]] for n, e in zip(names, entries)})
            for (n, p), (shape, flags, off, state_off) in zip(model.named_parameters(), entries):
                p.grad = at(shape, off[1])
                if flags != lc.FROZEN:          # the states start where the tests' do: the optimizer takes what is there
                    shapes = adafactor_state_shapes(shape) if cls is HypernetAdafactor else {"exp_avg": shape, "exp_avg_sq": shape}
                    opt.state[n] = {k: at(s, o) for (k, s), o in zip(shapes.items(), state_off)}
            for step in range(3):
                for p, g in zip(model.parameters(), grads[step]):
                    p.grad.copy_(g)
                opt.step(zero_grad=zero_grad)
                torch.cuda.synchronize()
                case = f"{name}/{'zero_grad' if zero_grad else 'keep_grad'}/step{step}"
                words = (opt.record if hasattr(opt, "record") else opt._record).cpu()          # (a tree from before the accessor: to compare it with this one)
                stats = opt.last_step_stats()
                assert (stats["skipped"], stats["clip_coef"] < 1.0, stats["step"]) == ((0, True, 1), (1, True, 1), (0, False, 2))[step], (case, stats)
                print(f"{case}\trecord\t{sha(words)}\t{words.view(torch.int32).tolist()}")
                for n, p in model.named_parameters():
                    print(f"{case}\t{n}\t{sha(p.detach())}\n{case}\t{n}.grad\t{sha(p.grad)}")
                    for k, t in sorted(opt.state.get(n, {}).items()):
                        print(f"{case}\t{n}.{k}\t{sha(t)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--optimizer", action="store_true")
    ap.add_argument("--peak", nargs=2, metavar=("SCHEDULE", "PRECISION"))
    args = ap.parse_args()
    if args.optimizer:
        return optimizer_digest()
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
