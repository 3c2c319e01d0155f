#!/usr/bin/env python
"""The rest of the collator (collator.py:180-205 and 283-337 of the reference, and the whole ``Collator.__call__``) timed in one process on the
same inputs, at the reference's training shape: 128 rows x 128 positions = 16 384 positions, a vocabulary of 32 768 ids, L = 7, Zipf-like
ids, 5 special ids.

  label_batch, mlm and clm
    hip   : zett_amd.collate.label_batch(check=False) (csrc/train_batch.hip, two launches) — no host read
    numpy : the installed DataCollatorForLanguageModeling(return_tensors="np") with numpy's own generator (clm: a copy), the reference's
            metrics lines, and the host-to-device copies of input_ids, labels, byte_lengths and the two metrics
    torch : the same arithmetic (the same counter-based draws) with torch's operators on the device
  the vocabulary behind it, subsampled (N = 16 384) and padded
    hip   : subsample_batch_vocabulary(check=False) / pad_vocabulary
    numpy : tests/batch_vocab_ref.py / numpy.pad, and the copies
    torch : (padded only) torch.cat with constant blocks on the device
  a whole DeviceCollator call against the host path it replaces (the converted tokenizer's own call, the numpy restatement, the copies): at
  the vocabulary of the test tokenizer (554 ids), the only tokenizer the repository carries; 128 texts, block_size 128

    python tools/collate_bench.py [--steps 10] [--warmup 3] [--out FILE.md]

Outputs are compared (torch.equal) first wherever they are defined equal: hip against torch always, hip against numpy with the counter-based
generator injected into the library (the TIMED numpy path draws from numpy's generator, as the reference does).  The variants of a group
ALTERNATE and the starting variant rotates from one repetition to the next, 3 warm-up and 10 timed repetitions; a repetition is timed with a HIP event pair and with the host clock between two
synchronisations (the numpy paths work on the host: only the host clock sees them).  Prints markdown tables and one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from tests import collate_ref as cr  # noqa: E402
from tests.batch_vocab_ref import batch_vocab_ref  # noqa: E402
from zett_amd import collate, training  # noqa: E402


def measure(variants, steps, warmup):
    ev, wall = {k: [] for k in variants}, {k: [] for k in variants}
    names = list(variants)
    for rep in range(warmup + steps):
        for name in names[rep % len(names):] + names[:rep % len(names)]:          # the starting variant rotates: no variant always runs behind the same one
            fn = variants[name]
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


def table(title, variants, steps, warmup, lines, result):
    ev, wall = measure(variants, steps, warmup)
    lines.append(f"| {title} | events: median ms | min | max | host clock: median ms | min | max |")
    lines.append("|---|---:|---:|---:|---:|---:|---:|")
    res = {}
    for name in variants:
        e, w = ev[name], wall[name]
        res[name] = {"event_median_ms": statistics.median(e), "event_min_ms": min(e), "event_max_ms": max(e), "wall_median_ms": statistics.median(w), "wall_min_ms": min(w),
                     "wall_max_ms": max(w)}
        lines.append(f"| {name} | {statistics.median(e):.3f} | {min(e):.3f} | {max(e):.3f} | {statistics.median(w):.3f} | {min(w):.3f} | {max(w):.3f} |")
    lines.append("")
    result[title] = res


# ---- the labelling arithmetic with torch's operators: uint64 as int64 bit patterns --------------------------------------------------------------
def _i64(x):
    x &= (1 << 64) - 1
    return x - (1 << 64) if x >= 1 << 63 else x


def _lsr(x, k):
    return (x >> k) & ((1 << (64 - k)) - 1)


def _mix64(x):
    x = (x ^ _lsr(x, 30)) * _i64(0xBF58476D1CE4E5B9)
    x = (x ^ _lsr(x, 27)) * _i64(0x94D049BB133111EB)
    return x ^ _lsr(x, 31)


def torch_label(ids, special_t, table_t, vocab_len, mask_id, unk_id, seed, thresholds, mlm):
    t = ids.numel()
    flat = ids.reshape(-1)
    out = flat.clone()
    if mlm:
        p = torch.arange(t, dtype=torch.int64, device=ids.device)
        h = [_mix64(p ^ _i64(k)) for k in cr.keys(seed)]
        k = [_lsr(x, 11) for x in h[:3]]
        masked = ~torch.isin(flat, special_t) & (k[0] < thresholds[0])
        replaced = masked & (k[1] < thresholds[1])
        random = masked & ~replaced & (k[2] < thresholds[2])
        labels = torch.where(masked, flat, -100)
        word = ((_lsr(h[3], 1) % vocab_len) * 2 + (h[3] & 1)) % vocab_len          # an unsigned 64-bit word modulo vocab_len
        out = torch.where(replaced, mask_id, torch.where(random, word, flat))
    else:
        labels = flat.clone()
    lengths = table_t[out]
    plain = ~torch.isin(out, special_t)
    metrics = torch.stack([(lengths * plain).sum().double() / plain.sum().double(), (out == unk_id).sum().double() / t])
    return out.view_as(ids), labels.view_as(ids), lengths.view_as(ids), metrics


class _Tokenizer:
    mask_token, pad_token, padding_side = "<mask>", "<pad>", "right"

    def __init__(self, vocab_len, special, mask_id, unk_id):
        self.vocab_len, self.all_special_ids, self.mask_token_id, self.unk_token_id, self.pad_token_id = vocab_len, list(special), mask_id, unk_id, special[0]
        self._special = np.zeros(vocab_len, dtype=bool)
        self._special[special] = True

    def __len__(self):
        return self.vocab_len

    def get_special_tokens_mask(self, ids, already_has_special_tokens=False):
        return self._special[np.asarray(ids)].astype(np.int64).tolist()

    def convert_tokens_to_ids(self, token):
        return self.mask_token_id


def numpy_label(ids_h, tokenizer, table_h, dev, mlm, generator=None):
    """collator.py:180-205 as the reference runs it, and the copies"""
    if mlm:
        from transformers import DataCollatorForLanguageModeling
        inner = DataCollatorForLanguageModeling(tokenizer, mlm=True, return_tensors="np")
        inner.generator = generator
        enc = inner(ids_h.copy())
        input_ids, labels = enc["input_ids"], enc["labels"]
    else:
        input_ids, labels = ids_h, ids_h.copy()
    plain = np.isin(input_ids, tokenizer.all_special_ids, invert=True)
    lengths = table_h[input_ids]
    metrics = np.array([lengths[plain].mean(), (input_ids == tokenizer.unk_token_id).mean()])
    return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (input_ids, labels, lengths, metrics)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-collator", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    b, s, v, n, l, seed = 128, 128, 32768, 16384, 7, 1234
    rng = np.random.default_rng(seed)
    special, mask_id, unk_id = [1, 0, 2, 3, 4], 4, 3
    ids_h = np.minimum(5 + np.floor((v - 5) * rng.random((b, s)) ** 3).astype(np.int64), v - 1)
    ids_h[:, 0], ids_h[:, -1] = 0, 2
    ids_h[rng.random((b, s)) < 0.002] = unk_id
    table_h = rng.integers(1, 17, v).astype(np.int64)
    sf_h = rng.integers(0, 50000, (v, l)).astype(np.int32)
    priors_h = rng.standard_normal(v)
    order_h = rng.permutation(v).astype(np.int64)
    ids, table_t, sf, priors64, order = (torch.from_numpy(x).to(dev) for x in (ids_h, table_h, sf_h, priors_h, order_h))
    priors32 = priors64.float()
    special_t = torch.tensor(special, device=dev)
    thresholds = collate.mlm_thresholds()
    tokenizer = _Tokenizer(v, special, mask_id, unk_id)
    lines, result = [], {"metric": "collate", "b": b, "s": s, "v": v, "n": n, "l": l, "steps": args.steps, "warmup": args.warmup}

    labelled = {}
    for loss in ("mlm", "clm"):
        mlm = loss == "mlm"

        def hip(check=False, loss=loss):
            return collate.label_batch(ids, special, table_t, vocab_len=v, loss=loss, mask_token_id=mask_id, unk_token_id=unk_id, seed=seed, check=check)

        def torch_path(mlm=mlm):
            return torch_label(ids, special_t, table_t, v, mask_id, unk_id, seed, thresholds, mlm)

        def numpy_path(mlm=mlm, generator=None):
            return numpy_label(ids_h, tokenizer, table_h, dev, mlm, generator)

        lb = labelled[loss] = hip(check=True)
        for name, other in (("torch", torch_path()), ("numpy", numpy_path(generator=cr.CounterGenerator(seed) if mlm else None))):
            for key, x in zip(("input_ids", "labels", "byte_lengths", "metrics"), other):
                got = getattr(lb, key)
                assert torch.equal(got, x) and got.dtype == x.dtype, (loss, name, key)
        table(f"label_batch, {loss}: {int(lb.record[4])} masked of {b * s}", {"hip, check=False": hip, "hip, check=True (one host read)": lambda: hip(True),
              "numpy (the library's collator, metrics) + host-to-device copies": numpy_path, "torch on the device": torch_path}, args.steps, args.warmup, lines, result)

    lb = labelled["mlm"]
    members = ("input_ids", "labels", "ids_to_embed", "target_surface_forms", "target_priors", "mask")
    lb_ids_h, lb_labels_h = lb.input_ids.cpu().numpy(), lb.labels.cpu().numpy()

    def hip_sub():
        return training.subsample_batch_vocabulary(lb.input_ids, lb.labels, special, n, sf, priors32, mode="random", negative_order=order, check=False)

    def numpy_sub():
        out = batch_vocab_ref(lb_ids_h, lb_labels_h, special, n, sf_h, priors_h.astype(np.float32), "random", order_h)
        return [torch.from_numpy(np.ascontiguousarray(out[k])).to(dev) for k in members]

    for key, x in zip(members, numpy_sub()):
        assert torch.equal(getattr(hip_sub(), key), x), key
    table(f"the vocabulary, subsampled to N = {n} (mlm labels)", {"hip (subsample_batch_vocabulary, check=False)": hip_sub, "numpy restatement + host-to-device copies": numpy_sub},
          args.steps, args.warmup, lines, result)

    rows = collate.padded_rows(v - 3, 128)          # a vocabulary of 32 765 ids padded to 32 768 rows
    sf_p, priors_p, sf_ph, priors_ph = sf[:v - 3], priors64[:v - 3], sf_h[:v - 3], priors_h[:v - 3]
    pad_members = ("target_surface_forms", "target_priors", "mask", "ids_to_embed")

    def hip_pad():
        return collate.pad_vocabulary(sf_p, priors_p, rows)

    def numpy_pad():
        k = rows - len(priors_ph)
        out = (np.pad(sf_ph, ((0, k), (0, 0)), constant_values=0), np.pad(priors_ph, (0, k), constant_values=-100000).astype(np.float32),
               np.concatenate([np.ones(len(priors_ph), dtype=bool), np.zeros(k, dtype=bool)]), np.concatenate([np.arange(len(priors_ph)), np.zeros(k, dtype=np.int32)]))
        return [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in out]

    def torch_pad():
        k, m = rows - priors_p.numel(), priors_p.numel()
        return (torch.cat([sf_p, sf_p.new_zeros((k, l))]), torch.cat([priors_p.float(), priors_p.new_full((k,), -100000.0, dtype=torch.float32)]),
                torch.cat([torch.ones(m, dtype=torch.bool, device=dev), torch.zeros(k, dtype=torch.bool, device=dev)]),
                torch.cat([torch.arange(m, device=dev), torch.zeros(k, dtype=torch.int64, device=dev)]))

    for name, other in (("numpy", numpy_pad()), ("torch", torch_pad())):
        for key, x in zip(pad_members, other):
            assert torch.equal(getattr(hip_pad(), key), x), (name, key)
    table(f"the vocabulary, {v - 3} ids padded to {rows} rows (float64 priors)", {"hip (pad_vocabulary, one launch)": hip_pad, "numpy.pad + host-to-device copies": numpy_pad,
          "torch.cat on the device": torch_pad}, args.steps, args.warmup, lines, result)

    if not args.skip_collator:
        _bpe = cr.bpe_tokenizer
        words = "the quick brown fox jumps over the lazy dog , it's 12 345 times . we'll see".split(" ")
        texts = [" ".join(words[i] for i in rng.integers(0, len(words), size=150)) for _ in range(b)]
        data = [{"texts": texts, "lang_code": "en"}]
        for loss, n_sub in (("mlm", 512), ("clm", None)):
            a = types.SimpleNamespace(do_tokenizer_sampling=False, n_token_subsample=n_sub, pad_to_multiple_of=8, subsample_mode="random", block_size=s,
                                      use_passthrough_hypernet=False, add_prefix_space=False, hn_surface_maxlen=l, sample_text_span=True, langs=["en"])
            c = collate.DeviceCollator(_bpe(), _bpe(False), a, loss=loss, tokenizer=_bpe(), device=dev)
            vv = len(c.tokenizer)
            table_c, sf_c, scores_c = c.byte_lengths.cpu().numpy(), c.surface_forms.cpu().numpy(), c.scores.cpu().numpy()

            def device_call(check=False, c=c):
                return c(data, seed=seed, check=check)

            def host_call(c=c, loss=loss, n_sub=n_sub, vv=vv, table_c=table_c, sf_c=sf_c, scores_c=scores_c):
                r = np.random.default_rng(seed)
                cut = []
                for text in texts:
                    start = int(r.integers(0, max(len(text) - 16 * s, 0) + 1))
                    cut.append(text[start:start + 16 * s])
                enc = c.tokenizer(cut, max_length=s, truncation=True, padding="max_length", return_tensors="np", add_special_tokens=True)
                out = cr.encode(enc["input_ids"], c.special_ids, table_c, sf_c, scores_c, loss=loss, mask_token_id=c.mask_token_id, unk_token_id=c.unk_token_id,
                                seed=collate.derived_seed(seed, 0), n_token_subsample=n_sub, negative_order=r.permutation(vv) if n_sub else None)
                out["attention_mask"] = enc["attention_mask"]
                return {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in out.items() if isinstance(x, np.ndarray)}

            got, want = device_call(True), host_call()
            for key in ("attention_mask", "byte_lengths") + (() if n_sub else ("input_ids", "labels", "target_surface_forms", "target_priors", "mask", "ids_to_embed")):
                assert torch.equal(got[key], want[key].to(got[key].dtype)), (loss, key)          # (subsampled: the two paths draw negative_order from different generators)
            table(f"a whole collator call, {loss}, {'N = ' + str(n_sub) if n_sub else 'padded'}: {b} texts x block_size {s}, V = {vv}",
                  {"DeviceCollator, check=False": device_call, "DeviceCollator, check=True": lambda: device_call(True),
                   "host: the tokenizer's call, the numpy restatement, host-to-device copies": host_call}, args.steps, args.warmup, lines, result)

    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
