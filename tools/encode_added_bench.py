"""Text encoding with added tokens split out of the texts (profiles/encode_added_bench.md): what the cut step costs.

    python tools/encode_added_bench.py [--texts 512] [--chars 2048] [--block 128] [--pieces 32768] [--every 300] [--json out.json]

The workload and the two tokenizers of tools/encode_bench.py.  One process, the arms alternating, 10 repetitions after 3 warm-ups, each
arm's minimum, median and maximum between HIP events (the library on the host clock):
  plain          zett_encode_texts (the default mode) on the texts as they are — no token string in them
  split0         zett_encode_texts_added with an empty table on the same texts: the same launches
  split2/256     the mode on PACKED texts — the eos string about every --every characters — with 2 and with 256 tokens in the table (the
                 256: </s> and 255 tokens behind ``<|``), checked equal to the library before anything is timed
  library2/256   the installed library on the packed texts on 16 threads, plus its two host-to-device copies
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

import encode_bench as eb      # noqa: E402  (sets the library's thread count before it is imported)
import numpy as np             # noqa: E402
import torch                   # noqa: E402

from zett_amd import text_encode as te      # noqa: E402


def packed(texts, every, eos="</s>", seed=1):
    rng = np.random.default_rng(seed)
    out = []
    for text in texts:
        parts, i = [], 0
        while i < len(text):
            n = int(rng.integers(every // 2, every + every // 2 + 1))
            parts.append(text[i:i + n])
            i += n
        out.append(eos.join(parts))
    return out


def with_tokens(tokenizer, n):
    """the tokenizer's JSON with n added tokens: </s> at its id and n - 1 more behind the vocabulary (<s> for n = 2, else <|k|>)"""
    data = json.loads(tokenizer._tokenizer.to_str())
    v = len(tokenizer)
    names = [("</s>", 2)] + ([("<s>", 0)] if n == 2 else [("<|%d|>" % k, v + k) for k in range(n - 1)])
    data["added_tokens"] = [{"id": i, "content": c, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": True} for c, i in names]
    return data


def stats(samples):
    s = np.asarray(samples) * 1e3
    return {"min": float(s.min()), "median": float(np.median(s)), "max": float(s.max())}


def bench(name, tokenizer, texts, texts_packed, block, dev):
    from tokenizers import Tokenizer
    specials, ids = list(tokenizer.all_special_tokens), [int(i) for i in tokenizer.all_special_ids]
    base = json.loads(tokenizer._tokenizer.to_str())
    make = lambda data, split: te.DeviceTextEncoder.from_tokenizer_json(data, tokenizer.pad_token_id, specials, ids, device=dev, split_added_tokens=split)      # noqa: E731
    plain = make(base, False)
    arms = {"plain": (plain, texts), "split0": (make(dict(base, added_tokens=[]), True), texts)}
    libs = {}
    for n in (2, 256):
        data = with_tokens(tokenizer, n)
        arms["split%d" % n] = (make(data, True), texts_packed)
        tk = Tokenizer.from_str(json.dumps(data))
        tk.enable_truncation(max_length=block)
        tk.enable_padding(length=block, pad_id=tokenizer.pad_token_id, pad_token=tokenizer.pad_token)
        libs["library%d" % n] = tk

    def library(tk):
        out = tk.encode_batch(texts_packed, add_special_tokens=True)
        got = torch.from_numpy(np.array([e.ids for e in out], dtype=np.int64)).to(dev), torch.from_numpy(np.array([e.attention_mask for e in out], dtype=np.int64)).to(dev)
        torch.cuda.synchronize()
        return got

    def device(arm):
        enc, tx = arms[arm]
        out = enc(tx, block, check=False)
        return out["input_ids"], out["attention_mask"]
    a, b = device("plain"), device("split0")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), f"{name}: an empty table changes the rows"
    n_eos = {}
    for n in (2, 256):
        got, want = device("split%d" % n), library(libs["library%d" % n])
        assert int(arms["split%d" % n][0].last_status.item()) == 0
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{name}: the device encoder and the library differ with {n} tokens"
        n_eos[n] = int((got[0][:, 1:-1] == 2).sum().item())
    times = {k: [] for k in list(arms) + list(libs)}
    for i in range(13):
        for arm in arms:
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            device(arm)
            e.record()
            torch.cuda.synchronize()
            if i >= 3:
                times[arm].append(s.elapsed_time(e) * 1e-3)
        for arm, tk in libs.items():
            t0 = time.perf_counter()
            library(tk)
            if i >= 3:
                times[arm].append(time.perf_counter() - t0)
    return {"tokenizer": name, "equal": True, "texts": len(texts), "text_bytes": len("".join(texts).encode("utf-8")), "packed_bytes": len("".join(texts_packed).encode("utf-8")),
            "eos_in_packed_texts": sum(t.count("</s>") for t in texts_packed), "eos_ids_in_rows": n_eos, "block_size": block, "ms": {k: stats(v) for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=512)
    ap.add_argument("--chars", type=int, default=2048)
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--pieces", type=int, default=32768)
    ap.add_argument("--every", type=int, default=300)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    texts = eb.corpus(args.texts, args.chars)
    texts = [t.replace("<|", "< |") for t in texts]
    texts_packed = packed(texts, args.every)
    te.class_table()
    results = []
    for name, make in (("unigram", lambda: eb.unigram_tokenizer(texts, args.pieces)), ("bpe", lambda: eb.bpe_tokenizer(texts))):
        results.append(bench(name, make(), texts, texts_packed, args.block, dev))
        print(json.dumps(results[-1]), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
