"""Text encoding: the device encoder against the ``tokenizers`` library it replaces (profiles/encode_texts_bench.md).

    python tools/encode_bench.py [--texts 512] [--chars 2048] [--block 128] [--pieces 32768] [--json out.json] [--once]

One process, the variants alternating, the median of 10 after 3 warm-ups, the variants checked equal before anything is timed:
  device    DeviceTextEncoder.__call__(check=False): host clock (call to synchronised stream) and HIP events
  library   tokenizer(texts, max_length=block, truncation=True, padding="max_length") on 16 threads, plus the host-to-device copy
and the one-time costs: the class-table probe, zett_retok_create for a fresh tokenizer, DeviceTextEncoder.from_tokenizer.
Two tokenizers: a Unigram model of --pieces pieces dressed the way the reference's sample_tokenizer dresses one (Prepend(" "), the
split pattern, ByteLevel), and a byte-level BPE trained here with the ByteLevel(use_regex=True) pre-tokenizer.  --once: one call per
tokenizer to check it and ten more of the device encoder, nothing timed (for a kernel trace).
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import sys
import time
from collections import Counter

os.environ.setdefault("TOKENIZERS_PARALLELISM", "true")
os.environ.setdefault("RAYON_NUM_THREADS", "16")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from zett_amd import text_encode as te                                     # noqa: E402
from zett_amd.surface_forms import BYTES_TO_CHARS_LIST, DeviceRetokenizer, HnTokenizerSpec      # noqa: E402

SPECIALS = {"<s>": 0, "<pad>": 1, "</s>": 2, "<unk>": 3}


def corpus(n_texts, max_chars, seed=0):
    """Texts of up to max_chars characters: the repository's own documents and sources, cut at random places, every fourth text with
    runs of Cyrillic, Greek, CJK and accented words mixed in."""
    rng = np.random.default_rng(seed)
    blob = ""
    for path in sorted(glob.glob(os.path.join(REPO, "*.md")) + glob.glob(os.path.join(REPO, "zett_amd", "*.py"))):
        with open(path, encoding="utf-8", errors="ignore") as f:
            blob += f.read() + "\n"
    blob = blob.replace("<s>", "< s>").replace("</s>", "< /s>").replace("<pad>", "< pad>").replace("<unk>", "< unk>")
    blocks = [(0x00C0, 0x017F), (0x0400, 0x045F), (0x0370, 0x03FF), (0x4E00, 0x4E80)]
    texts = []
    for i in range(n_texts):
        n = int(rng.integers(max_chars // 4, max_chars + 1))
        start = int(rng.integers(0, len(blob) - n))
        text = blob[start:start + n]
        if i % 4 == 3:
            lo, hi = blocks[int(rng.integers(0, len(blocks)))]
            words = ["".join(chr(int(c)) for c in rng.integers(lo, hi, size=int(rng.integers(2, 8)))) for _ in range(40)]
            text = (" ".join(words) + " " + text)[:n]
        texts.append(text)
    return texts


def unigram_tokenizer(texts, n_pieces, add_prefix_space=True):
    """zett/collator.py:363-431 with pieces counted here: the most frequent substrings (up to 16 bytes) of the words, log relative
    frequencies as scores, every missing byte at the minimum score, the specials at their ids."""
    import tokenizers
    from tokenizers import Tokenizer, decoders, models, normalizers, pre_tokenizers, processors
    from transformers import PreTrainedTokenizerFast
    split = pre_tokenizers.Split(tokenizers.Regex(te.SPLIT_PATTERN_MARKS), "removed", invert=True)
    words = Counter()
    for text in texts:
        words.update(w for w, _ in split.pre_tokenize_str(" " + text))
    counts = Counter()
    for word, c in words.items():
        w = "".join(BYTES_TO_CHARS_LIST[b] for b in word.encode("utf-8"))
        for i in range(len(w)):
            for j in range(i + 1, min(len(w), i + 16) + 1):
                counts[w[i:j]] += c
    top = sorted(counts.items(), key=lambda kv: (-kv[1], kv[0]))[:n_pieces]
    total = sum(c for _, c in top)
    pieces = [p for p, _ in top]
    scores = [float(np.log(c / total)) for _, c in top]
    have = set(pieces)
    missing = sorted(set(BYTES_TO_CHARS_LIST) - have)
    pieces, scores = missing + pieces, [min(scores)] * len(missing) + scores
    for name, i in sorted(SPECIALS.items(), key=lambda kv: kv[1]):
        pieces.insert(i, name)
        scores.insert(i, 0.0)
    tk = Tokenizer(models.Unigram(list(zip(pieces, scores))))
    if add_prefix_space:
        tk.normalizer = normalizers.Prepend(" ")
    tk.pre_tokenizer = pre_tokenizers.Sequence([split, pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=False)])
    tk.decoder = decoders.ByteLevel()
    tk.post_processor = processors.TemplateProcessing(single="<s> $A </s>", special_tokens=[("<s>", 0), ("</s>", 2)])
    return PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>", clean_up_tokenization_spaces=False)


def bpe_tokenizer(texts, vocab_size=8192):
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    from transformers import PreTrainedTokenizerFast
    tk = Tokenizer(models.BPE())
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    trainer = trainers.BpeTrainer(vocab_size=vocab_size, special_tokens=sorted(SPECIALS, key=SPECIALS.get), initial_alphabet=pre_tokenizers.ByteLevel.alphabet(),
                                  show_progress=False)
    tk.train_from_iterator(texts, trainer)
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(use_regex=True, add_prefix_space=True)
    tk.decoder = decoders.ByteLevel()
    tk.post_processor = processors.TemplateProcessing(single="<s> $A </s>", special_tokens=[("<s>", 0), ("</s>", 2)])
    return PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>", clean_up_tokenization_spaces=False)


def median_ms(samples):
    return float(np.median(samples)) * 1e3


def bench(name, tokenizer, texts, block, dev, once):
    t0 = time.perf_counter()
    spec = HnTokenizerSpec.from_tokenizer(tokenizer)
    t_spec = time.perf_counter() - t0
    t0 = time.perf_counter()
    rt = DeviceRetokenizer(spec, dev)
    torch.cuda.synchronize()
    t_create = time.perf_counter() - t0
    rt.close()
    t0 = time.perf_counter()
    enc = te.DeviceTextEncoder.from_tokenizer(tokenizer, dev)
    torch.cuda.synchronize()
    t_from = time.perf_counter() - t0

    def library():
        out = tokenizer(texts, max_length=block, truncation=True, padding="max_length", return_tensors="np", add_special_tokens=True)
        ids = torch.from_numpy(out["input_ids"]).to(dev, non_blocking=False)
        mask = torch.from_numpy(out["attention_mask"]).to(dev, non_blocking=False)
        torch.cuda.synchronize()
        return ids, mask

    def device():
        out = enc(texts, block, check=False)
        return out["input_ids"], out["attention_mask"]
    got, want = device(), library()
    torch.cuda.synchronize()
    assert int(enc.last_status.item()) == 0
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), f"{name}: the device encoder and the library differ"
    if once:
        for _ in range(10):
            device()
        torch.cuda.synchronize()
        return {"tokenizer": name, "equal": True}
    host, events, lib = [], [], []
    for i in range(13):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        device()
        b.record()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        t0 = time.perf_counter()
        library()
        dl = time.perf_counter() - t0
        if i >= 3:
            host.append(dt); events.append(a.elapsed_time(b) * 1e-3); lib.append(dl)
    n_bytes = len("".join(texts).encode("utf-8"))
    return {"tokenizer": name, "equal": True, "texts": len(texts), "text_bytes": n_bytes, "block_size": block, "vocab": len(tokenizer),
            "real_ids": int(got[1].sum().item()), "device_host_ms": median_ms(host), "device_events_ms": median_ms(events), "library_ms": median_ms(lib),
            "workspace_mb": enc.workspace_bytes(n_bytes, len(texts)) / 2 ** 20,
            "one_time_ms": {"model_arrays_host": t_spec * 1e3, "zett_retok_create": t_create * 1e3, "from_tokenizer": t_from * 1e3}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=512)
    ap.add_argument("--chars", type=int, default=2048)
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--pieces", type=int, default=32768)
    ap.add_argument("--json", default=None)
    ap.add_argument("--once", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    texts = corpus(args.texts, args.chars)
    t0 = time.perf_counter()
    te.class_table()
    t_table = time.perf_counter() - t0
    results = {"class_table_probe_ms": t_table * 1e3, "threads": os.environ["RAYON_NUM_THREADS"], "cases": []}
    for name, make in (("unigram", lambda: unigram_tokenizer(texts, args.pieces)), ("bpe", lambda: bpe_tokenizer(texts))):
        results["cases"].append(bench(name, make(), texts, args.block, dev, args.once))
        print(json.dumps(results["cases"][-1]), flush=True)
    print(json.dumps({"class_table_probe_ms": results["class_table_probe_ms"]}))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
