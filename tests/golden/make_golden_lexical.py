"""Lexical-transfer fixtures: outputs of the reference's scripts/transfer_lexical.py, run as it is.

Runs only in the build container (like make_golden_retok.py, whose corpus, trainers and import stubs it reuses).  Two tiny
local models are built in a temporary directory:

  unigram   Unigram / Metaspace source tokenizer, tied RoBERTa whose embedding matrix has 60 rows FEWER than the tokenizer
  bpe       Mistral-like byte-fallback BPE source tokenizer, untied GPT-NeoX whose matrices have 24 rows MORE

the target is the byte-level BPE of the retok fixtures.  The reference script itself runs (runpy, HF_HUB_OFFLINE=1) once per
fvt_mode, plus one fallback_mode=random run with np.random.seed set.  A fixture holds DATA only: the converted source
tokenizer's model JSON, its whole get_vocab(), unk_token_id, the target token list, the source matrices, the matrices the
script saved and the overlap counts it printed.

    python tests/golden/make_golden_lexical.py [OUTPUT_DIR]

Deterministic: the generator runs itself in a child process with PYTHONHASHSEED=0 (the reference's convert_to_byte_level walks
Python sets: the order of the byte-level merges it adds follows the string hash) and RAYON_NUM_THREADS=1 (the Unigram trainer's
threads); the vocabulary is stored sorted by id.  The Unigram source tokenizer is read from lexical_unigram_tokenizer.json.gz (the
output of one `tokenizers` training run on the local corpus: that trainer is not reproducible from run to run), so the committed
fixtures regenerate bit for bit from the committed inputs.
"""
from __future__ import annotations

import contextlib
import gzip
import io
import json
import os
import re
import runpy
import sys
import tempfile
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = HERE          # where the fixtures go (argv[1] overrides)
sys.path.insert(0, HERE)
import make_golden_retok as mgr  # noqa: E402

SCRIPT = os.path.join(mgr.REFERENCE, "scripts", "transfer_lexical.py")
UNIGRAM_TOKENIZER = os.path.join(HERE, "lexical_unigram_tokenizer.json.gz")      # the Unigram source tokenizer before conversion (see make_uni)
HIDDEN = 32
RANDOM_SEED = 1234


def write_gz(path, text):
    """gzip without a time stamp or file name in the header: the same text gives the same bytes"""
    with open(path, "wb") as raw, gzip.GzipFile(filename="", mode="wb", fileobj=raw, mtime=0) as f:
        f.write(text.encode("utf-8"))


def run_reference(output, tokenizer_dir, model_dir, model_class, fvt_mode, fallback_mode="unk", seed=None):
    """The reference script in this process; returns the (k, n) of its "Overlapping tokens: k/n" line."""
    argv = sys.argv
    sys.argv = [SCRIPT, "--output", output, "--tokenizer_name", tokenizer_dir, "--model_name_or_path", model_dir,
                "--model_class", model_class, "--fvt_mode", fvt_mode, "--fallback_mode", fallback_mode]
    if seed is not None:
        np.random.seed(seed)
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            runpy.run_path(SCRIPT, run_name="__main__")
    finally:
        sys.argv = argv
    m = re.search(r"Overlapping tokens: (\d+)/(\d+)", buf.getvalue())
    return int(m.group(1)), int(m.group(2))


def matrices(output, model_class, tied):
    import transformers
    model = getattr(transformers, model_class).from_pretrained(output)
    w_in = model.get_input_embeddings().weight.data.numpy().copy()
    return (w_in, None) if tied else (w_in, model.get_output_embeddings().weight.data.numpy().copy())


def dump_case(name, tmp, src_tok, model, model_class, tgt_dir, convert_to_byte_level):
    from transformers import AutoTokenizer
    model_dir = os.path.join(tmp, name + "_model")
    src_tok.save_pretrained(model_dir)
    model.save_pretrained(model_dir)
    tied = bool(model.config.tie_word_embeddings)
    # what the script works on (scripts/transfer_lexical.py:27-34)
    source = convert_to_byte_level(AutoTokenizer.from_pretrained(model_dir))[0]
    target = convert_to_byte_level(AutoTokenizer.from_pretrained(tgt_dir), match_special_tokens_to=source, make_whitespace_consistent=True)[0]
    tokens = target.convert_ids_to_tokens(range(len(target)))
    src_in = model.get_input_embeddings().weight.data.numpy().copy()
    src_out = None if tied else model.get_output_embeddings().weight.data.numpy().copy()
    meta = {
        "model": json.loads(source._tokenizer.to_str())["model"],
        "vocab": dict(sorted(source.get_vocab().items(), key=lambda kv: (kv[1], kv[0]))),
        "special_tokens": list(source.all_special_tokens),
        "unk_token_id": source.unk_token_id,
        "tokenizer_length": len(source),
        "n_source_rows": int(src_in.shape[0]),
        "tied": tied,
        "model_class": model_class,
        "tokens": tokens,
        "overlap": {},
        "random_seed": RANDOM_SEED,
    }
    arrays = {"source_in": src_in}
    if src_out is not None:
        arrays["source_out"] = src_out
    np.savez_compressed(os.path.join(OUT, f"lexical_{name}_source.npz"), **arrays)
    runs = [("no", "unk"), ("fvt", "unk"), ("bfvt", "unk")] + ([("fvt", "random")] if tied else [])
    for fvt_mode, fallback_mode in runs:
        out_dir = os.path.join(tmp, f"{name}_{fvt_mode}_{fallback_mode}")
        k, n = run_reference(out_dir, tgt_dir, model_dir, model_class, fvt_mode, fallback_mode, seed=RANDOM_SEED if fallback_mode == "random" else None)
        assert n == len(tokens), (n, len(tokens))
        w_in, w_out = matrices(out_dir, model_class, tied)
        key = fvt_mode if fallback_mode == "unk" else f"{fvt_mode}_{fallback_mode}"
        meta["overlap"][key] = k
        arrays = {"expected_in": w_in}
        if w_out is not None:
            arrays["expected_out"] = w_out
        path = os.path.join(OUT, f"lexical_{name}_{key}.npz")
        np.savez_compressed(path, **arrays)
        print("wrote", os.path.basename(path), f"overlap {k}/{n}, {os.path.getsize(path) / 1024:.0f} KiB")
    path = os.path.join(OUT, f"lexical_{name}.json.gz")
    write_gz(path, json.dumps(meta, ensure_ascii=False, separators=(",", ":")))
    print("wrote", os.path.basename(path), f"{len(tokens)} tokens, R = {src_in.shape[0]}, tokenizer {len(source)}, {os.path.getsize(path) / 1024:.0f} KiB")
    return meta, tokens, source


def row_classes(meta, tokens, source):
    """How many rows fall in each class per mode, and the longest decomposition (printed, not stored)."""
    R, vocab, model = meta["n_source_rows"], meta["vocab"], source._tokenizer.model
    for mode in ("fvt", "bfvt"):
        exact = mean = fallback = long_rows = longest = 0
        for t in tokens:
            idx = vocab.get(t)
            if idx is not None and idx < R:
                exact += 1
                continue
            ids = [x.id for x in model.tokenize(t)]
            if mode == "fvt":
                ids = [] if any(i >= R for i in ids) else ids
            else:
                ids = [i for i in ids if i < R]
            if ids:
                mean += 1
                longest = max(longest, len(ids))
                long_rows += len(ids) > 16
            else:
                fallback += 1
        print(f"  {mode}: {exact} exact, {mean} mean, {fallback} fallback; longest decomposition {longest}, rows with n > 16: {long_rows}")


def main():
    global OUT
    if len(sys.argv) > 1:
        OUT = os.path.abspath(sys.argv[1])
        os.makedirs(OUT, exist_ok=True)
    if os.environ.get("PYTHONHASHSEED") != "0" or os.environ.get("RAYON_NUM_THREADS") != "1":
        import subprocess
        env = dict(os.environ, PYTHONHASHSEED="0", RAYON_NUM_THREADS="1", TOKENIZERS_PARALLELISM="false")
        raise SystemExit(subprocess.run([sys.executable, os.path.abspath(__file__), OUT], env=env).returncode)
    os.environ["HF_HUB_OFFLINE"] = "1"
    os.environ["TRANSFORMERS_OFFLINE"] = "1"
    sys.modules.setdefault("datasets", MagicMock())          # the script imports load_dataset and never calls it
    convert_to_byte_level = mgr._import_reference()[0]
    import torch
    from transformers import GPTNeoXConfig, GPTNeoXForCausalLM, RobertaConfig, RobertaForMaskedLM

    lines_a, lines_b = mgr.corpus(1), mgr.corpus(2)
    with tempfile.TemporaryDirectory() as tmp:
        tgt_dir = os.path.join(tmp, "target")
        mgr.wrap(mgr.train_bytelevel_bpe(lines_b, 2500, ["<|endoftext|>"]), eos_token="<|endoftext|>").save_pretrained(tgt_dir)

        def converted_length(make):          # the row counts are set against the tokenizer the script works on, i.e. after conversion
            return len(convert_to_byte_level(make())[0])

        def make_uni():
            # tokenizers' Unigram trainer is not reproducible (its sums follow the iteration order of hash maps seeded per process:
            # scores differ in the last bits from run to run, sometimes the vocabulary too), so the trained tokenizer is itself a
            # committed input of the generator; it is trained afresh only when that file is missing
            from tokenizers import Tokenizer
            if not os.path.exists(UNIGRAM_TOKENIZER):
                write_gz(UNIGRAM_TOKENIZER, mgr.train_metaspace_unigram(lines_a, 2000).to_str())
                print("trained", os.path.basename(UNIGRAM_TOKENIZER))
            return mgr.wrap(Tokenizer.from_str(gzip.open(UNIGRAM_TOKENIZER, "rt", encoding="utf-8").read()), bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>")

        def make_mis():
            return mgr.wrap(mgr.train_mistral_like(lines_a, 2200), bos_token="<s>", eos_token="</s>", unk_token="<unk>")

        uni = make_uni()
        torch.manual_seed(1)
        roberta = RobertaForMaskedLM(RobertaConfig(vocab_size=converted_length(make_uni) - 60, hidden_size=HIDDEN, num_hidden_layers=1, num_attention_heads=2,
                                                   intermediate_size=64, max_position_embeddings=66, pad_token_id=uni.pad_token_id,
                                                   bos_token_id=uni.bos_token_id, eos_token_id=uni.eos_token_id, tie_word_embeddings=True))
        print("unigram (tied RoBERTa, 60 rows fewer than the tokenizer)")
        row_classes(*dump_case("unigram", tmp, uni, roberta, "AutoModelForMaskedLM", tgt_dir, convert_to_byte_level))

        mis = make_mis()
        torch.manual_seed(2)
        neox = GPTNeoXForCausalLM(GPTNeoXConfig(vocab_size=converted_length(make_mis) + 24, hidden_size=HIDDEN, num_hidden_layers=1, num_attention_heads=2,
                                                intermediate_size=64, max_position_embeddings=64, bos_token_id=mis.bos_token_id,
                                                eos_token_id=mis.eos_token_id, tie_word_embeddings=False))
        print("bpe (untied GPT-NeoX, 24 rows more than the tokenizer)")
        row_classes(*dump_case("bpe", tmp, mis, neox, "AutoModelForCausalLM", tgt_dir, convert_to_byte_level))


if __name__ == "__main__":
    main()
