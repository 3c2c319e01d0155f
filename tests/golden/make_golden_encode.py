"""Text-encoding fixtures: what the reference's ``Collator.encode`` (zett/collator.py:155-178) returns for a batch of texts.

Runs only in the build container, next to a checkout of the reference.  The tokenizers come from the reference's own
``Collator.sample_tokenizer`` (zett/collator.py:341-452) with a stand-in sampler that returns a prepared ``(piece, score)`` list — the
stub route of make_golden_batch_vocab.py: ``rust_utils`` is a MagicMock — and, for the fixed-tokenizer case, from a small byte-level BPE
trained here that wears the ``ByteLevel(use_regex=True)`` pre-tokenizer of zett/collator.py:65.  Nothing of the reference is copied: a
fixture holds the tokenizer's JSON (settings), the texts, block_size, special_ids_map, and the ``input_ids`` / ``attention_mask`` the
reference's ``encode`` returned.

Every case is also run through tests/encode_ref.py before it is written: a fixture the restatement does not reproduce is not written.

    python tests/golden/make_golden_encode.py
"""
from __future__ import annotations

import gzip
import json
import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

SPECIALS = {"<s>": 0, "<pad>": 1, "</s>": 2, "<unk>": 3}
# name -> (model, add_prefix_space, post-processor template or None, block_size, special_ids_map as [from, to] pairs)
CASES = {
    "encode_unigram_prefix_bos_eos_t32": ("unigram", True, "<s> $A </s>", 32, []),
    "encode_unigram_noprefix_bos_t8": ("unigram", False, "<s> $A", 8, []),
    "encode_unigram_prefix_nopost_t8_map": ("unigram", True, None, 8, "auto"),
    "encode_unigram_noprefix_bos_eos_t32_map": ("unigram", False, "<s> $A </s>", 32, "auto"),
    "encode_bpe_prefix_bos_eos_t32": ("bpe", True, "<s> $A </s>", 32, []),
    "encode_bpe_noprefix_nopost_t8": ("bpe", False, None, 8, []),
}
FILLER = ("the quick brown fox jumps over the lazy dog and then it's gone again , isn't it ? we'll see what they've done ; I'm sure you'd say "
          "that numbers like 12 345 and 2024 matter . tokenizers split text into words , words into pieces , pieces into ids .").split(" ")
FIXED_TEXTS = {
    "empty": "",
    "whitespace": " \t\n  ",
    "short": "it's fine",
    "contractions": "x's \"'s a  's\n's x'd'd'll",
    "mixed": "e\u0301 \u0301x na\u00efve \uff11\uff12\uff13\u00a0\U0001F600\u4e2d\u6587\u5b57 ok",
    "trailing": "words then spaces   \n \n",
}


def _collator_class():
    from make_golden_retok import _import_reference
    _import_reference()
    sys.modules.setdefault("rust_utils", MagicMock())
    from zett.collator import Collator
    return Collator


def _reference_tokenizer(template):
    """The tokenizer whose specials, ids and post-processor the sampled tokenizers inherit (zett/collator.py:378-431)."""
    from tokenizers import Tokenizer, models, processors
    from transformers import PreTrainedTokenizerFast
    tk = Tokenizer(models.WordLevel(dict(SPECIALS), unk_token="<unk>"))
    if template is not None:
        names = [x for x in template.split(" ") if x != "$A"]
        tk.post_processor = processors.TemplateProcessing(single=template, special_tokens=[(n, SPECIALS[n]) for n in names])
    return PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>", clean_up_tokenization_spaces=False)


def _corpus():
    rng = np.random.default_rng(7)
    lines = [" ".join(FILLER[i] for i in rng.integers(0, len(FILLER), size=12)) for _ in range(200)]
    return lines + list(FIXED_TEXTS.values())


def _byte_level(word: str) -> str:
    from zett_amd.surface_forms import BYTES_TO_CHARS_LIST
    return "".join(BYTES_TO_CHARS_LIST[b] for b in word.encode("utf-8"))


class StandInSampler:
    """What ``sample_tokenizer`` asks of ``rust_utils.TokenizerSampler``: a ``(piece, score)`` list.  The pieces are the most frequent
    substrings of the corpus' byte-level words, the scores their log relative frequencies."""

    def __init__(self, n_pieces=320):
        from collections import Counter
        from tests import encode_ref
        counts = Counter()
        for line in _corpus():
            for word in encode_ref.split_words(" " + line, True):
                w = _byte_level(word)
                for i in range(len(w)):
                    for j in range(i + 1, min(len(w), i + 6) + 1):
                        counts[w[i:j]] += 1
        top = sorted(counts.items(), key=lambda kv: (-kv[1], kv[0]))[:n_pieces]
        total = sum(c for _, c in top)
        self.pieces = [(p, float(np.log(c / total))) for p, c in top]

    def sample_tokenizer(self, *_args):
        return list(self.pieces)


def _unigram_tokenizer(Collator, add_prefix_space, template):
    reference = _reference_tokenizer(template)
    data_args = types.SimpleNamespace(do_tokenizer_sampling=True, n_token_subsample=None, pad_to_multiple_of=8, block_size=0, tokenizer_sample_mean=320,
                                      tokenizer_sample_std=0, tokenizer_sample_min=320, tokenizer_sample_max=1024, tokenizer_noise_mean=0, tokenizer_noise_std=0,
                                      add_prefix_space=add_prefix_space, use_passthrough_hypernet=False)
    collator = Collator(reference, None, data_args, tokenizer_name=None)
    np.random.seed(0)
    tokenizer, special_ids_map, _sf, priors, _bl = collator.sample_tokenizer(["unused"], StandInSampler())
    assert special_ids_map == {}, special_ids_map
    return collator, tokenizer, priors


def _bpe_tokenizer(Collator, add_prefix_space, template):
    """A byte-level BPE trained on the corpus, dressed as zett/collator.py:64-68 dresses a fixed tokenizer."""
    from tokenizers import Tokenizer, decoders, models, pre_tokenizers, processors, trainers
    from transformers import PreTrainedTokenizerFast
    tk = Tokenizer(models.BPE())
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    trainer = trainers.BpeTrainer(vocab_size=420, special_tokens=sorted(SPECIALS, key=SPECIALS.get), initial_alphabet=pre_tokenizers.ByteLevel.alphabet(), show_progress=False)
    tk.train_from_iterator(_corpus(), trainer)
    assert all(tk.token_to_id(s) == i for s, i in SPECIALS.items())
    tk.pre_tokenizer = pre_tokenizers.ByteLevel(use_regex=True, add_prefix_space=add_prefix_space)
    tk.decoder = decoders.ByteLevel()
    if template is not None:
        names = [x for x in template.split(" ") if x != "$A"]
        tk.post_processor = processors.TemplateProcessing(single=template, special_tokens=[(n, SPECIALS[n]) for n in names])
    tokenizer = PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>", clean_up_tokenization_spaces=False)
    data_args = types.SimpleNamespace(do_tokenizer_sampling=True, n_token_subsample=None, pad_to_multiple_of=8, block_size=0, tokenizer_sample_max=1024,
                                      use_passthrough_hypernet=False)
    collator = Collator(tokenizer, None, data_args, tokenizer_name=None)
    return collator, tokenizer, np.zeros(len(tokenizer))


def _restatement(tokenizer):
    """(EncodeSpec, segment): the arguments of tests/encode_ref.encode for this tokenizer; segmentation by oracle/retok_ref.py."""
    from oracle import retok_ref
    from zett_amd.text_encode import EncodeSpec
    spec = EncodeSpec.from_tokenizer(tokenizer)
    model = retok_ref.model_from_tokenizer_json(json.loads(tokenizer._tokenizer.to_str()))
    return spec, (lambda raw: retok_ref.tokenize(model, raw))


def _texts(spec, segment, block_size):
    """The 8 texts of a case; two of them are fitted to the tokenizer: exactly the ids the row has room for, and a cut inside a word."""
    from tests import encode_ref
    cap = block_size - len(spec.prefix_ids) - len(spec.suffix_ids)

    def count(text):
        return len(encode_ref.text_ids(text, spec.prefix_mode, spec.marks_are_letters, segment, spec.resplit))
    exact = None
    for base in (" ".join(FILLER), "say 12 345 , it's done . " * 8, "a b c d e f g h i j k l m n o p q r s t u v w x y z " * 4):
        for k in range(1, len(base)):
            if count(base[:k]) == cap and not base[:k].endswith(" "):
                exact = base[:k]
                break
        if exact:
            break
    assert exact is not None, "no text with exactly the row's room"
    cut = "ab " + "qxzjkvwq" * 24
    total = 0
    ends = set()
    for word in encode_ref.split_words(encode_ref.apply_prefix(cut, spec.prefix_mode), spec.marks_are_letters, spec.resplit):
        total += len(segment(word.encode("utf-8")))
        ends.add(total)
    assert total > cap and cap not in ends, "the cut does not fall inside a word"
    t = FIXED_TEXTS
    return [t["empty"], t["whitespace"], t["short"], exact, cut, t["contractions"], t["mixed"], t["trailing"]]


def make(name):
    from tests import encode_ref
    kind, add_prefix_space, template, block_size, id_map = CASES[name]
    Collator = _collator_class()
    collator, tokenizer, priors = (_unigram_tokenizer if kind == "unigram" else _bpe_tokenizer)(Collator, add_prefix_space, template)
    collator.data_args.block_size = block_size
    spec, segment = _restatement(tokenizer)
    texts = _texts(spec, segment, block_size)
    plain = collator.encode(tokenizer, texts, np.zeros((len(priors), 1), dtype=np.int64), np.asarray(priors, dtype=np.float32), {})
    if id_map == "auto":          # ids that occur: the most frequent id becomes the pad id, and a chain a -> b, b -> c pins the order
        values, counts = np.unique(plain["input_ids"][plain["attention_mask"] == 1], return_counts=True)
        a, b, c = (int(x) for x in values[np.argsort(-counts, kind="stable")][:3])
        id_map = [[a, b], [b, c], [spec.pad_id, a]]
    special_ids_map = {int(k): int(v) for k, v in id_map}
    enc = collator.encode(tokenizer, texts, np.zeros((len(priors), 1), dtype=np.int64), np.asarray(priors, dtype=np.float32), special_ids_map)
    ids, mask = np.asarray(enc["input_ids"]).astype(np.int64), np.asarray(enc["attention_mask"]).astype(np.int64)
    want_ids, want_mask = encode_ref.encode(texts, block_size, prefix_mode=spec.prefix_mode, marks_are_letters=spec.marks_are_letters, prefix_ids=spec.prefix_ids,
                                            suffix_ids=spec.suffix_ids, pad_id=spec.pad_id, segment=segment, special_ids_map=special_ids_map, resplit=spec.resplit)
    assert np.array_equal(ids, want_ids) and np.array_equal(mask, want_mask), f"{name}: the restatement differs from the reference"
    return {
        "tokenizer": json.loads(tokenizer._tokenizer.to_str()), "pad_token_id": int(tokenizer.pad_token_id), "padding_side": tokenizer.padding_side,
        "truncation_side": tokenizer.truncation_side, "special_tokens": list(tokenizer.all_special_tokens), "special_ids": [int(i) for i in tokenizer.all_special_ids],
        "texts": texts, "block_size": block_size, "special_ids_map": [[int(k), int(v)] for k, v in id_map],
        "input_ids": ids.tolist(), "attention_mask": mask.tolist(),
    }


def save(path, obj):
    """A .json.gz without a time stamp: the fixtures must regenerate bit for bit."""
    with open(path, "wb") as f:
        with gzip.GzipFile(filename="", mode="wb", fileobj=f, mtime=0) as z:
            z.write(json.dumps(obj, ensure_ascii=True, sort_keys=True, separators=(",", ":")).encode("ascii"))


def main():
    for name in CASES:
        out = make(name)
        path = os.path.join(HERE, name + ".json.gz")
        save(path, out)
        real = [int(sum(r)) for r in out["attention_mask"]]
        print("wrote", os.path.basename(path), os.path.getsize(path), "bytes; ids per row", real)


if __name__ == "__main__":
    main()
