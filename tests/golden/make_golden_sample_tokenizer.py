"""Tokenizer-sampling fixtures: what the reference's ``Collator.sample_tokenizer`` (zett/collator.py:341-452) makes of a prepared
``(piece, score)`` list.

Runs only in the build container, next to a checkout of the reference.  ``rust_utils`` is a MagicMock (the stub route of
make_golden_encode.py): the sampler is a stand-in that returns the prepared list, so the fixture pins the HOST half — unknown characters,
the reference's special-token strings among the pieces, specials inserted at their ids, ``special_ids_map``, the tokenizer, ``byte_lengths``
and the surface forms.  The reference tokenizer's ``<unk>`` sits at id 700, beyond the end of the list, so ``special_ids_map`` is not
empty; the list holds the string ``<s>``.  Nothing of the reference is copied: a fixture holds settings, names and recorded results.

    python tests/golden/make_golden_sample_tokenizer.py
"""
from __future__ import annotations

import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

SPECIALS = {"<s>": 0, "<pad>": 1, "</s>": 2, "<unk>": 700}
CASES = {"sample_tokenizer_prefix": True, "sample_tokenizer_noprefix": False}
SURFACE_MAXLEN = 7


def reference_tokenizer():
    from tokenizers import Tokenizer, models, processors
    from transformers import PreTrainedTokenizerFast
    tk = Tokenizer(models.WordLevel(dict(SPECIALS), unk_token="<unk>"))
    tk.post_processor = processors.TemplateProcessing(single="<s> $A </s>", special_tokens=[("<s>", 0), ("</s>", 2)])
    return PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>", clean_up_tokenization_spaces=False)


class PreparedSampler:
    def __init__(self, pieces):
        self.pieces = pieces
        self.calls = []

    def sample_tokenizer(self, *args):
        self.calls.append(args)
        return list(self.pieces)


def prepared_list():
    import make_golden_encode
    pieces = make_golden_encode.StandInSampler(320).pieces
    return pieces[:100] + [("<s>", -3.0)] + pieces[100:]


def make(add_prefix_space: bool):
    import make_golden_encode
    Collator = make_golden_encode._collator_class()
    _, hn_tokenizer, _ = make_golden_encode._bpe_tokenizer(Collator, False, None)
    reference = reference_tokenizer()
    data_args = types.SimpleNamespace(do_tokenizer_sampling=True, n_token_subsample=None, pad_to_multiple_of=8, block_size=0, tokenizer_sample_mean=321,
                                      tokenizer_sample_std=0, tokenizer_sample_min=321, tokenizer_sample_max=1024, tokenizer_noise_mean=0, tokenizer_noise_std=0,
                                      add_prefix_space=add_prefix_space, use_passthrough_hypernet=False, hn_surface_maxlen=SURFACE_MAXLEN)
    collator = Collator(reference, hn_tokenizer, data_args, tokenizer_name=None)
    pieces = prepared_list()
    sampler = PreparedSampler(pieces)
    np.random.seed(0)
    texts = ["one text", "another text"]
    tokenizer, special_ids_map, surface_forms, priors, byte_lengths = collator.sample_tokenizer(texts, sampler)
    assert special_ids_map, "the case must move a special token"
    (counts, n_total, max_length, stride, noise_std, pop_prev, push_current), = sampler.calls
    return {
        "add_prefix_space": add_prefix_space, "texts": texts, "prepared": [[p, float(s)] for p, s in pieces],
        "sampler_call": {"counts": counts, "n_total": int(n_total), "max_length": int(max_length), "stride": int(stride), "noise_std": float(noise_std),
                         "pop_prev": bool(pop_prev), "push_current": bool(push_current)},
        "reference": {"tokenizer": json.loads(reference._tokenizer.to_str()), "bos_token": "<s>", "eos_token": "</s>", "unk_token": "<unk>", "pad_token": "<pad>"},
        "hn_tokenizer": {"tokenizer": json.loads(hn_tokenizer._tokenizer.to_str()), "bos_token": "<s>", "eos_token": "</s>", "unk_token": "<unk>", "pad_token": "<pad>"},
        "hn_surface_maxlen": SURFACE_MAXLEN,
        "pieces": tokenizer.convert_ids_to_tokens(range(len(tokenizer))), "scores": [float(x) for x in priors],
        "special_ids_map": [[int(k), int(v)] for k, v in special_ids_map.items()], "byte_lengths": [int(x) for x in byte_lengths],
        "tokenizer": json.loads(tokenizer._tokenizer.to_str()), "special_tokens": list(tokenizer.all_special_tokens),
        "special_ids": [int(i) for i in tokenizer.all_special_ids], "pad_token_id": int(tokenizer.pad_token_id),
        "surface_forms": np.asarray(surface_forms).astype(np.int64).tolist(),
    }


def main():
    import make_golden_encode
    for name, add_prefix_space in CASES.items():
        out = make(add_prefix_space)
        path = os.path.join(HERE, name + ".json.gz")
        make_golden_encode.save(path, out)
        print("wrote", os.path.basename(path), os.path.getsize(path), "bytes;", len(out["pieces"]), "pieces; special_ids_map", out["special_ids_map"])


if __name__ == "__main__":
    main()
