"""Collator fixtures: the WHOLE dict the reference's ``Collator.encode`` (zett/collator.py:155-339) returns — the inner collator, the metrics,
byte_lengths and both vocabulary branches.

Runs only in the build container, next to a checkout of the reference, the way make_golden_batch_vocab.py does: the stubs of
make_golden_retok._import_reference(), a MagicMock for ``rust_utils``, a stand-in tokenizer that returns prepared input_ids, and
``np.random.shuffle`` recorded.  The Collator is built with ``do_tokenizer_sampling=True`` and ``tokenizer_name=None`` so that no tokenizer is
loaded; ``encode`` reads the flag again, so the fixed-tokenizer case clears it before the call.  Under MLM the ``inner_collator`` is a factory
that returns the installed ``DataCollatorForLanguageModeling`` with the counter-based generator of tests/collate_ref.py injected — the
library accepts a ``generator`` object — so the draws are the ones the product defines and everything else is the library's arithmetic.
Nothing of the reference is copied: a fixture holds the inputs and the arrays it returned.

Under MLM with n_token_subsample the reference lets the label -100 into ``np.unique`` and lists it as an id (it then indexes the priors and
surface forms from the end); the product deliberately does not.  Those two fixtures record what the reference
returned all the same; tests/test_collate_host.py compares them through ``ids_to_embed[input_ids]``, which the extra entry does not change.

A second kind of fixture (``collate_call_*.npz``) records the reference's ``Collator.__call__`` on TEXTS with a fixed tokenizer: the Collator
is built with ``tokenizer_name`` pointing at a saved copy of the repository's test BPE tokenizer, so its own ``__init__`` runs
(``AutoTokenizer.from_pretrained``, ``convert_to_byte_level``, the surface-form matrix, scores, byte lengths) and so does the tokenizer call.
Those fixtures hold the texts, the tables ``__init__`` prepared and the returned dict; the label seed is the one ``DeviceCollator`` derives
from the call's seed.

    python tests/golden/make_golden_collate.py
"""
from __future__ import annotations

import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from make_golden_batch_vocab import _collator_class, save  # noqa: E402

from tests import collate_ref as cr  # noqa: E402

L = 5
# name -> loss, n_token_subsample, subsample_mode, do_tokenizer_sampling, tokenizer_sample_max, V, (B, S), special ids (pad, bos, eos, mask[, unk]), unk?, probabilities, seed
CASES = {
    "collate_mlm_random": ("mlm", 128, "random", True, 512, 300, (4, 16), [0, 1, 2, 299, 3], True, (0.15, 0.8, 0.1), 5),
    "collate_mlm_positives_only": ("mlm", 256, "positives_only", True, 512, 300, (8, 32), [0, 1, 2, 299, 3], True, (0.3, 0.5, 0.5), 6),
    "collate_clm_padded_sampled": ("clm", None, "random", True, 384, 300, (4, 16), [0, 1, 2, 299, 3], True, (0.15, 0.8, 0.1), 7),
    "collate_clm_padded_fixed": ("clm", None, "random", False, 384, 397, (3, 17), [1, 0, 396, 2, 3], True, (0.15, 0.8, 0.1), 8),
    "collate_mlm_padded_no_unk": ("mlm", None, "random", True, 384, 300, (4, 16), [0, 1, 2, 299], False, (0.15, 0.8, 0.1), 9),
}
PAD_TO = 8


class StandInTokenizer:
    """What ``encode`` and ``DataCollatorForLanguageModeling`` ask of a tokenizer."""
    mask_token = "<mask>"
    pad_token = "<pad>"
    padding_side = "right"

    def __init__(self, input_ids, v, special_ids, has_unk):
        self.input_ids, self.v = input_ids, v
        self.all_special_ids = list(special_ids)
        self.all_special_tokens = [f"<s{i}>" for i in special_ids]
        self.pad_token_id, self.mask_token_id = special_ids[0], special_ids[3]
        self.unk_token_id = special_ids[4] if has_unk else None

    def __call__(self, texts, **_kw):
        return {"input_ids": self.input_ids.copy(), "attention_mask": (self.input_ids != self.pad_token_id).astype(np.int64)}

    def __len__(self):
        return self.v

    def get_special_tokens_mask(self, ids, already_has_special_tokens=False):
        assert already_has_special_tokens
        return [1 if i in self.all_special_ids else 0 for i in ids]

    def convert_tokens_to_ids(self, token):
        if token == self.mask_token:
            return self.mask_token_id
        return self.all_special_ids[self.all_special_tokens.index(token)]


def inputs_of(name):
    loss, n, mode, sampling, sample_max, v, (b, s), special, has_unk, probabilities, seed = CASES[name]
    rng = np.random.default_rng(seed)
    pad, bos, eos = special[:3]
    ids = np.minimum(4 + np.floor((v - 4) * rng.random((b, s)) ** 2).astype(np.int64), v - 2)
    ids[:, 0] = bos
    for r in range(b):          # rows end with eos and padding of different lengths; one row is full
        fill = int(rng.integers(0, s // 2)) if r else 0
        ids[r, s - 1 - fill] = eos
        ids[r, s - fill:] = pad
    if has_unk:
        ids[b - 1, 1], ids[0, 2] = special[4], special[4]
    surface_forms = rng.integers(0, 1000, (v, L)).astype(np.int32)
    priors = rng.standard_normal(v)          # float64, as the sampler's scores are
    byte_lengths = rng.integers(1, 17, v).astype(np.int64)
    return dict(loss=loss, n=n, mode=mode, sampling=sampling, sample_max=sample_max, v=v, special=special, has_unk=has_unk, probabilities=probabilities, seed=seed,
                ids=ids, surface_forms=surface_forms, priors=priors, byte_lengths=byte_lengths)


def make(name):
    from transformers import DataCollatorForLanguageModeling
    Collator = _collator_class()
    c = inputs_of(name)
    data_args = types.SimpleNamespace(do_tokenizer_sampling=True, n_token_subsample=c["n"], pad_to_multiple_of=PAD_TO, subsample_mode=c["mode"], block_size=c["ids"].shape[1],
                                      tokenizer_sample_max=c["sample_max"], use_passthrough_hypernet=False)
    tokenizer = StandInTokenizer(c["ids"], c["v"], c["special"], c["has_unk"])

    def inner(tok, return_tensors):
        collator = DataCollatorForLanguageModeling(tok, mlm=True, mlm_probability=c["probabilities"][0], mask_replace_prob=c["probabilities"][1],
                                                   random_replace_prob=c["probabilities"][2], return_tensors=return_tensors)
        collator.generator = cr.CounterGenerator(c["seed"])
        return collator

    collator = Collator(tokenizer, None, data_args, tokenizer_name=None, inner_collator=inner if c["loss"] == "mlm" else None)
    data_args.do_tokenizer_sampling = c["sampling"]
    recorded = []
    shuffle = np.random.shuffle

    def recording_shuffle(a):
        shuffle(a)
        recorded.append(a.copy())

    np.random.seed(c["seed"])
    np.random.shuffle = recording_shuffle
    try:
        enc = collator.encode(tokenizer, ["text"] * len(c["ids"]), c["surface_forms"], c["priors"], metrics_data=(c["byte_lengths"],))
    finally:
        np.random.shuffle = shuffle
    if recorded:
        shuffled, = recorded
        order = np.concatenate([shuffled, np.setdiff1d(np.arange(c["v"]), shuffled)]).astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(c["v"]))
    else:
        order = np.zeros(0, dtype=np.int64)
    none = lambda x: np.int64(-1 if x is None else x)          # noqa: E731
    out = {"in_input_ids": c["ids"], "in_special_ids": np.array(c["special"], dtype=np.int64), "in_byte_lengths": c["byte_lengths"], "in_surface_forms": c["surface_forms"],
           "in_priors": c["priors"], "in_loss": np.array(c["loss"]), "in_n_token_subsample": none(c["n"]), "in_subsample_mode": np.array(c["mode"]),
           "in_tokenizer_sample_max": none(c["sample_max"] if c["sampling"] else None), "in_pad_to_multiple_of": np.int64(PAD_TO),
           "in_mask_token_id": np.int64(tokenizer.mask_token_id), "in_unk_token_id": none(tokenizer.unk_token_id), "in_seed": np.int64(c["seed"]),
           "in_probabilities": np.array(c["probabilities"], dtype=np.float64), "in_negative_order": order}
    for key, value in enc.items():
        if key == "metrics":
            out["out_metrics"] = np.array([value["avg_byte_length"], value["unk_ratio"]], dtype=np.float64)
        else:
            out["out_" + key] = np.asarray(value)
    return out


# ---- Collator.__call__ on texts with a fixed tokenizer: the reference's own __init__ (AutoTokenizer.from_pretrained on a saved copy of the
# repository's test BPE tokenizer, convert_to_byte_level, the surface-form matrix, scores, byte lengths), its tokenizer call and encode -----------
# name -> loss, n_token_subsample, subsample_mode, seed of the call
CALL_CASES = {"collate_call_mlm_random": ("mlm", 256, "random", 5), "collate_call_clm_padded": ("clm", None, "random", 6)}
BLOCK, MAXLEN, LANGS = 24, 7, ["de", "en", "fr"]


def call_texts():
    rng = np.random.default_rng(3)
    words = "the quick brown fox jumps over the lazy dog , it's 12 345 times . we'll see".split(" ")
    return [" ".join(words[i] for i in rng.integers(0, len(words), size=int(rng.integers(0, 30)))) for _ in range(8)]


def make_call(name):
    import tempfile

    from transformers import DataCollatorForLanguageModeling
    os.environ["HF_HUB_OFFLINE"] = "1"
    Collator = _collator_class()
    loss, n, mode, seed = CALL_CASES[name]
    texts = call_texts()
    data_args = types.SimpleNamespace(do_tokenizer_sampling=False, n_token_subsample=n, pad_to_multiple_of=PAD_TO, subsample_mode=mode, block_size=BLOCK,
                                      use_passthrough_hypernet=False, add_prefix_space=False, hn_surface_maxlen=MAXLEN, sample_text_span=False, langs=LANGS)

    def inner(tok, return_tensors):
        collator = DataCollatorForLanguageModeling(tok, mlm=True, return_tensors=return_tensors)
        collator.generator = cr.CounterGenerator(cr.derived_seed(seed, 0))          # the label seed DeviceCollator derives from the call's seed
        return collator

    with tempfile.TemporaryDirectory() as saved:
        cr.bpe_tokenizer().save_pretrained(saved)
        collator = Collator(cr.bpe_tokenizer(), cr.bpe_tokenizer(False), data_args, tokenizer_name=saved, inner_collator=inner if loss == "mlm" else None)
    recorded = []
    shuffle = np.random.shuffle

    def recording_shuffle(a):
        shuffle(a)
        recorded.append(a.copy())

    np.random.seed(seed)
    np.random.shuffle = recording_shuffle
    try:
        enc = collator([{"texts": texts, "lang_code": "en"}])
    finally:
        np.random.shuffle = shuffle
    out = {"in_texts": np.array(texts), "in_loss": np.array(loss), "in_n_token_subsample": np.int64(-1 if n is None else n), "in_subsample_mode": np.array(mode),
           "in_pad_to_multiple_of": np.int64(PAD_TO), "in_seed": np.int64(seed), "in_block_size": np.int64(BLOCK), "in_hn_surface_maxlen": np.int64(MAXLEN),
           "in_langs": np.array(LANGS), "in_lang_code": np.array("en"),
           "init_surface_forms": np.asarray(collator.surface_forms), "init_scores": np.asarray(collator.scores, dtype=np.float64),
           "init_byte_lengths": np.asarray(collator.byte_lengths).astype(np.int64), "init_original_length": np.int64(collator.original_length),
           "init_special_ids": np.array(collator.tokenizer.all_special_ids, dtype=np.int64)}
    for key, value in enc.items():
        if key == "metrics":
            out["out_metrics"] = np.array([value["avg_byte_length"], value["unk_ratio"]], dtype=np.float64)
        elif key != "lang_code":
            out["out_" + key] = np.asarray(value)
    assert enc["lang_code"] == "en"
    return out


def main():
    for name in CALL_CASES:
        out = make_call(name)
        path = os.path.join(HERE, name + ".npz")
        save(path, out)
        print("wrote", os.path.basename(path), os.path.getsize(path), "bytes;", {k: (v.dtype.str, v.shape) for k, v in out.items() if not k.startswith("in_")})
    for name in CASES:
        out = make(name)
        path = os.path.join(HERE, name + ".npz")
        save(path, out)
        print("wrote", os.path.basename(path), os.path.getsize(path), "bytes;", {k[4:]: (v.dtype.str, v.shape) for k, v in out.items() if k.startswith("out_")})


if __name__ == "__main__":
    main()
