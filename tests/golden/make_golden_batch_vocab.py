"""Batch-vocabulary fixtures: what the reference's ``Collator.encode`` (zett/collator.py:155-339, the n_token_subsample branch) returns.

Runs only in the build container, next to a checkout of the reference.  zett/collator.py imports the trainer's stack at module
level; the stubs of make_golden_retok._import_reference() plus a MagicMock for ``rust_utils`` are enough for ``encode``.  The Collator
is built with ``do_tokenizer_sampling=True`` and ``tokenizer_name=None`` (no tokenizer is loaded) and is handed a stand-in tokenizer
object that returns prepared input_ids.  Nothing of the reference is copied: a fixture holds the inputs and the arrays it returned.

``np.random.shuffle`` is wrapped to record the shuffled negatives; ``negative_order`` = that order followed by the remaining ids
ascending, so that "the first K entries of negative_order that are not in the batch" is the reference's shuffle-then-truncate — as long
as the reference's own list has no duplicate (it excludes only ``unique(input_ids)`` from its pool), which is asserted for every
"random" case and decided by the case's seed.

The MLM-style case gives the reference labels WITHOUT -100: the reference lets -100 into ``np.unique`` and lists it as an id, which
the product deliberately does not, so no fixture with -100 labels can be equal element for element.  The tests
derive the "labels mostly -100" variant from this fixture by blanking labels whose id still occurs elsewhere, which leaves every other
array of the reference unchanged.

    python tests/golden/make_golden_batch_vocab.py
"""
from __future__ import annotations

import os
import sys
import types
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

V, B, S, N, L = 300, 4, 8, 64, 5
# name -> (special ids in the tokenizer's order, subsample_mode, labels, seed)
CASES = {
    "batch_vocab_clm_random": ([1, 0, 299, 2], "random", "clm", 0),
    "batch_vocab_clm_positives_only": ([1, 0, 299, 2], "positives_only", "clm", 0),
    "batch_vocab_mlm_random": ([1, 0, 299, 2], "random", "mlm", 0),
    "batch_vocab_absent_special_random": ([0, 1, 2], "random", "clm", 0),
}


class StandInTokenizer:
    """What ``encode`` asks of a tokenizer: the call that returns input_ids, the special lists, a length."""

    def __init__(self, input_ids, special_ids):
        self.input_ids = input_ids
        self.all_special_ids = list(special_ids)
        self.all_special_tokens = [f"<s{i}>" for i in special_ids]

    def __call__(self, texts, **_kw):
        return {"input_ids": self.input_ids.copy()}

    def __len__(self):
        return V

    def convert_tokens_to_ids(self, token):
        return self.all_special_ids[self.all_special_tokens.index(token)]


def _collator_class():
    from make_golden_retok import _import_reference
    _import_reference()
    sys.modules.setdefault("rust_utils", MagicMock())
    from zett.collator import Collator
    return Collator


def inputs_of(name):
    special, mode, kind, seed = CASES[name]
    rng = np.random.default_rng(seed)
    ids = np.minimum(np.floor(V * rng.random((B, S)) ** 2).astype(np.int64), V - 1)
    if name.startswith("batch_vocab_absent"):
        ids[ids == 2] = 7                      # special id 2 never occurs
        ids[0, 0], ids[1, 0] = 0, 1
    else:
        ids[0, 0], ids[1, 0], ids[2, -1] = 1, 299, 2
    labels = ids.copy()
    if kind == "mlm":                          # a mask token (special id 2) hides some positions; two ids survive in the labels alone
        labels[0, 3], labels[3, 5] = 123, 250
        hidden = rng.random((B, S)) < 0.3
        hidden[0, 3] = hidden[3, 5] = True
        ids = np.where(hidden, 2, ids)
        assert not np.isin([123, 250], ids).any()
    surface_forms = rng.integers(0, 1000, (V, L)).astype(np.int64)
    priors = rng.standard_normal(V).astype(np.float32)
    return special, mode, kind, seed, ids, labels, surface_forms, priors


def make(name):
    Collator = _collator_class()
    special, mode, kind, seed, ids, labels, surface_forms, priors = inputs_of(name)
    data_args = types.SimpleNamespace(do_tokenizer_sampling=True, n_token_subsample=N, pad_to_multiple_of=8, subsample_mode=mode, block_size=S,
                                      tokenizer_sample_max=V, use_passthrough_hypernet=False)
    tokenizer = StandInTokenizer(ids, special)
    inner = None if kind == "clm" else (lambda tok, return_tensors: (lambda input_ids: {"labels": labels.copy()}))
    collator = Collator(tokenizer, None, data_args, tokenizer_name=None, inner_collator=inner)
    recorded = []
    shuffle = np.random.shuffle

    def recording_shuffle(a):
        shuffle(a)
        recorded.append(a.copy())

    np.random.seed(seed)
    np.random.shuffle = recording_shuffle
    try:
        enc = collator.encode(tokenizer, ["text"] * B, surface_forms, priors)
    finally:
        np.random.shuffle = shuffle
    ids_to_embed = np.asarray(enc["ids_to_embed"])
    assert (ids_to_embed != -100).all() and (ids_to_embed >= 0).all(), name
    if mode == "random":
        assert len(np.unique(ids_to_embed)) == N, f"{name}: the reference's list repeats an id with seed {seed}; choose another"
        shuffled, = recorded
        order = np.concatenate([shuffled, np.setdiff1d(np.arange(V), shuffled)]).astype(np.int64)
        assert np.array_equal(np.sort(order), np.arange(V))
    else:
        assert not recorded
        order = np.zeros(0, dtype=np.int64)
    out = {
        "in_input_ids": ids, "in_labels": labels, "in_special_ids": np.array(special, dtype=np.int64), "in_n": np.int64(N), "in_mode": np.array(mode),
        "in_surface_forms": surface_forms, "in_priors": priors, "in_negative_order": order,
        "out_input_ids": np.asarray(enc["input_ids"]).astype(np.int64), "out_labels": np.asarray(enc["labels"]).astype(np.int64),
        "out_ids_to_embed": ids_to_embed.astype(np.int64), "out_target_surface_forms": np.asarray(enc["target_surface_forms"]).astype(np.int64),
        "out_target_priors": np.asarray(enc["target_priors"]).astype(np.float32), "out_mask": np.asarray(enc["mask"]),
        "out_special_indices": np.asarray(enc["special_indices"]).astype(np.int64),
    }
    return out


def save(path, arrays):
    """An .npz that np.load reads, with a fixed member date: np.savez stamps the time of writing, and the fixtures must regenerate bit for bit."""
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for key in sorted(arrays):
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[key]), allow_pickle=False)


def main():
    for name in CASES:
        out = make(name)
        path = os.path.join(HERE, name + ".npz")
        save(path, out)
        print("wrote", os.path.basename(path), os.path.getsize(path), "bytes; special rows", out["out_special_indices"].tolist())


if __name__ == "__main__":
    main()
