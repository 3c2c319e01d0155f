"""A numpy restatement of zett_amd/collate.py: the labelling pass (include/zett_hip.h, "labelling a batch"), the padded vocabulary, and
the generator that makes the installed ``DataCollatorForLanguageModeling`` draw the same numbers.  Written from the definition, not
from the kernel: the tests compare the two."""
from __future__ import annotations

import math
import os

import numpy as np

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix64(x):
    """the finalizer of splitmix64 on uint64 arrays (wrapping arithmetic)"""
    x = np.asarray(x, dtype=np.uint64)
    with np.errstate(over="ignore"):
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def mix64_int(x: int) -> int:
    """the same on Python integers"""
    x &= M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def keys(seed: int):
    return [mix64_int((int(seed) & M64) + (i + 1) * GOLDEN) for i in range(4)]


def words(seed: int, stream: int, n_positions: int) -> np.ndarray:
    """h_stream(p) for p = 0 .. n_positions - 1"""
    return mix64(np.uint64(keys(seed)[stream]) ^ np.arange(n_positions, dtype=np.uint64))


def thresholds(mlm_probability=0.15, mask_replace_prob=0.8, random_replace_prob=0.1):
    scale = float(1 << 53)
    if mask_replace_prob == 1 or random_replace_prob == 0:
        t_random = 0
    else:
        t_random = min(int(math.ceil(random_replace_prob / (1 - mask_replace_prob) * scale)), 1 << 53)
    return int(math.ceil(mlm_probability * scale)), int(math.ceil(mask_replace_prob * scale)), t_random


def label_batch(input_ids, special_ids, byte_lengths_per_token, *, vocab_len, loss="clm", mask_token_id=None, unk_token_id=None, seed=0, thresholds_=None):
    """-> dict(input_ids, labels, byte_lengths, metrics, record); an id outside the table is never masked, has byte length 0, sets status"""
    ids = np.array(input_ids)
    b, s = ids.shape
    t = b * s
    table = np.asarray(byte_lengths_per_token).astype(np.int64)
    v = len(table)
    flat = ids.reshape(-1).astype(np.int64)
    ok = (flat >= 0) & (flat < v)
    special = np.isin(flat, np.array(list(special_ids), dtype=np.int64))
    out = flat.copy()
    n_masked = n_replaced = n_random = 0
    if loss == "mlm":
        t_mask, t_replace, t_random = thresholds() if thresholds_ is None else thresholds_
        k = [words(seed, i, t) >> np.uint64(11) for i in range(3)]
        masked = ok & ~special & (k[0] < np.uint64(t_mask))
        replaced = masked & (k[1] < np.uint64(t_replace))
        random = masked & ~replaced & (k[2] < np.uint64(t_random))
        labels = np.where(masked, flat, -100)
        out[replaced] = mask_token_id
        out[random] = (words(seed, 3, t) % np.uint64(vocab_len)).astype(np.int64)[random]
        n_masked, n_replaced, n_random = int(masked.sum()), int(replaced.sum()), int(random.sum())
    else:
        labels = flat.copy()
    byte_lengths = np.where(ok, table[np.where(ok, out, 0)], 0)
    plain = ~np.isin(out, np.array(list(special_ids), dtype=np.int64))
    n_plain, byte_sum = int(plain.sum()), int(byte_lengths[plain].sum())
    n_unk = 0 if unk_token_id is None else int((out == unk_token_id).sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        metrics = np.array([np.float64(byte_sum) / np.float64(n_plain), np.float64(n_unk) / np.float64(t)])
    record = np.array([t, n_plain, byte_sum, n_unk, n_masked, n_replaced, n_random, int(not ok.all())], dtype=np.int64)
    return {"input_ids": out.reshape(b, s).astype(ids.dtype), "labels": labels.reshape(b, s).astype(ids.dtype), "byte_lengths": byte_lengths.reshape(b, s),
            "metrics": metrics, "record": record}


def pad_vocabulary(surface_forms, priors, n_rows):
    sf, priors = np.asarray(surface_forms), np.asarray(priors)
    v, l = sf.shape
    out_sf = np.zeros((n_rows, l), dtype=sf.dtype)
    out_sf[:v] = sf
    out_priors = np.full(n_rows, -100000.0, dtype=np.float32)
    out_priors[:v] = priors.astype(np.float32)
    return {"target_surface_forms": out_sf, "target_priors": out_priors, "mask": np.arange(n_rows) < v,
            "ids_to_embed": np.where(np.arange(n_rows) < v, np.arange(n_rows), 0).astype(np.int64)}


class CounterGenerator:
    """What ``DataCollatorForLanguageModeling.generator`` may hold: the i-th ``binomial`` call returns ``k_i(p) * 2^-53 < prob`` at every
    position, and ``integers`` the words ``h_3(p) mod high`` of the positions the library selected — which it does not pass, so they are
    recomputed from the three draws made so far, the way the library combines them."""

    def __init__(self, seed: int):
        self.seed, self.calls, self.draws = int(seed), 0, []

    def binomial(self, n, p, size):
        assert n == 1
        t = int(np.prod(size))
        u = ((words(self.seed, self.calls, t) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53).reshape(size)          # (53 bits: exact in float64)
        self.calls += 1
        hit = u < p
        self.draws.append(hit)
        return hit.astype(np.int64)

    def integers(self, low, high, size, dtype):
        assert low == 0 and len(self.draws) == 3
        masked, replaced, random = self.draws
        selected = random & masked & ~replaced
        assert int(selected.sum()) == size
        w = (words(self.seed, 3, selected.size) % np.uint64(high)).astype(dtype).reshape(selected.shape)
        return w[selected]


# ---- the dict of Collator.encode ---------------------------------------------------------------------------------------------------------------
CALL_FIXTURES = ("collate_call_mlm_random", "collate_call_clm_padded")          # the reference's Collator.__call__ on texts, fixed tokenizer
FIXTURES = ("collate_mlm_random", "collate_mlm_positives_only", "collate_clm_padded_sampled", "collate_clm_padded_fixed", "collate_mlm_padded_no_unk")
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def padded_rows(length, pad_to_multiple_of, tokenizer_sample_max=None):
    if tokenizer_sample_max is not None:
        return tokenizer_sample_max + pad_to_multiple_of
    return -(-length // pad_to_multiple_of) * pad_to_multiple_of


def encode(input_ids, special_ids, byte_lengths_per_token, surface_forms, priors, *, loss, mask_token_id=None, unk_token_id=None, seed=0, thresholds_=None,
           n_token_subsample=None, subsample_mode="random", negative_order=None, pad_to_multiple_of=8, tokenizer_sample_max=None):
    """What ``Collator.encode`` returns behind the tokenizer call (input_ids: its output with special_ids_map applied), as zett_amd defines it."""
    from tests.batch_vocab_ref import batch_vocab_ref
    v = len(priors)
    lb = label_batch(input_ids, special_ids, byte_lengths_per_token, vocab_len=v, loss=loss, mask_token_id=mask_token_id, unk_token_id=unk_token_id, seed=seed,
                     thresholds_=thresholds_)
    out = {"input_ids": lb["input_ids"], "labels": lb["labels"], "byte_lengths": lb["byte_lengths"], "metrics": lb["metrics"], "record": lb["record"]}
    if n_token_subsample is not None:
        bv = batch_vocab_ref(lb["input_ids"], lb["labels"], special_ids, n_token_subsample, surface_forms, np.asarray(priors).astype(np.float32), subsample_mode, negative_order)
        out.update({k: bv[k] for k in ("input_ids", "labels", "ids_to_embed", "target_surface_forms", "target_priors", "mask", "special_indices")})
    else:
        out.update(pad_vocabulary(surface_forms, priors, padded_rows(v, pad_to_multiple_of, tokenizer_sample_max)))
        out["special_indices"] = [int(s) for s in special_ids]
    return out


def load_fixture(name):
    """A fixture of tests/golden/make_golden_collate.py: (inputs, the dict the reference's Collator.encode returned)."""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    inputs = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    for key in ("loss", "subsample_mode"):
        inputs[key] = str(inputs[key])
    for key in ("n_token_subsample", "tokenizer_sample_max", "mask_token_id", "unk_token_id", "pad_to_multiple_of", "seed"):
        inputs[key] = None if int(inputs[key]) < 0 else int(inputs[key])
    inputs["special_ids"] = [int(x) for x in inputs["special_ids"]]
    inputs["probabilities"] = tuple(float(x) for x in inputs["probabilities"])
    return inputs, {k[4:]: z[k] for k in z.files if k.startswith("out_")}


def encode_fixture(inputs):
    return encode(inputs["input_ids"], inputs["special_ids"], inputs["byte_lengths"], inputs["surface_forms"], inputs["priors"], loss=inputs["loss"],
                  mask_token_id=inputs["mask_token_id"], unk_token_id=inputs["unk_token_id"], seed=inputs["seed"], thresholds_=thresholds(*inputs["probabilities"]),
                  n_token_subsample=inputs["n_token_subsample"], subsample_mode=inputs["subsample_mode"], negative_order=inputs["negative_order"],
                  pad_to_multiple_of=inputs["pad_to_multiple_of"], tokenizer_sample_max=inputs["tokenizer_sample_max"])


def bpe_tokenizer(mask=True):
    """The byte-level BPE tokenizer of the encode fixtures (420 ids, <s> <pad> </s> <unk> in front), with a mask token behind it."""
    import json

    from tokenizers import Tokenizer
    from transformers import PreTrainedTokenizerFast

    from tests import encode_ref as er
    tk = Tokenizer.from_str(json.dumps(er.load_fixture("encode_bpe_prefix_bos_eos_t32")["tokenizer"]))
    kw = {"mask_token": "<mask>"} if mask else {}
    return PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>", clean_up_tokenization_spaces=False, **kw)


def derived_seed(seed: int, stream: int) -> int:
    """zett_amd.collate.derived_seed, restated"""
    return mix64_int(mix64_int(int(seed)) + (int(stream) + 1) * GOLDEN)


def load_call_fixture(name):
    """A fixture of make_golden_collate.py's second kind: (inputs with the texts and data_args, the dict Collator.__call__ returned, and the
    tables Collator.__init__ prepared)."""
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    inputs = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    inputs["texts"] = [str(x) for x in inputs["texts"]]
    for key in ("loss", "subsample_mode", "lang_code"):
        inputs[key] = str(inputs[key])
    for key in ("n_token_subsample", "pad_to_multiple_of", "seed", "block_size", "hn_surface_maxlen"):
        inputs[key] = None if int(inputs[key]) < 0 else int(inputs[key])
    inputs["langs"] = [str(x) for x in inputs["langs"]]
    return inputs, {k[4:]: z[k] for k in z.files if k.startswith("out_")}, {k[5:]: z[k] for k in z.files if k.startswith("init_")}
