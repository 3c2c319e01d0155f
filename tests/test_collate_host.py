"""The definitions behind zett_amd/collate.py, without a GPU: the restatement of tests/collate_ref.py against the installed
``DataCollatorForLanguageModeling`` (with the counter-based generator injected) and against the reference's own ``Collator.encode`` dicts
(tests/golden/collate_*.npz), the thresholds, the rates the draws give, and the C interface."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import collate_ref as cr
from zett_amd import _lib
from zett_amd.collate import mlm_thresholds, padded_rows

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zett_op_label_batch", "zett_op_pad_vocabulary")
PROBABILITIES = ((0.15, 0.8, 0.1), (0.5, 1.0, 0.0), (0.3, 0.5, 0.5), (1.0, 0.0, 1.0))


class _Tokenizer:
    """What DataCollatorForLanguageModeling asks of a tokenizer when it is handed an array of ids."""
    mask_token = "<mask>"
    pad_token = "<pad>"
    pad_token_id = 0
    padding_side = "right"

    def __init__(self, vocab_len, special_ids, mask_token_id):
        self.vocab_len, self.all_special_ids, self.mask_token_id = vocab_len, list(special_ids), mask_token_id

    def __len__(self):
        return self.vocab_len

    def get_special_tokens_mask(self, ids, already_has_special_tokens=False):
        assert already_has_special_tokens
        return [1 if i in self.all_special_ids else 0 for i in ids]

    def convert_tokens_to_ids(self, token):
        assert token == self.mask_token
        return self.mask_token_id


def library_mask(ids, tokenizer, seed, probabilities):
    from transformers import DataCollatorForLanguageModeling
    collator = DataCollatorForLanguageModeling(tokenizer, mlm=True, mlm_probability=probabilities[0], mask_replace_prob=probabilities[1],
                                               random_replace_prob=probabilities[2], return_tensors="np")
    collator.generator = cr.CounterGenerator(seed)
    out = collator(ids.copy())
    return out["input_ids"], out["labels"]


@pytest.mark.parametrize("n_special", (0, 1, 5))
@pytest.mark.parametrize("probabilities", PROBABILITIES, ids=lambda p: "-".join(map(str, p)))
@pytest.mark.parametrize("shape", ((1, 1), (3, 17), (8, 64)), ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_the_library_with_the_injected_generator(shape, probabilities, n_special):
    v = 50
    special = [3, 0, 49, 7, 21][:n_special]
    rng = np.random.default_rng(shape[1] + n_special)
    table = rng.integers(1, 9, v)
    for seed in (0, 12345, 2 ** 64 - 1):
        ids = rng.integers(0, v, shape).astype(np.int64)
        if n_special:
            ids[0, 0] = special[0]
        tokenizer = _Tokenizer(v, special, 3)
        got_ids, got_labels = library_mask(ids, tokenizer, seed, probabilities)
        want = cr.label_batch(ids, special, table, vocab_len=v, loss="mlm", mask_token_id=3, unk_token_id=1, seed=seed, thresholds_=cr.thresholds(*probabilities))
        assert np.array_equal(got_ids, want["input_ids"]) and np.array_equal(got_labels, want["labels"]), (seed, shape)
        assert np.array_equal(want["byte_lengths"], table[got_ids])
        plain = np.isin(got_ids, special, invert=True)
        with np.errstate(invalid="ignore"), _quiet():
            avg, unk = table[got_ids][plain].mean() if plain.any() else np.float64("nan"), (got_ids == 1).mean()
        assert np.array_equal(want["metrics"].view(np.int64)[1:], np.array([unk]).view(np.int64))
        assert (np.isnan(avg) and np.isnan(want["metrics"][0])) or np.float64(avg).tobytes() == want["metrics"][:1].tobytes()
        r = want["record"]
        assert r[0] == ids.size and r[4] == (got_labels != -100).sum() and r[5] + r[6] <= r[4] and r[7] == 0
        if probabilities == (1.0, 0.0, 1.0):          # everything that is not special is masked, and every masked position gets a random id
            assert r[4] == (~np.isin(ids, special)).sum() == r[6] and r[5] == 0
        if probabilities[1] == 1.0:
            assert r[5] == r[4] and r[6] == 0


class _quiet:
    def __enter__(self):
        import warnings
        self.c = warnings.catch_warnings()
        self.c.__enter__()
        warnings.simplefilter("ignore")

    def __exit__(self, *a):
        return self.c.__exit__(*a)


def test_thresholds():
    two53 = 1 << 53
    assert mlm_thresholds() == (math.ceil(0.15 * two53), math.ceil(0.8 * two53), math.ceil(0.5000000000000001 * two53)) == cr.thresholds()
    assert 0.1 / (1 - 0.8) == 0.5000000000000001 and mlm_thresholds()[2] == two53 // 2 + 1          # the library's quotient, not 0.5
    assert mlm_thresholds(0.0, 0.0, 0.0) == (0, 0, 0)
    assert mlm_thresholds(1.0, 1.0, 0.0) == (two53, two53, 0)          # the library returns before the third draw
    assert mlm_thresholds(1.0, 0.5, 0.0) == (two53, two53 // 2, 0)
    assert mlm_thresholds(1.0, 0.0, 1.0) == (two53, 0, two53)
    assert mlm_thresholds(0.3, 0.5, 0.5) == (math.ceil(0.3 * two53), two53 // 2, two53)
    for p in (0.15, 0.3, 1e-300, 1 - 2 ** -53, 2 ** -53):          # k < ceil(p 2^53)  <=>  k 2^-53 < p, at the integers next to the threshold
        t = mlm_thresholds(p, 0.8, 0.1)[0]
        for k in (t - 1, t, t + 1):
            if 0 <= k < two53:
                assert (k < t) == (k * 2.0 ** -53 < p), (p, k)
    from transformers import DataCollatorForLanguageModeling
    tokenizer = _Tokenizer(10, [], 3)
    for bad in ((-0.1, 0.8, 0.1), (1.5, 0.8, 0.1), (0.15, 0.8, 0.3), (0.15, -0.1, 0.1), (0.15, 1.1, -0.2), (0.15, 0.5, -0.1), (None, 0.8, 0.1)):
        with pytest.raises(ValueError) as ours:
            mlm_thresholds(*bad)
        with pytest.raises(ValueError) as theirs:
            DataCollatorForLanguageModeling(tokenizer, mlm=True, mlm_probability=bad[0], mask_replace_prob=bad[1], random_replace_prob=bad[2])
        assert str(ours.value) == str(theirs.value), bad


@pytest.mark.parametrize("seed", (0, 1, 7))
def test_rates(seed):
    """T = 65 536 positions, none special, the default probabilities: the masked fraction, replaced given masked and random given the rest
    each within 4 binomial standard deviations of 0.15, 0.8 and 0.5 (the definition itself gives |z| <= 2.1 on these nine)."""
    t = 65536
    ids = np.full((256, 256), 5, dtype=np.int64)
    r = cr.label_batch(ids, [], np.ones(10, dtype=np.int64), vocab_len=10, loss="mlm", mask_token_id=3, seed=seed)["record"]
    masked, replaced, random = int(r[4]), int(r[5]), int(r[6])
    for hits, n, p in ((masked, t, 0.15), (replaced, masked, 0.8), (random, masked - replaced, 0.5)):
        z = (hits - n * p) / math.sqrt(n * p * (1 - p))
        assert abs(z) <= 4, (seed, hits, n, p, z)


def test_padded_rows():
    assert padded_rows(392, 8) == 392 and padded_rows(393, 8) == 400 and padded_rows(1, 128) == 128
    assert padded_rows(300, 8, tokenizer_sample_max=512) == 520 and padded_rows(520, 8, tokenizer_sample_max=512) == 520
    with pytest.raises(ValueError, match="multiple"):
        padded_rows(300, 8, tokenizer_sample_max=500)
    with pytest.raises(ValueError, match="does not fit"):
        padded_rows(521, 8, tokenizer_sample_max=512)


def test_padded_vocabulary_restatement_is_numpy_pad():
    rng = np.random.default_rng(0)
    sf, priors = rng.integers(0, 99, (13, 3)), rng.standard_normal(13)
    want = cr.pad_vocabulary(sf, priors, 16)
    assert np.array_equal(want["target_surface_forms"], np.pad(sf, ((0, 3), (0, 0)), constant_values=0))
    assert np.array_equal(want["target_priors"], np.pad(priors, (0, 3), constant_values=-100000).astype(np.float32))
    assert np.array_equal(want["mask"], np.concatenate([np.ones(13, dtype=bool), np.zeros(3, dtype=bool)]))
    assert np.array_equal(want["ids_to_embed"], np.concatenate([np.arange(13), np.zeros(3, dtype=np.int32)])) and want["ids_to_embed"].dtype == np.int64


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "zett_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", NEW)
def test_entry_points_are_declared_bound_and_exported(name):
    assert re.search(r"\bint " + name + r"\(", _header())
    assert name in _lib.ABI_SYMBOLS
    lib = _lib.load()
    assert hasattr(lib, name) and getattr(lib, name).restype is C.c_int
    assert _lib.ABI_VERSION == 8 and lib.zett_abi_version() == 8 and re.search(r"#define ZETT_ABI_VERSION 8\b", open(os.path.join(REPO, "include", "zett_hip.h")).read())
    assert re.search(r"#define ZETT_LABEL_WORKSPACE_BYTES " + str(_lib.LABEL_WORKSPACE_BYTES) + r"\b", _header())


def test_bad_arguments_are_refused_before_any_launch():
    """(no GPU: a refused call launches nothing, so host addresses do)"""
    lib = _lib.load()
    a = (C.c_int64 * 4096)()
    p = C.cast(a, C.c_void_p)
    i32 = lambda *x: (C.c_int32 * max(len(x), 1))(*x)          # noqa: E731

    def label(ids=p, ids_bytes=8, ld_in=4, b=2, s=4, special=(1,), table=p, table_bytes=8, v=10, vocab_len=10, mask_id=3, unk=-1, mode=_lib.LABEL_MLM, t=(1, 1, 1),
              out=p, ld_out=4, labels=p, lengths=p, record=p, metrics=p, work=p, work_bytes=_lib.LABEL_WORKSPACE_BYTES, n_special=None):
        return lib.zett_op_label_batch(ids, ids_bytes, ld_in, b, s, i32(*special), len(special) if n_special is None else n_special, table, table_bytes, v, vocab_len,
                                       mask_id, unk, mode, *t, 0, out, ld_out, labels, lengths, record, metrics, work, work_bytes, None)

    for kw, code in ((dict(ids=None), _lib.E_INVALID), (dict(table=None), _lib.E_INVALID), (dict(labels=None), _lib.E_INVALID), (dict(record=None), _lib.E_INVALID),
                     (dict(metrics=None), _lib.E_INVALID), (dict(work=None), _lib.E_INVALID), (dict(work_bytes=_lib.LABEL_WORKSPACE_BYTES - 1), _lib.E_INVALID),
                     (dict(ids_bytes=2), _lib.E_INVALID), (dict(table_bytes=1), _lib.E_INVALID), (dict(ld_in=3), _lib.E_INVALID), (dict(ld_out=3), _lib.E_INVALID),
                     (dict(b=0), _lib.E_INVALID), (dict(s=0), _lib.E_INVALID), (dict(v=0), _lib.E_INVALID), (dict(vocab_len=0), _lib.E_INVALID),
                     (dict(vocab_len=11), _lib.E_INVALID), (dict(mode=2), _lib.E_INVALID), (dict(special=(10,)), _lib.E_INDEX), (dict(special=(-1,)), _lib.E_INDEX),
                     (dict(n_special=257), _lib.E_INVALID), (dict(mask_id=10), _lib.E_INDEX), (dict(mask_id=-1), _lib.E_INDEX), (dict(unk=-2), _lib.E_INVALID),
                     (dict(t=((1 << 53) + 1, 0, 0)), _lib.E_INVALID)):
        assert label(**kw) == code, kw

    def pad(sf=p, sf_bytes=8, ld=3, l=3, v=5, r=8, priors=p, priors_bytes=4, out=p, out_priors=p, mask=p, ids=p):
        return lib.zett_op_pad_vocabulary(sf, sf_bytes, ld, l, v, r, priors, priors_bytes, out, out_priors, mask, ids, None)

    for kw in (dict(sf=None), dict(priors=None), dict(out=None), dict(out_priors=None), dict(mask=None), dict(ids=None), dict(sf_bytes=2), dict(priors_bytes=2),
               dict(ld=2), dict(l=0), dict(v=0), dict(r=4)):
        assert pad(**kw) == _lib.E_INVALID, kw


@pytest.mark.parametrize("name", cr.FIXTURES)
def test_restatement_equals_the_reference(name):
    """The whole dict ``Collator.encode`` of the reference returned, against the restatement on the same inputs: every array element for
    element, the metrics as float64 bits, target_priors as the float32 they reach the model as.  Under MLM with n_token_subsample the
    reference lists the label -100 as an id (the product does not), which takes one row from the negatives and moves
    the rows behind it: there input_ids and labels are compared through ``ids_to_embed[.]`` — the ids they stand for — and the rows as sets."""
    inputs, ref = cr.load_fixture(name)
    got = cr.encode_fixture(inputs)
    assert got["metrics"].tobytes() == ref["metrics"].astype(np.float64).tobytes()
    assert np.array_equal(got["byte_lengths"], ref["byte_lengths"]) and got["byte_lengths"].dtype == ref["byte_lengths"].dtype == np.int64
    assert np.array_equal(ref["attention_mask"], inputs["input_ids"] != inputs["special_ids"][0])          # (the stand-in tokenizer's own; nothing touches it)
    assert got["special_indices"] == ref["special_indices"].tolist()
    assert ref["special_indices_in_reference"].tolist() == inputs["special_ids"]
    minus_100_listed = inputs["loss"] == "mlm" and inputs["n_token_subsample"] is not None
    assert minus_100_listed == bool((ref["ids_to_embed"] == -100).any())
    if not minus_100_listed:
        for key in ("input_ids", "labels", "ids_to_embed", "target_surface_forms", "mask"):
            assert np.array_equal(got[key], ref[key]), key
        assert np.array_equal(got["target_priors"], ref["target_priors"].astype(np.float32)) and got["target_priors"].dtype == np.float32
        return
    n = inputs["n_token_subsample"]
    assert len(ref["ids_to_embed"]) == len(got["ids_to_embed"]) == n and ref["mask"].all() and got["mask"].all()
    assert np.array_equal(got["ids_to_embed"][got["input_ids"]], ref["ids_to_embed"][ref["input_ids"]])
    on = ref["labels"] != -100
    assert np.array_equal(on, got["labels"] != -100) and np.array_equal(got["ids_to_embed"][got["labels"][on]], ref["ids_to_embed"][ref["labels"][on]])
    theirs, ours = set(ref["ids_to_embed"].tolist()) - {-100}, set(got["ids_to_embed"].tolist())
    repeats = n - len(set(ref["ids_to_embed"].tolist()))          # (the reference's negatives exclude unique(input_ids) only: a label-only id can come twice, section 7f)
    assert theirs <= ours and len(ours - theirs) <= 1 + repeats          # the row -100 took, and the repeated rows, go to further negatives
    rows = {int(i): r for r, i in enumerate(got["ids_to_embed"])}
    for r, i in enumerate(ref["ids_to_embed"]):          # the rows that are there hold the same surface forms and priors
        if i != -100 and (inputs["subsample_mode"] == "random" or i != 0):
            assert np.array_equal(ref["target_surface_forms"][r], got["target_surface_forms"][rows[int(i)]])
            assert np.float32(ref["target_priors"][r]) == got["target_priors"][rows[int(i)]]


def test_the_reference_s_call_fixtures():
    """The two dicts recorded from the reference's ``Collator.__call__`` on texts (fixed tokenizer): the tables its ``__init__`` prepared have
    the shapes the dict was built from, and the padded CLM dict is the restatement of its own input_ids over those tables."""
    for name in cr.CALL_FIXTURES:
        inputs, ref, init = cr.load_call_fixture(name)
        v = len(init["scores"])
        assert init["surface_forms"].shape == (v, inputs["hn_surface_maxlen"]) and init["byte_lengths"].shape == (v,) and int(init["original_length"]) <= v
        assert len(inputs["texts"]) == ref["attention_mask"].shape[0] and ref["attention_mask"].shape[1] == inputs["block_size"]
        assert ref["special_indices_in_reference"].tolist() == init["special_ids"].tolist()          # the tokenizer is the reference here
    inputs, ref, init = cr.load_call_fixture("collate_call_clm_padded")
    got = cr.encode(ref["input_ids"], init["special_ids"].tolist(), init["byte_lengths"], init["surface_forms"], init["scores"], loss="clm", unk_token_id=3,
                    pad_to_multiple_of=inputs["pad_to_multiple_of"])
    assert got["metrics"].tobytes() == ref["metrics"].tobytes()
    for key in ("input_ids", "labels", "byte_lengths", "target_surface_forms", "mask", "ids_to_embed"):
        assert np.array_equal(got[key], ref[key]), key
    assert np.array_equal(got["target_priors"], ref["target_priors"].astype(np.float32)) and got["special_indices"] == ref["special_indices"].tolist()
