"""Tokenizer sampling on the host: the definition (tests/sampler_ref.py) against hand-computed tables and the library, and the host half of
``sample_tokenizer`` (zett_amd/tokenizer_sampling.py) against what the reference's ``Collator.sample_tokenizer`` returned
(tests/golden/sample_tokenizer_*.json.gz).  No GPU."""
import json
import math
import os
import re

import numpy as np
import pytest

from tests import encode_ref
from tests import sampler_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the definition ----------------------------------------------------------------------------------------------------------------------
def test_pre_tokens_are_the_library_words_with_character_offsets():
    """500 seeded texts: the pre-tokens tile the sentence, their bytes are the UTF-8 of their character ranges, and the words are those
    of the split pattern without marks as tests/encode_ref.py's state machine finds them."""
    rng = np.random.default_rng(2024)
    n_words = 0
    for i in range(500):
        sentence = " " + (R.random_prose(rng, 12) if i % 3 == 0 else R.random_text(rng))
        got = R.pre_tokens(sentence)
        library = R.pre_tokenizer().pre_tokenize_str(sentence)
        assert [R.byte_level(raw) for raw, _ in got] == [piece for piece, _ in library]
        at = 0
        for raw, (o0, o1) in got:
            assert o0 == at and o1 > o0 and raw == sentence[o0:o1].encode("utf-8")
            at = o1
        assert at == len(sentence)
        assert [sentence[o0:o1] for _, (o0, o1) in got] == encode_ref.split_words(sentence, False)
        n_words += len(got)
    assert n_words > 5000


def test_table_of_the_empty_text():
    # " " is one pre-token, the first of its text: the start list is [0, 0], and "Ġ" is two UTF-8 bytes
    assert R.count_substrings([""]) == {b" ": 4}
    assert R.SamplerRef().sample_tokenizer([""], 1000)[:1] == [(R.byte_level(b"\x00"), 0.0)]


def test_table_with_stride_4():
    assert R.starts_of(" abcdefghij", 0, 0, 11, 4) == [0, 3, 7]
    want = {}
    for start in (0, 3, 7):
        for k in range(1, 12 - start):
            key = b" abcdefghij"[start:start + k]
            want[key] = len(key) + (1 if key.startswith(b" ") else 0)
    assert len(want) == 23 and R.count_substrings(["abcdefghij"], 16, 4) == want


def test_table_of_duplicate_multibyte_texts():
    """The duplicate counts once; starts 2 and 5 lie inside é and 日."""
    e, j = "é".encode(), "日".encode()
    word = b" " + e + j + b"x"
    assert R.starts_of(" é日x", 0, 0, 4, 1) == [0, 0, 2, 5, 6]
    want = {}
    for k, score in zip(range(1, 8), (4, 8, 12, 16, 20, 24, 26)):          # start 0, twice
        want[word[:k]] = score
    for k, score in zip(range(1, 6), (2, 4, 6, 8, 9)):
        want[word[2:2 + k]] = score
    want[word[5:6]], want[word[5:7]], want[word[6:7]] = 2, 3, 1
    assert R.count_substrings(["é日x", "é日x"]) == want


@pytest.mark.parametrize("n", [15, 16, 17])
def test_table_of_one_long_word(n):
    """A word of n bytes with its prefix space, stride 1, max_length 16: keys stop at 15 bytes."""
    want = {b" " + b"x" * j: 2 * (2 + j) for j in range(0, 15)}
    want.update({b"x" * m: m * (n - m) for m in range(1, min(15, n - 1) + 1)})
    got = R.count_substrings(["x" * (n - 1)])
    assert got == want and max(map(len, got)) == 15


def _sum(*texts):
    out = {}
    for t in texts:
        for k, v in R.count_substrings([t]).items():
            out[k] = out.get(k, 0) + v
    return out


@pytest.mark.parametrize("pop_prev,push_current", [(False, False), (False, True), (True, False), (True, True)])
def test_queue_over_four_calls(pop_prev, push_current):
    s = R.SamplerRef()
    s.sample(["p1"], 0, pop_prev=False)
    s.sample(["p2"], 0, pop_prev=False)
    queue = ["p2", "p1"]          # front first
    for t in ("t1", "t2", "t3", "t4"):
        out = s.sample([t], 1000, 16, 1, 0.0, pop_prev, push_current)
        if pop_prev:
            merged = [t] + queue[:-1]          # the oldest left before the sum
            assert s.merged == _sum(*merged)
            assert len(out) > 391
            if push_current:
                queue = merged
        else:
            assert out == []
            if push_current:
                queue = [t] + queue
        assert [dict(q) for q in s.queue] == [R.count_substrings([x]) for x in queue]


def test_seed_size_edges():
    texts = ["hello world, it's me"]
    kept = [k for k in R.count_substrings(texts) if not R.is_fixed(k)]
    for seed_size, n in ((0, 392), (391, 392), (392, 392), (393, 393), (10 ** 6, 391 + len(kept))):
        out = R.SamplerRef().sample(texts, seed_size)
        assert len(out) == n
        assert [k for k, _ in out[:256]] == [bytes([b]) for b in range(256)]
        assert [k for k, _ in out[256:391]] == R.whitespace_runs(16) and all(s == 0.0 for _, s in out[256:391])
        assert out[256][0] == b"  " and out[258][0] == b"\t " and out[259][0] == b"   " and out[390][0] == b"\t" * 16
    assert R.SamplerRef().sample(texts, 1000, pop_prev=False) == []
    assert len(R.SamplerRef().sample(texts, 1000, max_length=2)) == 256 + 9 + len([k for k in R.count_substrings(texts, 2) if not R.is_fixed(k)])


def test_output_order_and_scores():
    texts = ["aa ab", "ab  \n x"]
    s = R.SamplerRef()
    out = s.sample(texts, 10 ** 6)
    total = sum(s.merged.values())
    assert out[0][1] == math.log(min(s.merged.values()) / total)
    tail = out[391:]
    assert all(len(k) > 1 and sum(b in R.WHITESPACE_BYTES for b in k) < 2 for k, _ in tail)
    assert [k for k, _ in tail] == sorted((k for k, _ in tail), key=lambda k: (-s.merged[k], len(k), k))
    assert all(score == math.log(s.merged[k] / total) for k, score in tail)
    z = {k: (-1.0 if k == tail[0][0] else 0.5) for k in s.merged}
    noisy = R.SamplerRef().sample(texts, 10 ** 6, noise_std=1.0, noise=lambda k: z[k])
    assert noisy[-1] == (tail[0][0], R.FLOOR) and noisy[391][1] == math.log(s.merged[noisy[391][0]] / total + 0.5)


def test_the_library_accepts_the_output():
    from tokenizers import Tokenizer, models
    out = R.SamplerRef().sample_tokenizer(["hello world, it's me", "é日x  \n\tok"], 2000)
    tk = Tokenizer(models.Unigram(out))
    assert tk.get_vocab_size() == len(out)


def test_five_standard_errors_hold_a_numpy_normal_sample():
    """The bounds tests/test_sampler_gpu.py puts on z: a sample of a correct generator stays inside them."""
    for seed in range(20):
        z = np.random.default_rng(seed).standard_normal(20000)
        n = len(z)
        assert abs(z.mean()) <= 5 / math.sqrt(n) and abs(z.var() - 1) <= 5 * math.sqrt(2 / n)


# ---- the host half against the reference's Collator.sample_tokenizer -----------------------------------------------------------------------
_fixture, _tokenizer_of, StandIn = R.load_fixture, R.tokenizer_of, R.StandInSampler


@pytest.mark.parametrize("name", R.FIXTURES)
def test_host_half_equals_the_reference(name):
    from zett_amd.tokenizer_sampling import sample_tokenizer
    fx = _fixture(name)
    assert any(p == "<s>" for p, _ in fx["prepared"]) and fx["special_ids_map"]
    sampler = StandIn([(p, s) for p, s in fx["prepared"]])
    call = fx["sampler_call"]
    tokenizer, special_ids_map, surface_forms, priors, byte_lengths = sample_tokenizer(
        fx["texts"], sampler, _tokenizer_of(fx["reference"]), n_total=call["n_total"], noise_std=call["noise_std"], add_prefix_space=fx["add_prefix_space"])
    assert sampler.calls == [(call["counts"], call["n_total"], call["max_length"], call["stride"], call["noise_std"], call["pop_prev"], call["push_current"])]
    assert surface_forms is None          # no hn_tokenizer: the matrix is a device computation (tests/test_sampler_gpu.py)
    assert tokenizer.convert_ids_to_tokens(range(len(tokenizer))) == fx["pieces"]
    assert priors.dtype == np.float64 and priors.tolist() == fx["scores"]
    assert [[k, v] for k, v in special_ids_map.items()] == fx["special_ids_map"]
    assert byte_lengths.tolist() == fx["byte_lengths"]
    assert json.loads(tokenizer._tokenizer.to_str()) == fx["tokenizer"]
    assert list(tokenizer.all_special_tokens) == fx["special_tokens"] and list(tokenizer.all_special_ids) == fx["special_ids"]
    assert tokenizer.pad_token_id == fx["pad_token_id"]
    # the encoder takes it (its refusals run on the host, before any device work)
    from zett_amd.text_encode import PREFIX_ALWAYS, PREFIX_NONE, EncodeSpec
    spec = EncodeSpec.from_tokenizer(tokenizer)
    assert spec.prefix_mode == (PREFIX_ALWAYS if fx["add_prefix_space"] else PREFIX_NONE) and spec.marks_are_letters
    assert spec.prefix_ids == (0,) and spec.suffix_ids == (2,)


def test_validation_does_not_push():
    from zett_amd.tokenizer_sampling import sample_tokenizer
    fx = _fixture("sample_tokenizer_prefix")
    sampler = StandIn([(p, s) for p, s in fx["prepared"]])
    sample_tokenizer(["a", "a", "b"], sampler, _tokenizer_of(fx["reference"]), n_total=500, noise_std=0.25, add_prefix_space=False, is_validation=True)
    assert sampler.calls == [({"a": 1, "b": 1}, 500, 16, 4, 0.25, True, False)]


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_the_host(monkeypatch):
    import torch

    from zett_amd import tokenizer_sampling as ts
    with pytest.raises(NotImplementedError, match="count 2"):
        ts._texts_of({"a": 1, "b": 2})
    with pytest.raises(TypeError):
        ts._texts_of("one string")
    with pytest.raises(TypeError):
        ts._texts_of(["a", b"b"])
    assert ts._texts_of(["b", "a", "b", ""]) == ["b", "a", ""] and ts._texts_of({"x": 1, "y": True}) == ["x", "y"]
    fx = _fixture("sample_tokenizer_prefix")
    reference = _tokenizer_of(fx["reference"])
    with pytest.raises(ValueError, match="no pieces"):
        ts.sample_tokenizer(["a"], StandIn([]), reference, n_total=10, noise_std=0.0, add_prefix_space=True)
    with pytest.raises(ValueError, match="hn_surface_maxlen"):
        ts.sample_tokenizer(["a"], StandIn([("a", 0.0)]), reference, n_total=10, noise_std=0.0, add_prefix_space=True, hn_tokenizer=reference)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ts.DeviceTokenizerSampler()
    with pytest.raises(RuntimeError, match="no CPU path"):
        ts.DeviceTokenizerSampler(device="cpu")
    for bit, error in ((ts.SAMPLE_BAD_OFFSETS, ValueError), (ts.SAMPLE_TABLE_FULL, RuntimeError), (ts.SAMPLE_LIST_FULL, RuntimeError),
                       (ts.SAMPLE_SUM_OVERFLOW, OverflowError), (ts.SAMPLE_OUT_FULL, RuntimeError)):
        with pytest.raises(error):
            ts.raise_for_status(bit)
    ts.raise_for_status(0)
    assert ts.n_fixed_pieces(16) == 391 and ts.n_fixed_pieces(2) == 265


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_abi_is_additive():
    from zett_amd import _lib
    with open(os.path.join(REPO, "include", "zett_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define ZETT_ABI_VERSION 8\b", header)
    names = ("zett_sampler_create", "zett_sampler_destroy", "zett_sampler_depth", "zett_sampler_workspace_bytes", "zett_sampler_sample", "zett_sampler_table")
    lib = _lib.load()
    for name in names:
        assert re.search(r"\bint " + name + r"\(", header) and name in _lib.ABI_SYMBOLS and hasattr(lib, name)
    for name, value in (("BAD_OFFSETS", 2), ("TABLE_FULL", 4), ("LIST_FULL", 8), ("SUM_OVERFLOW", 16), ("OUT_FULL", 32)):
        assert re.search(r"ZETT_SAMPLE_" + name + r" = " + str(value) + r"\b", header) and getattr(_lib, "SAMPLE_" + name) == value
    assert _lib.SAMPLE_BAD_OFFSETS == _lib.ENCODE_BAD_OFFSETS          # the shared classify kernel sets it
    import ctypes as C
    n = C.c_int64(0)
    assert lib.zett_sampler_workspace_bytes(1000, 10, C.byref(n)) == 0 and 0 < n.value < 1000 * 64
    assert lib.zett_sampler_workspace_bytes(-1, 0, C.byref(n)) < 0 and lib.zett_sampler_workspace_bytes(1 << 30, 0, C.byref(n)) < 0
