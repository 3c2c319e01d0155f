"""Added tokens split out of texts, on the host (no GPU): the restatement of tests/encode_added_ref.py against the installed
``tokenizers`` on every measured fact of DESIGN.md section 7g ("the cut step") and on seeded random texts, and what
``EncodeSpec(split_added_tokens=True)`` splits, refuses per call, refuses outright and leaves alone.

The tokenizers are the fixtures' (tests/golden/encode_*.json.gz) with another ``added_tokens`` list: Unigram behind Split + ByteLevel
with ``Prepend(" ")`` (PREFIX_ALWAYS) or nothing (PREFIX_NONE), BPE behind ByteLevel with ``add_prefix_space`` (PREFIX_UNLESS_SPACE) or
without.  The library renumbers an added token whose id lies beyond the model's vocabulary, so new tokens get the ids v, v + 1, ..."""
import json

import numpy as np
import pytest

from tests import encode_added_ref as ar
from tests import encode_ref as er
from tests.sampled_vocab_cases import CASES, case_pieces, stand_in_reference
from zett_amd import text_encode as te

ALWAYS, NONE_U, UNLESS, NONE_B = "encode_unigram_prefix_bos_eos_t32", "encode_unigram_noprefix_bos_t8", "encode_bpe_prefix_bos_eos_t32", "encode_bpe_noprefix_nopost_t8"
NAMES = (ALWAYS, NONE_U, UNLESS, NONE_B)


def _tokens(fx):
    """</s> at its own row of the vocabulary, the overlap set and a multi-byte token behind the vocabulary"""
    v = len(fx["tokenizer"]["model"]["vocab"])
    return [("</s>", 2), ("<x>", v), ("<x><y>", v + 1), ("x><", v + 2), ("<é中>", v + 3)]


def _setup(name, **flags):
    fx = er.load_fixture(name)
    data = ar.with_added_tokens(fx["tokenizer"], _tokens(fx), **flags)
    return fx, data, ar.library(data), dict(_tokens(fx))


def _ours(fx, toks, text):
    spec = fx["spec"]
    return ar.text_ids(text, toks, spec.prefix_mode, spec.marks_are_letters, fx["segment"], spec.resplit)


def _pieces(tk, text):
    return tk.encode(text, add_special_tokens=False).tokens


def _sections(tk, text, toks):
    """the library's pieces with those of one section joined (how a small model cuts a section is not the point): ``Ġa </s> ĠĠb``"""
    out, run = [], ""
    for piece in _pieces(tk, text) + [None]:
        if piece is None or piece in toks:
            out += [run] if run else []
            out += [piece] if piece is not None else []
            run = ""
        else:
            run += piece
    return out


def test_fixtures_cover_the_modes():
    specs = {n: er.load_fixture(n)["spec"] for n in NAMES}
    assert [specs[n].prefix_mode for n in NAMES] == [te.PREFIX_ALWAYS, te.PREFIX_NONE, te.PREFIX_UNLESS_SPACE, te.PREFIX_NONE]
    assert [er.load_fixture(n)["tokenizer"]["model"]["type"] for n in NAMES] == ["Unigram", "Unigram", "BPE", "BPE"]
    assert [er.load_fixture(n)["tokenizer"]["pre_tokenizer"]["type"] for n in NAMES] == ["Sequence", "Sequence", "ByteLevel", "ByteLevel"]


def test_cut_is_leftmost_longest():
    toks = {"<x>": 1, "<x><y>": 2, "x><": 3}
    assert ar.cut("a<x><y>b", toks) == ["a", 2, "b"]
    assert ar.cut("<x><x><y>", toks) == [1, 2]
    assert ar.cut("a<x><", toks) == ["a", 1, "<"]
    assert ar.cut("<<x>>", toks) == ["<", 1, ">"]
    assert ar.cut("", toks) == [] and ar.cut("<x>", toks) == [1] and ar.cut("ax><", toks) == ["a", 3]


@pytest.mark.parametrize("name", NAMES)
def test_measured_facts_against_the_library(name):
    """items 2 and 3 of the issue: the pieces the library gives, and the restatement's ids equal to the library's"""
    fx, data, tk, toks = _setup(name)
    mode = fx["spec"].prefix_mode
    g = "Ġ"
    lead = g if mode != te.PREFIX_NONE else ""
    sec = lambda text: _sections(tk, text, toks)          # noqa: E731
    assert sec("a<x><y>b") == [lead + "a", "<x><y>", lead + "b"]
    assert _pieces(tk, "<x><x><y>") == ["<x>", "<x><y>"]
    assert sec("a<x><") == [lead + "a", "<x>", lead + "<"]
    assert sec("<<x>>") == [lead + "<", "<x>", lead + ">"]
    assert tk.encode("</s>", add_special_tokens=False).ids == [2]          # exactly one id, a row of the vocabulary
    if mode == te.PREFIX_ALWAYS:
        assert sec("a</s> b") == [g + "a", "</s>", g + g + "b"]
        assert sec("</s></s>a") == ["</s>", "</s>", g + "a"]
        assert sec(" </s>") == [g + g, "</s>"]
    elif mode == te.PREFIX_UNLESS_SPACE:
        assert sec("a</s> b") == [g + "a", "</s>", g + "b"]
        assert sec("a</s>b") == [g + "a", "</s>", g + "b"]
    else:
        assert sec("a</s>b") == ["a", "</s>", "b"]
        assert sec("a  </s>  b") == ["a" + g + g, "</s>", g + g + "b"]
        assert sec("a</s>'s") == ["a", "</s>", "'s"]
        if fx["tokenizer"]["model"]["type"] == "Unigram":          # (a word is a run of pieces: the model's unigrams of one character)
            pre = ar.library(data).pre_tokenizer
            assert [w for w, _ in pre.pre_tokenize_str("a  ")] == ["a", g + g]          # \s+(?!\S) gives nothing back in front of a match,
            assert [w for w, _ in pre.pre_tokenize_str("a  b")] == ["a", g, g + "b"]          # as it does in front of a letter
            assert [w for w, _ in pre.pre_tokenize_str("'s")] == ["'s"]          # a contraction can start a section
    examples = ["a</s>b", "a<x><y>b", "<x><x><y>", "a<x><", "<<x>>", "a</s> b", "</s></s>a", " </s>", "a  </s>  b", "a</s>'s", "</s>", "", " ", "中</s>é",
                "a<é中>b", "</s> </s>", "a </s>", "a\n\n</s>\n\nb", "x</s>'ll do", "<x><y><x>", "x><x>"]
    for text in examples:
        assert _ours(fx, toks, text) == tk.encode(text, add_special_tokens=False).ids, (name, text)


@pytest.mark.parametrize("name", NAMES)
def test_random_texts_against_the_library(name):
    fx, data, tk, toks = _setup(name)
    rng = np.random.default_rng(20241)
    strings = [c for c, _ in _tokens(fx)]
    texts = [ar.random_text(rng, strings) for _ in range(300)]
    cuts = [ar.cut(t, toks) for t in texts]
    assert sum(any(isinstance(p, int) for p in c) for c in cuts) >= 100          # at least a third hold a match
    assert sum(any(isinstance(a, int) and isinstance(b, int) for a, b in zip(c, c[1:])) for c in cuts) >= 5          # and some two adjacent ones
    for text in texts:
        assert _ours(fx, toks, text) == tk.encode(text, add_special_tokens=False).ids, (name, text)


def test_normalized_and_strip_flags_in_the_library():
    """item 4: without a normalizer ``normalized=True`` changes nothing; under Prepend the token is looked for in the normalized text;
    lstrip / rstrip swallow the whitespace next to the match — which is why those keep the refusal"""
    for name in (NONE_U, UNLESS):
        fx, data, tk, toks = _setup(name)
        tkn = ar.library(ar.with_added_tokens(fx["tokenizer"], _tokens(fx), normalized=True))
        for text in ("a</s>b", "a </s> b", "</s>", "a<x><y>"):
            assert tkn.encode(text, add_special_tokens=False).ids == tk.encode(text, add_special_tokens=False).ids
    fx, data, tk, toks = _setup(ALWAYS)
    tkn = ar.library(ar.with_added_tokens(fx["tokenizer"], _tokens(fx), normalized=True))
    assert tkn.encode("a</s>b", add_special_tokens=False).ids != tk.encode("a</s>b", add_special_tokens=False).ids
    for flag in ("lstrip", "rstrip"):
        tks = ar.library(ar.with_added_tokens(fx["tokenizer"], _tokens(fx), **{flag: True}))
        assert tks.encode("a </s> b", add_special_tokens=False).ids != tk.encode("a </s> b", add_special_tokens=False).ids


def test_a_sampled_tokenizer_has_no_backend_added_tokens():
    """item 1: built the way Collator.sample_tokenizer builds one, the eos string is ordinary text"""
    from zett_amd.tokenizer_sampling import build_sampled_tokenizer
    case = CASES["ids_0123"]
    reference = stand_in_reference(case["specials"])
    tokenizer = build_sampled_tokenizer(case_pieces("ids_0123", 40), reference, True)[0]
    assert json.loads(tokenizer._tokenizer.to_str())["added_tokens"] == []
    eos = reference.eos_token
    assert eos and eos in tokenizer.all_special_tokens and len(eos) > 2
    ids = tokenizer._tokenizer.encode("a" + eos + "b", add_special_tokens=False).ids
    assert len(ids) > 3 and tokenizer.convert_tokens_to_ids(eos) not in ids          # cut into pieces like any text
    assert "".join(tokenizer.convert_ids_to_tokens(ids)) == "Ġa" + eos + "b"
    spec = te.EncodeSpec.from_tokenizer(tokenizer, split_added_tokens=True)
    assert spec.split_added_tokens and spec.added_tokens == () and spec.refused_strings == () and len(spec.added_table()[2]) == 0
    assert eos in spec.special_strings
    assert spec.check_call(["a" + eos + "b"], 8, None)[0] == "a" + eos + "b"          # neither split nor refused
    with pytest.raises(NotImplementedError):
        te.EncodeSpec.from_tokenizer(tokenizer).check_call(["a" + eos + "b"], 8, None)          # the default mode refuses as before


def _spec(data, **kw):
    return te.EncodeSpec.from_tokenizer_json(data, 1, **kw)


def test_default_spec_is_unchanged():
    fx, data, tk, toks = _setup(UNLESS)
    spec = _spec(data)
    assert spec.split_added_tokens is False and spec.added_tokens == () and spec.refused_strings == spec.special_strings
    assert set(spec.special_strings) == set(toks) and spec.added_table()[1].tolist() == [0]
    with pytest.raises(NotImplementedError, match="</s>"):
        spec.check_call(["fine", "a</s>b"], 8, None)
    assert spec.check_call(["ends <", "/s> starts"], 8, None)[0] == "ends </s> starts"
    assert spec == te.EncodeSpec(spec.prefix_mode, spec.marks_are_letters, spec.resplit, spec.prefix_ids, spec.suffix_ids, spec.pad_id, spec.special_strings)


def test_plain_tokens_make_the_table():
    fx, data, tk, toks = _setup(UNLESS)
    spec = _spec(data, split_added_tokens=True)
    assert spec.split_added_tokens and {a.content: a.id for a in spec.added_tokens} == toks and all(spec.is_plain(a) for a in spec.added_tokens)
    assert spec.refused_strings == ()
    raw, offsets, ids = spec.added_table()
    keys = [raw[offsets[k]:offsets[k + 1]] for k in range(len(ids))]
    assert keys == sorted(c.encode() for c in toks) and [toks[k.decode()] for k in keys] == ids.tolist()
    assert offsets.dtype == np.int32 and ids.dtype == np.int32 and offsets[0] == 0 and offsets[-1] == len(raw)
    assert keys.index(b"<x>") + 1 == keys.index(b"<x><y>")          # a token right before the longer one it starts
    assert spec.check_call(["a</s>b", "<x><y>"], 8, None)[0] == "a</s>b<x><y>"
    # strings that are only in all_special_tokens are neither split nor refused
    spec.special_strings = tuple(sorted(set(spec.special_strings) | {"<mask>"}))
    assert spec.check_call(["a<mask>b"], 8, None)[0] == "a<mask>b"
    # normalized=True under no normalizer counts as plain
    assert _spec(ar.with_added_tokens(fx["tokenizer"], _tokens(fx), normalized=True), split_added_tokens=True).refused_strings == ()
    assert _spec(ar.with_added_tokens(er.load_fixture(NONE_U)["tokenizer"], [("</s>", 2)], normalized=True), split_added_tokens=True).refused_strings == ()


@pytest.mark.parametrize("case", ("lstrip", "rstrip", "single_word", "one_byte", "normalized_under_prepend"))
def test_tokens_that_keep_the_per_call_refusal(case):
    name = ALWAYS if case == "normalized_under_prepend" else UNLESS
    fx = er.load_fixture(name)
    v = len(fx["tokenizer"]["model"]["vocab"])
    odd = ("|", v) if case == "one_byte" else ("<odd>", v)
    data = ar.with_added_tokens(fx["tokenizer"], [("</s>", 2)])
    flags = {} if case == "one_byte" else {"normalized" if case == "normalized_under_prepend" else case: True}
    data["added_tokens"] += ar.with_added_tokens(fx["tokenizer"], [odd], **flags)["added_tokens"]
    spec = _spec(data, split_added_tokens=True)
    assert spec.refused_strings == (odd[0],)
    raw, offsets, ids = spec.added_table()
    assert raw == b"</s>" and ids.tolist() == [2]
    assert spec.check_call(["a</s>b", "no such token"], 8, None)[0] == "a</s>bno such token"          # only when a text holds the string
    with pytest.raises(NotImplementedError, match=r"\|" if case == "one_byte" else "<odd>"):
        spec.check_call(["a</s>b", "x" + odd[0] + "y"], 8, None)
    if case != "one_byte":
        assert spec.check_call(["x" + odd[0][:1], odd[0][1:] + "y"], 8, None)[1] == []          # across two texts: in neither


def test_cap_refusals():
    fx = er.load_fixture(UNLESS)
    v = len(fx["tokenizer"]["model"]["vocab"])
    assert te.MAX_ADDED_TOKENS >= 300 and te.MAX_ADDED_TOKEN_BYTES >= 48
    many = [(("<|reserved_special_token_%03d|>" % k).ljust(48, "."), v + k) for k in range(300)]
    assert all(len(c) == 48 for c, _ in many)
    assert len(_spec(ar.with_added_tokens(fx["tokenizer"], many), split_added_tokens=True).added_table()[2]) == 300
    at_cap = [("<|%d|>" % k, v + k) for k in range(te.MAX_ADDED_TOKENS)]
    assert len(_spec(ar.with_added_tokens(fx["tokenizer"], at_cap), split_added_tokens=True).added_table()[2]) == te.MAX_ADDED_TOKENS
    with pytest.raises(NotImplementedError, match="added tokens"):
        _spec(ar.with_added_tokens(fx["tokenizer"], at_cap + [("<|over|>", v + len(at_cap))]), split_added_tokens=True)
    longest = "<" + "a" * (te.MAX_ADDED_TOKEN_BYTES - 2) + ">"
    assert _spec(ar.with_added_tokens(fx["tokenizer"], [(longest, v)]), split_added_tokens=True).added_table()[1].tolist() == [0, te.MAX_ADDED_TOKEN_BYTES]
    with pytest.raises(NotImplementedError, match="bytes"):
        _spec(ar.with_added_tokens(fx["tokenizer"], [(longest + "a", v)]), split_added_tokens=True)
    with pytest.raises(NotImplementedError, match="bytes"):          # bytes, not characters
        _spec(ar.with_added_tokens(fx["tokenizer"], [("<" + "中" * 21 + ">", v)]), split_added_tokens=True)
    _spec(ar.with_added_tokens(fx["tokenizer"], at_cap + [("<|over|>", v + len(at_cap))]))          # the default mode does not look at the table


def test_host_work_does_not_grow_with_the_plain_tokens():
    """no str.find per splittable token: check_call looks for the refused strings alone"""
    fx = er.load_fixture(UNLESS)
    v = len(fx["tokenizer"]["model"]["vocab"])
    spec = _spec(ar.with_added_tokens(fx["tokenizer"], [("<|%d|>" % k, v + k) for k in range(256)]), split_added_tokens=True)
    assert spec.refused_strings == () and len(spec.added_tokens) == 256
