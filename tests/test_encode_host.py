"""Text encoding on the host (no GPU): the plain-Python restatement of tests/encode_ref.py against the reference's own outputs
(tests/golden/encode_*.json.gz) and against the installed ``tokenizers``, the class table of zett_amd/text_encode.py against direct
probes of the library, and every refusal of DESIGN.md section 7g."""
import copy
import json
import unicodedata

import numpy as np
import pytest

from tests import encode_ref as er
from zett_amd import text_encode as te


@pytest.mark.parametrize("name", er.FIXTURES)
def test_restatement_equals_the_reference(name):
    fx = er.load_fixture(name)
    ids, mask = er.encode_with(fx["spec"], fx["segment"], fx["texts"], fx["block_size"], fx["map"])
    assert np.array_equal(ids, np.array(fx["input_ids"])) and np.array_equal(mask, np.array(fx["attention_mask"]))
    assert len(fx["texts"]) == 8 and ids.shape == (8, fx["block_size"])


def test_fixtures_cover_the_cases():
    specs = [er.load_fixture(n)["spec"] for n in er.FIXTURES]
    assert {s.prefix_mode for s in specs} == {te.PREFIX_NONE, te.PREFIX_ALWAYS, te.PREFIX_UNLESS_SPACE}
    assert {(len(s.prefix_ids), len(s.suffix_ids)) for s in specs} == {(1, 1), (1, 0), (0, 0)}
    assert {s.marks_are_letters for s in specs} == {True, False}
    assert {er.load_fixture(n)["block_size"] for n in er.FIXTURES} == {8, 32}
    assert any(er.load_fixture(n)["map"] for n in er.FIXTURES)
    for n in er.FIXTURES:          # the map changes something, and in order: a -> b -> c
        fx = er.load_fixture(n)
        if fx["map"]:
            plain, _ = er.encode_with(fx["spec"], fx["segment"], fx["texts"], fx["block_size"], None)
            (a, b), (b2, c) = list(fx["map"].items())[:2]
            assert b == b2 and (plain == a).any() and not (np.array(fx["input_ids"]) == b).any()


def test_examples_of_the_definition():
    assert er.split_words("\"'s", True) == ["\"'", "s"]
    assert er.split_words("x'd'd", True) == ["x", "'d", "'d"]
    assert er.split_words("a  's", True) == ["a", " ", " '", "s"]
    assert er.split_words("x'D", True) == ["x", "'", "D"]          # case-sensitive
    assert er.split_words("a\u00a0b", True) == ["a", "\u00a0", "b"] and er.split_words("a b", True) == ["a", " b"]          # ` ?` is U+0020 only
    assert er.split_words("\u0301.", True) == ["\u0301", "."] and er.split_words("\u0301.", False) == ["\u0301."]
    assert er.split_words("e\u0301", True) == ["e\u0301"] and er.split_words("e\u0301", True, True) == ["e", "\u0301"]


def test_split_equals_the_library_on_random_texts():
    import tokenizers
    from tokenizers import pre_tokenizers
    marks, plain = er.library_pre_tokenizers()
    both = pre_tokenizers.Sequence([marks, pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)])
    rng = np.random.default_rng(20240)
    for _ in range(2000):
        text = er.random_text(rng)
        for pre, marks_are_letters, resplit in ((marks, True, False), (plain, False, False), (both, True, True)):
            want = [text[s:e] for _, (s, e) in pre.pre_tokenize_str(text)]
            assert er.split_words(text, marks_are_letters, resplit) == want, (text, marks_are_letters, resplit)


def test_class_table_agrees_with_direct_probes():
    table = te.class_table()
    assert table.shape == (0x110000,) and te.class_table() is table
    rng = np.random.default_rng(5)
    newer = [c for c in range(0x32000) if table[c] == te.CLASS_L and unicodedata.category(chr(c)) == "Cn"]          # (choosing the points, not judging them)
    assert len(newer) > 1000
    points = np.concatenate([np.arange(0x100), rng.integers(0x100, 0x32000, size=2800), rng.choice(newer, size=1500, replace=False),
                             rng.integers(0xE0000, 0xE0200, size=250), rng.integers(0x32000, 0x110000, size=250)])
    points = points[(points < 0xD800) | (points > 0xDFFF)]
    points = points[:5000]
    assert len(points) == 5000
    for c in points.tolist():
        assert er.probe_class(chr(c)) == table[c], hex(c)
    packed = te.pack_class_table(table)
    for c in (0x20, 0x41, 0x301, 0x31, 0x2E, 0x10FFFF):
        assert (packed[c >> 1] >> (4 * (c & 1))) & 7 == table[c]


@pytest.mark.parametrize("name", er.FIXTURES)
def test_prefix_modes_against_the_library(name):
    from tokenizers import Tokenizer
    fx = er.load_fixture(name)
    tk = Tokenizer.from_str(json.dumps(fx["tokenizer"]))
    tk.no_padding()
    tk.no_truncation()
    spec = fx["spec"]
    for text in ("", " ", "a", " a", "  a", "\ta", " a", "'s", " 's"):
        want = tk.encode(text, add_special_tokens=False).ids
        assert er.text_ids(text, spec.prefix_mode, spec.marks_are_letters, fx["segment"], spec.resplit) == want, (name, text)
    assert tk.encode("", add_special_tokens=False).ids == []          # an empty text gets no prefix in any mode


def _spec(data, **kw):
    args = dict(pad_id=1, padding_side="right", truncation_side="right")
    args.update(kw)
    return te.EncodeSpec.from_tokenizer_json(data, args["pad_id"], args["padding_side"], args["truncation_side"])


def test_refusals():
    base = er.load_fixture("encode_unigram_prefix_bos_eos_t32")["tokenizer"]
    bpe = er.load_fixture("encode_bpe_prefix_bos_eos_t32")["tokenizer"]
    _spec(base), _spec(bpe)

    def changed(data, path, value):
        out = copy.deepcopy(data)
        node = out
        for key in path[:-1]:
            node = node[key]
        node[path[-1]] = value
        return out
    for data in (changed(base, ["normalizer"], {"type": "NFC"}), changed(base, ["normalizer"], {"type": "Prepend", "prepend": "_"}),
                 changed(base, ["pre_tokenizer"], {"type": "Whitespace"}), changed(base, ["pre_tokenizer"], None),
                 changed(base, ["pre_tokenizer", "pretokenizers", 0, "pattern"], {"Regex": r"\s+"}),
                 changed(base, ["pre_tokenizer", "pretokenizers", 0, "behavior"], "Isolated"),
                 changed(base, ["pre_tokenizer", "pretokenizers", 1, "add_prefix_space"], True),
                 changed(bpe, ["pre_tokenizer", "use_regex"], False), changed(bpe, ["normalizer"], {"type": "Prepend", "prepend": " "}),
                 changed(base, ["post_processor"], {"type": "BertProcessing", "sep": ["</s>", 2], "cls": ["<s>", 0]}),
                 changed(base, ["post_processor", "single"], [{"Sequence": {"id": "B", "type_id": 0}}]),
                 changed(base, ["model"], {"type": "WordPiece", "vocab": {"a": 0}, "unk_token": "a", "continuing_subword_prefix": "##", "max_input_chars_per_word": 100})):
        with pytest.raises(NotImplementedError):
            _spec(data)
    for kw in (dict(padding_side="left"), dict(truncation_side="left")):
        with pytest.raises(NotImplementedError):
            _spec(base, **kw)
    for data in (changed(base, ["padding", "direction"], "Left"), changed(base, ["truncation", "direction"], "Left")):
        with pytest.raises(NotImplementedError):
            _spec(data)
    with pytest.raises(ValueError):
        _spec(base, pad_id=None)
    roberta = _spec(changed(base, ["post_processor"], {"type": "RobertaProcessing", "sep": ["</s>", 2], "cls": ["<s>", 0], "trim_offsets": True, "add_prefix_space": False}))
    assert (roberta.prefix_ids, roberta.suffix_ids) == ((0,), (2,))
    assert _spec(changed(base, ["post_processor"], {"type": "ByteLevel", "add_prefix_space": True, "trim_offsets": False, "use_regex": True})).prefix_ids == ()
    spec = er.load_fixture("encode_unigram_prefix_bos_eos_t32")["spec"]
    for t in (0, 1, 2):          # block_size <= n_prefix + n_suffix
        with pytest.raises(ValueError):
            spec.check_call(["a"], t, None)
    assert spec.check_call(["a", "b"], 3, {5: 6})[1] == [(5, 6)]
    with pytest.raises(ValueError):
        spec.check_call(["a"], 8, {i: 0 for i in range(300)})
    assert "<s>" in spec.special_strings
    with pytest.raises(NotImplementedError):
        spec.check_call(["fine", "not <s> fine"], 8, None)
    assert spec.check_call(["ends <", "s> starts"], 8, None)[0] == "ends <s> starts"          # (a special's string across two texts is in neither)
