"""The definition half of zett_amd/sampled_vocab.py (no GPU): the closed form of the reference's list surgery (zett/collator.py:371-400)
against ``build_sampled_tokenizer``, which tests/test_sampler_host.py holds to the reference's own outputs."""
import os
import re

import numpy as np
import pytest

from tests import sampler_ref as R
from tests.sampled_vocab_cases import CASES, case_pieces, stand_in_reference
from zett_amd import sampled_vocab as sv
from zett_amd.surface_forms import BYTES_TO_CHARS_LIST
from zett_amd.tokenizer_sampling import build_sampled_tokenizer

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(pieces_and_scores, reference):
    tokenizer, special_ids_map, scores = build_sampled_tokenizer(pieces_and_scores, reference, True)
    tokens = tokenizer.convert_ids_to_tokens(range(len(tokenizer)))
    got = sv.layout_reference(pieces_and_scores, list(reference.all_special_tokens), list(reference.all_special_ids))
    assert got.pieces == tokens
    assert got.scores.dtype == np.float64 and got.scores.tobytes() == np.asarray(scores, dtype=np.float64).tobytes()
    assert got.byte_lengths.tolist() == [len(t) for t in tokens]
    assert list(got.special_ids_map.items()) == list(special_ids_map.items())
    m = len(tokens) - len(reference.all_special_ids)
    positions, again = sv.sampled_vocabulary_layout(m, list(reference.all_special_ids))
    assert list(again.items()) == list(special_ids_map.items())
    order = np.argsort(reference.all_special_ids)
    assert [tokens[p] for p in positions] == [reference.all_special_tokens[i] for i in order]
    assert got.n_removed == len(sv.prepend_unknown_chars(pieces_and_scores)) - m
    return got


@pytest.mark.parametrize("name", R.FIXTURES)
def test_fixtures_of_the_reference(name):
    fx = R.load_fixture(name)
    got = _check([(p, s) for p, s in fx["prepared"]], R.tokenizer_of(fx["reference"]))
    assert got.pieces == fx["pieces"] and got.scores.tolist() == fx["scores"] and got.byte_lengths.tolist() == fx["byte_lengths"]
    assert [[k, v] for k, v in got.special_ids_map.items()] == fx["special_ids_map"]
    assert got.n_removed == 1


@pytest.mark.parametrize("extra", (1, 9, 600))
@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made_lists(name, extra):
    got = _check(case_pieces(name, extra), stand_in_reference(CASES[name]["specials"]))
    want = CASES[name]
    assert bool(got.special_ids_map) == want["map"], got.special_ids_map
    assert got.n_removed == want["removed"]


def test_byte_level_code_points():
    cps = sv.byte_level_code_points()
    assert cps.shape == (256,) and [chr(c) for c in cps] == BYTES_TO_CHARS_LIST == R.BYTES_TO_CHARS
    assert len(set(cps.tolist())) == 256 and cps.max() == 323


def test_json_round_trip_is_the_library_s():
    """``json_round_trip`` against ``Tokenizer.from_str(tokenizer.to_str())`` on logarithms, small and large values and exact ones; and
    the probe of the installed library finds what ``build_sampled_tokenizer``'s tokenizer really holds."""
    import json

    from tokenizers import Tokenizer, models
    rng = np.random.default_rng(1)
    xs = np.concatenate([np.log(rng.random(4000)), -rng.random(500) * 1e-3, -rng.random(500) * 20, -1.0 - 0.37 * np.arange(600),
                         [-100000.0, 0.0, -0.5, -2.0 ** -10, -1e-5, 0.1, 1 / 3]]).tolist()
    tk = Tokenizer(models.Unigram([("p%d" % i, x) for i, x in enumerate(xs)]))
    back = [float(s) for _, s in json.loads(Tokenizer.from_str(tk.to_str()).to_str())["model"]["vocab"]]
    mine = [sv.json_round_trip(x) for x in xs]
    assert [np.float64(m).tobytes() for m in mine] == [np.float64(b).tobytes() for b in back]
    assert 100 < sum(b != x for b, x in zip(back, xs)) < 1500          # about one in nine
    assert sv.json_round_trip(float("inf")) == float("inf") and sv.json_round_trip(-100000.0) == -100000.0
    reference = stand_in_reference(CASES["special_is_an_alphabet_piece"]["specials"])
    pieces = case_pieces("special_is_an_alphabet_piece", 600)
    tokenizer, _, scores = build_sampled_tokenizer(pieces, reference, True)
    held = [float(s) for _, s in json.loads(tokenizer._tokenizer.to_str())["model"]["vocab"]]
    through = sv.DeviceSampledVocabulary._probe_scores(build_sampled_tokenizer(sv.fixed_pieces(), reference, True)[0], reference.all_special_tokens)
    assert held == [sv.json_round_trip(x) if through else x for x in scores.tolist()]


def test_fixed_pieces_are_the_sampler_s():
    want = [R.byte_level(bytes([b])) for b in range(256)] + [R.byte_level(run) for run in R.whitespace_runs(16)]
    assert [p for p, _ in sv.fixed_pieces()] == want and len(want) == 391


def test_refusals():
    with pytest.raises(ValueError, match="duplicate special ids"):
        sv.sampled_vocabulary_layout(400, [0, 1, 1])
    with pytest.raises(ValueError, match="duplicate special tokens"):
        sv.layout_reference(sv.fixed_pieces(), ["<s>", "<s>"], [0, 1])
    with pytest.raises(ValueError, match="negative"):
        sv.sampled_vocabulary_layout(400, [0, -1])
    with pytest.raises(ValueError, match="at most 256"):
        sv.sampled_vocabulary_layout(400, list(range(257)))
    with pytest.raises(ValueError):
        sv.sampled_vocabulary_layout(-1, [0])
    with pytest.raises(ValueError):
        sv.sorted_specials(["a"], [0, 1])
    assert sv.prepend_unknown_chars(sv.fixed_pieces()) == sv.fixed_pieces()
    assert sv.prepend_unknown_chars([("b", -1.0), ("c", -3.0)])[:2] == [("!", -3.0), ('"', -3.0)] and len(sv.prepend_unknown_chars([("b", -1.0)])) == 256
    for bits, error in ((sv.VOCAB_NOT_A_SAMPLE, NotImplementedError), (sv.VOCAB_DUPLICATE, ValueError), (sv.VOCAB_TABLE_FULL, RuntimeError), (sv.VOCAB_OUT_FULL, RuntimeError)):
        with pytest.raises(error):
            sv.raise_for_vocab_status(bits)
    sv.raise_for_vocab_status(0)


def test_refusals_of_the_device_class_that_need_no_device(monkeypatch):
    """More than max_vocab entries, a special token too long for the table, one outside the byte table that the hn tokenizer does not
    know: refused before anything touches a GPU."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    reference = stand_in_reference({"<s>": 0, "<pad>": 1, "</s>": 2, "<unk>": 3})
    with pytest.raises(RuntimeError, match="no CPU path"):
        sv.DeviceSampledVocabulary(reference, True)
    with pytest.raises(ValueError, match="hn_surface_maxlen"):
        sv.DeviceSampledVocabulary(reference, True, hn_tokenizer=reference)
    with pytest.raises(NotImplementedError, match="raw bytes"):
        sv.DeviceSampledVocabulary(stand_in_reference({"<s>": 0, "<pad>": 1, "</s>": 2, "<" + "x" * 70 + ">": 3}, unk="<" + "x" * 70 + ">"), True)
    hn = stand_in_reference({"<s>": 0, "<pad>": 1, "</s>": 2, "<unk>": 3})
    with pytest.raises(KeyError):
        sv.DeviceSampledVocabulary(stand_in_reference({"<s>": 0, "<pad>": 1, "</s>": 2, "<u k>": 3}, unk="<u k>"), True, hn_tokenizer=hn, hn_surface_maxlen=4)
    # seed_size + S > max_vocab is refused by build() before any launch: the same comparison, on the numbers alone
    vocabulary = sv.DeviceSampledVocabulary.__new__(sv.DeviceSampledVocabulary)
    vocabulary.special_ids, vocabulary.max_vocab, vocabulary.retok = [0, 1, 2, 3], 500, None

    class Pieces:
        shape = (497, 16)
    with pytest.raises(ValueError, match="max_vocab"):
        vocabulary.build(sv.SampledPieces(Pieces(), None, None, None, None), 497)


def test_abi_is_additive():
    from zett_amd import _lib, build
    header = open(os.path.join(REPO, "include", "zett_hip.h")).read()
    assert "#define ZETT_ABI_VERSION 8 " in header and _lib.ABI_VERSION == 8
    names = ("zett_retok_create_unigram_device", "zett_sampled_vocab_workspace_bytes", "zett_sampled_vocab_build", "zett_sampled_vocab_commit", "zett_sampled_vocab_table",
             "zett_sampled_vocab_patch_rows")
    lib = _lib.load()
    for name in names:
        assert re.search(r"\bint " + name + r"\(", header) and name in _lib.ABI_SYMBOLS and hasattr(lib, name)
    import ctypes
    assert ctypes.sizeof(_lib.ZettSampledVocabRecord) == 32 and _lib.ZettSampledVocabRecord.min_score.offset == 16
    assert re.search(r"ZETT_VOCAB_SCORES_THROUGH_JSON = 1\b", header) and _lib.VOCAB_SCORES_THROUGH_JSON == 1
    assert _lib.ZettSampledVocabRecord.table_min_score.offset == 24
    for name, bit in (("NOT_A_SAMPLE", 1), ("DUPLICATE", 2), ("TABLE_FULL", 4), ("OUT_FULL", 8)):
        assert re.search(r"ZETT_VOCAB_%s = %d\b" % (name, bit), header) and getattr(_lib, "VOCAB_" + name) == bit
    assert "sampled_vocab.hip" in build.SOURCES and "sampled_vocab.hip" not in build.TRAINING_ONLY
    assert not {os.path.basename(p) for p in build._includes(os.path.join(build.CSRC, "sampled_vocab.hip"))} & set(build.TRAINING_ONLY)


def test_arguments_are_refused_before_any_launch():
    """Null handles and arguments, sizes out of range: ZETT_E_INVALID without touching a device (nothing is launched)."""
    import ctypes as C

    from zett_amd import _lib
    lib = _lib.load()
    need, h = C.c_int64(0), C.c_void_p()
    assert lib.zett_sampled_vocab_workspace_bytes(0, 4, C.byref(need)) == _lib.E_INVALID
    assert lib.zett_sampled_vocab_workspace_bytes(1 << 16, 257, C.byref(need)) == _lib.E_INVALID
    assert lib.zett_sampled_vocab_workspace_bytes(1 << 16, 4, None) == _lib.E_INVALID
    assert lib.zett_sampled_vocab_workspace_bytes(1 << 16, 4, C.byref(need)) == 0 and need.value > (1 << 16) * 9
    assert lib.zett_retok_create_unigram_device(0, 0, C.byref(h)) == _lib.E_INVALID and not h.value
    assert lib.zett_retok_create_unigram_device(0, 1 << 16, None) == _lib.E_INVALID
    assert lib.zett_sampled_vocab_commit(None, None) == _lib.E_INVALID
    assert lib.zett_sampled_vocab_table(None, None, None, None, None, None, 0, None, None) == _lib.E_INVALID
    assert lib.zett_sampled_vocab_build(None, None, None, None, None, 1, 1, None, None, None, None, None, 0, 0, 0, None, None, None, 0, None, 0, None, 0, None, 0, None) == _lib.E_INVALID
    assert lib.zett_sampled_vocab_patch_rows(None, None, None, None, 0, None, 0, 1, 0, None) == _lib.E_INVALID
