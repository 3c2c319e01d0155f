"""Plain-Python restatement of text encoding: what ``DeviceTextEncoder`` must give, element for element.

Not product code: the tests and tests/golden/make_golden_encode.py use it.  The character classes come from the installed
``tokenizers`` (``classes_of`` probes its pre-tokenizers, character by character, and remembers), the ids of a word from a
``segment(raw_bytes) -> ids`` callable — oracle/retok_ref.py's ``tokenize`` in the tests.
"""
from __future__ import annotations

import gzip
import json
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

O, L, M, N, S = 0, 1, 2, 3, 4
PREFIX_NONE, PREFIX_ALWAYS, PREFIX_UNLESS_SPACE = 0, 1, 2
CONTRACTIONS = ("'s", "'t", "'re", "'ve", "'m", "'ll", "'d")          # in the pattern's order; no one is a prefix of another
PATTERN_MARKS = r"'s|'t|'re|'ve|'m|'ll|'d| ?[\p{L}\p{M}]+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("encode_unigram_prefix_bos_eos_t32", "encode_unigram_noprefix_bos_t8", "encode_unigram_prefix_nopost_t8_map", "encode_unigram_noprefix_bos_eos_t32_map",
            "encode_bpe_prefix_bos_eos_t32", "encode_bpe_noprefix_nopost_t8")

_CLASS: Dict[str, int] = {}
_PRE = None


def library_pre_tokenizers():
    """(the sampled tokenizers' Split with marks in the letter class, ByteLevel(use_regex=True)): the two pattern variants"""
    global _PRE
    if _PRE is None:
        import tokenizers
        from tokenizers import pre_tokenizers
        _PRE = (pre_tokenizers.Split(tokenizers.Regex(PATTERN_MARKS), "removed", invert=True), pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True))
    return _PRE


def probe_class(ch: str) -> int:
    """The class of one character, from four probes of the library: does it stay with a letter (under either variant), a digit, a
    full stop in front of it?  Whitespace is what stays with none of them."""
    marks, plain = library_pre_tokenizers()

    def one_word(pre, first):
        return len(pre.pre_tokenize_str(first + ch)) == 1
    if one_word(plain, "a"):
        return L
    if one_word(marks, "a"):
        return M
    if one_word(plain, "1"):
        return N
    if one_word(plain, "."):
        return O
    return S


def classes_of(text: str) -> List[int]:
    out = []
    for ch in text:
        c = _CLASS.get(ch)
        if c is None:
            c = _CLASS[ch] = probe_class(ch)
        out.append(c)
    return out


def apply_prefix(text: str, mode: int) -> str:
    """An empty text gets no prefix in any mode."""
    if not text or mode == PREFIX_NONE:
        return text
    if mode == PREFIX_ALWAYS or not text.startswith(" "):
        return " " + text
    return text


def match_end(text: str, cls: Sequence[int], i: int, marks_are_letters: bool) -> int:
    """The end of the pattern's match that starts at i: the alternatives in their order."""
    n = len(text)
    for c in CONTRACTIONS:          # case-sensitive, and only here: at a match start
        if text.startswith(c, i):
            return i + len(c)
    s = i
    if text[i] == " " and i + 1 < n and cls[i + 1] != S:          # ` ?` is U+0020 only
        s = i + 1
    k = cls[s]
    if k == S:
        j = s
        while j < n and cls[j] == S:
            j += 1
        if j == n or j - s == 1:          # \s+(?!\S) to the end of the text; a single character: \s+
            return j
        return j - 1                      # \s+(?!\S) gives the run's last character back
    if k == L or (k == M and marks_are_letters):
        inside = (lambda c: c == L or (c == M and marks_are_letters))
    elif k == N:
        inside = (lambda c: c == N)
    else:                                 # [^\s\p{L}\p{N}]: marks too, under both variants
        inside = (lambda c: c == O or c == M)
    j = s + 1
    while j < n and inside(cls[j]):
        j += 1
    return j


def split_words(text: str, marks_are_letters: bool, resplit: bool = False) -> List[str]:
    """resplit: every word is split again, on its own, with the plain pattern — a ByteLevel with use_regex behind the Split."""
    cls = classes_of(text)
    words, i = [], 0
    while i < len(text):
        j = match_end(text, cls, i, marks_are_letters)
        words.append(text[i:j])
        i = j
    if resplit:
        words = [w for word in words for w in split_words(word, False)]
    return words


def text_ids(text: str, prefix_mode: int, marks_are_letters: bool, segment: Callable[[bytes], List[int]], resplit: bool = False) -> List[int]:
    ids: List[int] = []
    for word in split_words(apply_prefix(text, prefix_mode), marks_are_letters, resplit):
        ids.extend(segment(word.encode("utf-8")))
    return ids


def encode(texts: Sequence[str], block_size: int, *, prefix_mode: int, marks_are_letters: bool, prefix_ids: Sequence[int], suffix_ids: Sequence[int],
           pad_id: int, segment: Callable[[bytes], List[int]], special_ids_map: Optional[Dict[int, int]] = None, resplit: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """(input_ids, attention_mask), int64 [len(texts), block_size]."""
    t = int(block_size)
    cap = t - len(prefix_ids) - len(suffix_ids)
    if cap <= 0:
        raise ValueError("block_size leaves no room for the text")
    ids = np.full((len(texts), t), pad_id, dtype=np.int64)
    mask = np.zeros((len(texts), t), dtype=np.int64)
    for r, text in enumerate(texts):
        row = list(prefix_ids) + text_ids(text, prefix_mode, marks_are_letters, segment, resplit)[:cap] + list(suffix_ids)
        ids[r, :len(row)] = row
        mask[r, :len(row)] = 1
    for key, value in (special_ids_map or {}).items():          # in order (collator.py:177-178)
        ids[ids == key] = value
    return ids, mask


def random_text(rng: np.random.Generator, max_len: int = 24) -> str:
    """The alphabet of the split tests: what the contractions, ` ?` and the whitespace rule look at, and one character of every class."""
    alphabet = ["'", "s", "t", "r", "e", "v", "m", "l", "d", " ", " ", "\n", "\t", "0", "7", '"', ".", "\u00a0", "\u0301", "\u00e9", "\u4e2d", "\U0001F600"]
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=int(rng.integers(0, max_len + 1))))


# ---- the fixtures of tests/golden/make_golden_encode.py ------------------------------------------------------------------------------
_LOADED: Dict[str, dict] = {}


def load_fixture(name: str) -> dict:
    """The fixture as written, plus "spec" (zett_amd.text_encode.EncodeSpec), "segment" (oracle/retok_ref.py on the tokenizer's model) and
    "map" (special_ids_map as a dict, in order).  Loaded once and shared: nobody changes it."""
    fx = _LOADED.get(name)
    if fx is None:
        from oracle import retok_ref
        from zett_amd.text_encode import EncodeSpec
        with gzip.open(os.path.join(GOLDEN, name + ".json.gz"), "rb") as f:
            fx = json.loads(f.read().decode("ascii"))
        spec = EncodeSpec.from_tokenizer_json(fx["tokenizer"], fx["pad_token_id"], fx["padding_side"], fx["truncation_side"])
        spec.special_strings = tuple(sorted(set(spec.special_strings) | set(fx["special_tokens"])))
        fx["spec"] = spec
        fx["segment"] = segment_of(fx["tokenizer"])
        fx["map"] = {int(k): int(v) for k, v in fx["special_ids_map"]}
        _LOADED[name] = fx
    return fx


def segment_of(tokenizer_json: dict) -> Callable[[bytes], List[int]]:
    """raw bytes of a word -> ids, by oracle/retok_ref.py's plain-Python twin of the library's models (remembered per word)"""
    from oracle import retok_ref
    model = retok_ref.model_from_tokenizer_json(tokenizer_json)
    seen: Dict[bytes, List[int]] = {}

    def segment(raw: bytes) -> List[int]:
        ids = seen.get(raw)
        if ids is None:
            ids = seen[raw] = list(retok_ref.tokenize(model, raw))
        return ids
    return segment


def encode_with(spec, segment, texts: Sequence[str], block_size: int, special_ids_map: Optional[Dict[int, int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    return encode(texts, block_size, prefix_mode=spec.prefix_mode, marks_are_letters=spec.marks_are_letters, prefix_ids=spec.prefix_ids, suffix_ids=spec.suffix_ids,
                  pad_id=spec.pad_id, segment=segment, special_ids_map=special_ids_map, resplit=spec.resplit)
