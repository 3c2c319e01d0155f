"""Plain-Python restatement of ``rust_utils.TokenizerSampler``: what ``DeviceTokenizerSampler`` must give.

Written from reading rust_utils/src/lib.rs:70-249; the Rust code itself was never run (no Rust toolchain where this project is built), so
this file is the yardstick.  Not product code: the tests and tools/sample_tokenizer_bench.py use it.  The pre-tokenizer is the installed
``tokenizers``' own — the Sequence the Rust code builds — read with ``pre_tokenize_str``, whose offsets are original character offsets.

Keys are raw ``bytes`` here (a byte-level character is one raw byte); ``byte_level`` turns them into the strings the Rust class returns.
Where the Rust code's order is an accident of HashMap iteration the order is fixed: the 256 alphabet pieces in byte order, the table by
(higher noised value, shorter key, smaller bytes); every noised value <= 0 is one tie class (it emits -100000.0).
"""
from __future__ import annotations

import gzip
import json
import math
import os
from collections import deque
from typing import Callable, Deque, Dict, Iterable, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

SPLIT_PATTERN = r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"
WHITESPACE_BYTES = (0x20, 0x0A, 0x09)          # Ġ Ċ ĉ
N_ALPHABET = 256
FLOOR = -100000.0


def _bytes_to_chars() -> List[str]:
    """The byte-level alphabet (GPT-2's bytes_to_unicode): printable bytes stand for themselves, the others for U+0100 + n."""
    keep = list(range(33, 127)) + list(range(161, 173)) + list(range(174, 256))
    chars, n = {}, 0
    for b in range(256):
        if b in keep:
            chars[b] = chr(b)
        else:
            chars[b] = chr(256 + n)
            n += 1
    return [chars[b] for b in range(256)]


BYTES_TO_CHARS = _bytes_to_chars()
CHARS_TO_BYTES = {c: b for b, c in enumerate(BYTES_TO_CHARS)}


def byte_level(raw: bytes) -> str:
    return "".join(BYTES_TO_CHARS[b] for b in raw)


def from_byte_level(piece: str) -> bytes:
    return bytes(CHARS_TO_BYTES[c] for c in piece)


_PRE = None


def pre_tokenizer():
    global _PRE
    if _PRE is None:
        import tokenizers
        from tokenizers import pre_tokenizers
        _PRE = pre_tokenizers.Sequence([pre_tokenizers.Split(tokenizers.Regex(SPLIT_PATTERN), "removed", invert=True),
                                        pre_tokenizers.ByteLevel(add_prefix_space=False, trim_offsets=True, use_regex=False)])
    return _PRE


def pre_tokens(sentence: str) -> List[Tuple[bytes, Tuple[int, int]]]:
    """(raw bytes of the pre-token, its original character range) for a sentence that already has its prefix space."""
    return [(from_byte_level(piece), (int(o0), int(o1))) for piece, (o0, o1) in pre_tokenizer().pre_tokenize_str(sentence)]


def score_of(raw: bytes) -> int:
    """UTF-8 length of the key's byte-level string"""
    return sum(1 if 33 <= b <= 126 else 2 for b in raw)


def starts_of(sentence: str, index: int, o0: int, o1: int, stride: int) -> List[int]:
    """Every stride-th entry of the start list of pre-token `index` = sentence[o0:o1]: cum[c] - cum[o0] over the inclusive scan of the
    UTF-8 lengths, one more 0 in front for the first pre-token."""
    cum = np.cumsum([len(ch.encode("utf-8")) for ch in sentence]).tolist()
    return _starts(cum, index, o0, o1, stride)


def _starts(cum: List[int], index: int, o0: int, o1: int, stride: int) -> List[int]:
    entries = [cum[c] - cum[o0] for c in range(o0, o1)]
    if index == 0:
        entries.insert(0, 0)
    return entries[::stride]


def count_substrings(texts: Iterable[str], max_length: int = 16, stride: int = 1) -> Dict[bytes, int]:
    """The table of one call: texts are dictionary keys (a duplicate counts once), each with count 1."""
    table: Dict[bytes, int] = {}
    for text in dict.fromkeys(texts):
        sentence = " " + text
        cum = np.cumsum([len(ch.encode("utf-8")) for ch in sentence]).tolist()
        for index, (raw, (o0, o1)) in enumerate(pre_tokens(sentence)):
            for start in _starts(cum, index, o0, o1, stride):
                for k in range(1, max_length):
                    if start + k > len(raw):
                        break
                    token = raw[start:start + k]
                    table[token] = table.get(token, 0) + score_of(token)
    return table


def whitespace_runs(max_length: int) -> List[bytes]:
    out = []
    for c1 in WHITESPACE_BYTES:
        for i in range(1, max_length):
            for c2 in WHITESPACE_BYTES:
                out.append(bytes([c2]) + bytes([c1]) * i)
    return out


def is_fixed(raw: bytes) -> bool:
    """a key the fixed pieces already cover: one character, or two and more of the three whitespace characters"""
    return len(raw) == 1 or sum(b in WHITESPACE_BYTES for b in raw) >= 2


class SamplerRef:
    """``rust_utils.TokenizerSampler`` with raw-byte keys.  ``noise``: key -> z (standard normal); the noised value is
    v / sum + noise_std * z in float64."""

    def __init__(self):
        self.queue: Deque[Dict[bytes, int]] = deque()
        self.merged: Dict[bytes, int] = {}

    def sample(self, texts: Union[Sequence[str], Mapping[str, int]], seed_size: int, max_length: int = 16, stride: int = 1, noise_std: float = 0.0,
               pop_prev: bool = True, push_current: bool = True, noise: Optional[Callable[[bytes], float]] = None) -> List[Tuple[bytes, float]]:
        current = count_substrings(texts, max_length, stride)
        prev = self.queue.pop() if (pop_prev and self.queue) else None
        self.queue.appendleft(current)
        out: List[Tuple[bytes, float]] = []
        if pop_prev:
            merged: Dict[bytes, int] = {}
            for table in self.queue:
                for key, v in table.items():
                    merged[key] = merged.get(key, 0) + v
            self.merged = merged
            total = float(sum(merged.values()))
            low = float(min(merged.values()))
            min_log = math.log(low / total)
            out = [(bytes([b]), min_log) for b in range(N_ALPHABET)]
            out += [(run, 0.0) for run in whitespace_runs(max_length)]
            noised = []
            for key, v in merged.items():
                p = v / total
                if noise_std != 0.0:
                    p = p + noise_std * float(noise(key))
                noised.append((key, p if p > 0.0 else 0.0))
            noised.sort(key=lambda kp: (-kp[1], len(kp[0]), kp[0]))
            for key, p in noised:
                if is_fixed(key):
                    continue
                out.append((key, math.log(p) if p > 0.0 else FLOOR))
                if len(out) >= seed_size:
                    break
        if not push_current:
            self.queue.popleft()
            if prev is not None:
                self.queue.append(prev)
        return out

    def sample_tokenizer(self, texts, seed_size, max_length=16, stride=1, noise_std=0.0, pop_prev=True, push_current=True, noise=None) -> List[Tuple[str, float]]:
        """The Rust class's return value: (byte-level string, score)."""
        return [(byte_level(k), s) for k, s in self.sample(texts, seed_size, max_length, stride, noise_std, pop_prev, push_current, noise)]


def random_text(rng: np.random.Generator, max_len: int = 48) -> str:
    """Mixed scripts, contractions, whitespace runs."""
    alphabet = ["'", "s", "t", "re", "ve", "m", "ll", "d", " ", " ", "  ", "\n", "\t", "0", "7", '"', ".", ",", " ", "́", "é", "中", "日",
                "\U0001F600", "a", "b", "the", "ing", "Ж", "א", "x", "I", "'"]
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=int(rng.integers(0, max_len + 1))))


def random_prose(rng: np.random.Generator, n_words: int = 60) -> str:
    """Words of random letters (many distinct substrings), some of them in other scripts, between the separators of ``random_text``."""
    letters = list("abcdefghijklmnopqrstuvwxyzABCDEFGH0123456789") + ["é", "ü", "Ж", "д", "中", "日", "א", "\U0001F600", "́"]
    seps = [" ", " ", " ", " ", ", ", ". ", "  ", "\n", " \t", "'s ", "'ll ", "\n\n ", " - "]
    out = []
    for _ in range(n_words):
        out.append("".join(letters[i] for i in rng.integers(0, len(letters), size=int(rng.integers(1, 11)))))
        out.append(seps[int(rng.integers(0, len(seps)))])
    return "".join(out)


# ---- the fixtures of tests/golden/make_golden_sample_tokenizer.py ---------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("sample_tokenizer_prefix", "sample_tokenizer_noprefix")


def load_fixture(name: str) -> dict:
    with gzip.open(os.path.join(GOLDEN, name + ".json.gz"), "rb") as f:
        return json.loads(f.read().decode("ascii"))


def tokenizer_of(entry: dict):
    """The transformers tokenizer of a fixture's "reference" or "hn_tokenizer" entry."""
    from tokenizers import Tokenizer
    from transformers import PreTrainedTokenizerFast
    tk = Tokenizer.from_str(json.dumps(entry["tokenizer"]))
    return PreTrainedTokenizerFast(tokenizer_object=tk, bos_token=entry["bos_token"], eos_token=entry["eos_token"], unk_token=entry["unk_token"],
                                   pad_token=entry["pad_token"], clean_up_tokenization_spaces=False)


class StandInSampler:
    """What the host half asks of a sampler: it returns a prepared list and remembers how it was called."""

    def __init__(self, pieces):
        self.pieces, self.calls = [tuple(p) for p in pieces], []

    def sample_tokenizer(self, *args):
        self.calls.append(args)
        return list(self.pieces)
