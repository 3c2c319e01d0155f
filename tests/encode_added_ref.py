"""Plain-Python restatement of text encoding with added tokens split out of the texts ("the cut step"): what
``DeviceTextEncoder(..., split_added_tokens=True)`` must give, element for element.  Built on tests/encode_ref.py.

Not product code.  ``tokens``: ``{content: id}`` of the PLAIN added tokens (``normalized=False`` or no normalizer, no ``lstrip`` /
``rstrip`` / ``single_word``).  tests/test_encode_added_host.py holds this file to the installed ``tokenizers``.
"""
from __future__ import annotations

import copy
import json
from typing import Callable, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np

from tests import encode_ref as er

Section = Union[str, int]          # a stretch of text, or the id of a match


def cut(text: str, tokens: Mapping[str, int]) -> List[Section]:
    """Leftmost-longest, non-overlapping matches on the raw bytes: from byte i, the first byte m >= i where a token matches is taken
    with the longest token that matches there; the search goes on behind the match.  Empty sections are left out."""
    raw = text.encode("utf-8")
    keys = sorted(((k.encode("utf-8"), v) for k, v in tokens.items()), key=lambda kv: -len(kv[0]))          # longest first
    out: List[Section] = []
    i = start = 0
    while i < len(raw):
        hit = next(((k, v) for k, v in keys if raw.startswith(k, i)), None)
        if hit is None:
            i += 1
            continue
        if i > start:
            out.append(raw[start:i].decode("utf-8"))
        out.append(int(hit[1]))
        i = start = i + len(hit[0])
    if len(raw) > start:
        out.append(raw[start:].decode("utf-8"))
    return out


def text_ids(text: str, tokens: Mapping[str, int], prefix_mode: int, marks_are_letters: bool, segment: Callable[[bytes], List[int]], resplit: bool = False) -> List[int]:
    """Every section is a text of its own (prefix, the pattern's view of its end), every match one id."""
    ids: List[int] = []
    for part in cut(text, tokens):
        if isinstance(part, int):
            ids.append(part)
        else:
            ids.extend(er.text_ids(part, prefix_mode, marks_are_letters, segment, resplit))
    return ids


def encode(texts: Sequence[str], block_size: int, tokens: Mapping[str, int], *, prefix_mode: int, marks_are_letters: bool, prefix_ids: Sequence[int],
           suffix_ids: Sequence[int], pad_id: int, segment: Callable[[bytes], List[int]], special_ids_map: Optional[Dict[int, int]] = None,
           resplit: bool = False) -> Tuple[np.ndarray, np.ndarray]:
    """encode_ref.encode with the cut: (input_ids, attention_mask), int64 [len(texts), block_size]."""
    t = int(block_size)
    cap = t - len(prefix_ids) - len(suffix_ids)
    if cap <= 0:
        raise ValueError("block_size leaves no room for the text")
    ids = np.full((len(texts), t), pad_id, dtype=np.int64)
    mask = np.zeros((len(texts), t), dtype=np.int64)
    for r, text in enumerate(texts):
        row = list(prefix_ids) + text_ids(text, tokens, prefix_mode, marks_are_letters, segment, resplit)[:cap] + list(suffix_ids)
        ids[r, :len(row)] = row
        mask[r, :len(row)] = 1
    for key, value in (special_ids_map or {}).items():
        ids[ids == key] = value
    return ids, mask


def encode_with(spec, segment, texts: Sequence[str], block_size: int, special_ids_map: Optional[Dict[int, int]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """``spec``: an EncodeSpec with split_added_tokens; its plain tokens are what is cut"""
    tokens = {a.content: a.id for a in spec.added_tokens if spec.is_plain(a)} if spec.split_added_tokens else {}
    return encode(texts, block_size, tokens, prefix_mode=spec.prefix_mode, marks_are_letters=spec.marks_are_letters, prefix_ids=spec.prefix_ids,
                  suffix_ids=spec.suffix_ids, pad_id=spec.pad_id, segment=segment, special_ids_map=special_ids_map, resplit=spec.resplit)


# ---- tokenizers for the tests: a fixture's tokenizer.json with another added-token list ---------------------------------------------------
def with_added_tokens(tokenizer_json: dict, tokens: Sequence[Tuple[str, int]], **flags) -> dict:
    """A copy of ``tokenizer_json`` whose ``added_tokens`` are ``tokens`` ((content, id) pairs; ``flags``: normalized / lstrip / rstrip /
    single_word / special for all of them)."""
    data = copy.deepcopy(tokenizer_json)
    data["added_tokens"] = [dict({"id": int(i), "content": c, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False, "special": True}, **flags)
                            for c, i in tokens]
    return data


def library(tokenizer_json: dict):
    """the installed library's tokenizer of ``tokenizer_json``, without padding and truncation"""
    from tokenizers import Tokenizer
    tk = Tokenizer.from_str(json.dumps(tokenizer_json))
    tk.no_padding()
    tk.no_truncation()
    return tk


ALPHABET_EXTRA = ["<", "/", ">", "x", "y"]


def random_text(rng: np.random.Generator, token_strings: Sequence[str], max_len: int = 24) -> str:
    """encode_ref.random_text's alphabet plus ``< / > x y``, with whole token strings spliced in (about one in six draws)."""
    alphabet = ["'", "s", "t", "r", "e", "v", "m", "l", "d", " ", " ", "\n", "\t", "0", "7", '"', ".", "\u00a0", "\u0301", "\u00e9", "\u4e2d", "\U0001F600"] + ALPHABET_EXTRA
    parts = []
    for _ in range(int(rng.integers(0, max_len + 1))):
        if token_strings and rng.random() < 1 / 6:
            parts.append(token_strings[int(rng.integers(0, len(token_strings)))])
        else:
            parts.append(alphabet[int(rng.integers(0, len(alphabet)))])
    return "".join(parts)
