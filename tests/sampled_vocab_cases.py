"""Hand-made piece lists and stand-in reference tokenizers for tests/test_sampled_vocab_host.py and tests/test_sampled_vocab_gpu.py: the
special-token layouts at which the closed form of zett_amd/sampled_vocab.py can go wrong.  Not product code."""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np

from tests import sampler_ref as R

TABLE_PIECE = R.byte_level(b" the")          # the first piece behind the fixed ones in every hand-made list

# specials: token -> id, in the order bos, eos, pad, unk (the fourth may be missing); map: is special_ids_map non-empty; removed: pieces that are a special's string
CASES: Dict[str, dict] = {
    "ids_0123": {"specials": {"<s>": 0, "</s>": 2, "<pad>": 1, "<unk>": 3}, "map": False, "removed": 0},
    "ids_027": {"specials": {"<s>": 0, "</s>": 2, "<pad>": 7}, "map": False, "removed": 0},
    "one_beyond_the_end": {"specials": {"<s>": 0, "</s>": 2, "<pad>": 1, "<unk>": 50256}, "map": True, "removed": 0},
    "two_beyond_the_end": {"specials": {"<s>": 0, "</s>": 50000, "<pad>": 1, "<unk>": 50256}, "map": True, "removed": 0},
    "special_is_a_table_piece": {"specials": {"<s>": 0, "</s>": 2, "<pad>": 1, TABLE_PIECE: 300}, "map": False, "removed": 1},
    "special_is_an_alphabet_piece": {"specials": {"<s>": 0, "</s>": 2, "<pad>": 1, "a": 3}, "map": False, "removed": 1},
}


def stand_in_reference(specials: Dict[str, int], unk: Optional[str] = None):
    """A tokenizer that has what the host half reads of the reference: all_special_tokens / all_special_ids, the named tokens and a
    post-processor (the ``_reference_tokenizer()`` pattern of tests/test_sampler_gpu.py).  The first three entries are bos, eos and pad,
    a fourth is the unk token."""
    from tokenizers import Tokenizer, models, processors
    from transformers import PreTrainedTokenizerFast
    names = list(specials)
    bos, eos, pad = names[0], names[1], names[2]
    unk = unk if unk is not None else (names[3] if len(names) > 3 else None)
    tk = Tokenizer(models.WordLevel(dict(specials), unk_token=unk or "<unk>"))
    tk.post_processor = processors.TemplateProcessing(single=f"{bos} $A {eos}", special_tokens=[(bos, specials[bos]), (eos, specials[eos])])
    return PreTrainedTokenizerFast(tokenizer_object=tk, bos_token=bos, eos_token=eos, unk_token=unk, pad_token=pad, clean_up_tokenization_spaces=False)


def table_pieces(extra: int, seed: int = 7) -> List[bytes]:
    """``extra`` distinct keys a sampler's table could hold (2 .. 15 bytes, fewer than two whitespace bytes), " the" first."""
    rng = np.random.default_rng(seed)
    alphabet = list(b"abcdefghijklmnopqrstuvwxyzABC0123456789.,'-") + [0x20, 0xC3, 0xA9, 0xE4, 0xB8, 0xAD, 0xF0, 0x9F, 0x98, 0x80, 0x00, 0x7F, 0xAD]
    out, seen = [b" the"], {b" the"}
    while len(out) < extra:
        raw = bytes(alphabet[i] for i in rng.integers(0, len(alphabet), size=int(rng.integers(2, 16))))
        if raw in seen or R.is_fixed(raw):
            continue
        seen.add(raw)
        out.append(raw)
    return out[:extra]


def hand_made(extra: int) -> List[Tuple[str, float]]:
    """391 fixed pieces and ``extra`` of the table, with distinct scores behind the fixed ones: the shape of a sampler's list."""
    fixed = [(R.byte_level(bytes([b])), -12.25) for b in range(256)] + [(R.byte_level(run), 0.0) for run in R.whitespace_runs(16)]
    return fixed + [(R.byte_level(raw), -1.0 - 0.37 * i) for i, raw in enumerate(table_pieces(extra))]


def case_pieces(name: str, extra: int) -> List[Tuple[str, float]]:
    assert name in CASES
    return hand_made(extra)


def texts_for(extra: int, n: int = 40, seed: int = 5) -> List[str]:
    """Texts that use the table's pieces, contractions, digits, other scripts and whitespace runs."""
    rng = np.random.default_rng(seed)
    words = [raw.decode("utf-8", "ignore").strip() for raw in table_pieces(extra)[:200]]
    words = [w for w in words if w and "\x00" not in w] + ["the", "it's", "12", "we'll", "é", "中", "\U0001F600", ".", ",", "  ", "\n"]
    return [" ".join(words[i] for i in rng.integers(0, len(words), size=int(rng.integers(0, 24)))) for _ in range(n)]
