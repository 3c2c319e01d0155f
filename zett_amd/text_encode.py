"""A batch of texts to padded ``input_ids`` on the device — the tokenizer call of the reference's ``Collator.encode``
(zett/collator.py:166-178) without the ``tokenizers`` library on the step's path.

    enc = DeviceTextEncoder.from_tokenizer(tokenizer)                 # once per tokenizer: tables to the device
    batch = enc(texts, block_size=128, special_ids_map={3: 1})        # {"input_ids", "attention_mask"}: [B, block_size] device tensors

What the kernels do (csrc/text_encode.hip): the optional prefix space, the split of every text into words with
the GPT-2 style pattern (zett/utils.py:29) as a state machine over five character classes, the retokenizer's stage 2 (BPE merge / Unigram
Viterbi) on every word's raw bytes, and the packing into rows: template ids, truncation from the right, padding, attention mask, the
``special_ids_map`` substitution.  Per call the host joins and encodes the texts once, takes their byte lengths and looks for the
strings of added tokens; nothing is done per word.

The character classes are DATA and come from the installed ``tokenizers``: its regex engine knows a newer Unicode than Python's
``unicodedata`` (code points unassigned in one are letters in the other), so the table is built by probing the library's own
pre-tokenizers, once per process (``class_table()``).

Everything the kernels do not reproduce is refused here, on the host, with NotImplementedError / ValueError: another normalizer,
pre-tokenizer, post-processor, padding or truncation side; WordPiece models; ``block_size <= n_prefix + n_suffix``; a text that holds the
string of an added or special token (the library would split it out).  There is no CPU path.

``split_added_tokens=True`` (``from_tokenizer``, ``from_tokenizer_json``, ``from_handle``) lifts the last refusal the way the library
does: the BACKEND's added tokens (``tokenizer._tokenizer``'s ``added_tokens``, not ``all_special_tokens``) are cut out of every text on
the device at leftmost-longest matches, each match gives the token's one id and every section between two matches is encoded as a
text of its own.  Tokens the kernels do not carry (``lstrip`` / ``rstrip`` / ``single_word``, one byte, ``normalized`` under
``Prepend``) keep the refusal, and only for a text that holds them.  The host's work per call does not grow with the table.
"""
from __future__ import annotations

import ctypes as C
import json
import dataclasses
from dataclasses import dataclass
from typing import Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._glue import default_device, ptr, stream

# the split pattern of the sampled tokenizers (zett/utils.py:29) and, without \p{M} in the letter class, of pre_tokenizers.ByteLevel(use_regex=True)
SPLIT_PATTERN_MARKS = r"'s|'t|'re|'ve|'m|'ll|'d| ?[\p{L}\p{M}]+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"
SPLIT_PATTERN_PLAIN = r"'s|'t|'re|'ve|'m|'ll|'d| ?\p{L}+| ?\p{N}+| ?[^\s\p{L}\p{N}]+|\s+(?!\S)|\s+"

CLASS_O, CLASS_L, CLASS_M, CLASS_N, CLASS_S = 0, 1, 2, 3, 4
N_CODE_POINTS = 0x110000
PREFIX_NONE, PREFIX_ALWAYS, PREFIX_UNLESS_SPACE = _lib.ENCODE_PREFIX_NONE, _lib.ENCODE_PREFIX_ALWAYS, _lib.ENCODE_PREFIX_UNLESS_SPACE
ENCODE_NO_UNK, ENCODE_BAD_OFFSETS, ENCODE_BAD_TABLE = _lib.ENCODE_NO_UNK, _lib.ENCODE_BAD_OFFSETS, _lib.ENCODE_BAD_TABLE
MAX_ADDED_TOKENS, MAX_ADDED_TOKEN_BYTES = _lib.ENCODE_MAX_ADDED, _lib.ENCODE_MAX_ADDED_BYTES
MAX_BLOCK_SIZE = 8192
_CHUNK = 256          # probes per call of a pre-tokenizer: its cost grows faster than the text


# ---- the class table ----------------------------------------------------------------------------------------------------------
def _pre_tokenizers():
    import tokenizers
    from tokenizers import pre_tokenizers
    marks = pre_tokenizers.Split(tokenizers.Regex(SPLIT_PATTERN_MARKS), "removed", invert=True)
    plain = pre_tokenizers.ByteLevel(add_prefix_space=False, use_regex=True)
    return marks, plain


def _joined(pre, first: str, code_points: np.ndarray) -> np.ndarray:
    """For every code point c: does the pre-tokenizer keep ``first + chr(c)`` in one word?  One call for the whole array: the probes
    stand on lines of their own (a line feed is whitespace to the pattern and joins nothing)."""
    text = "".join(first + chr(c) + "\n" for c in code_points.tolist())
    starts = np.fromiter((s for _, (s, e) in pre.pre_tokenize_str(text) if e - s == 2), dtype=np.int64)
    hit = np.zeros(len(code_points), dtype=bool)
    starts = starts[starts % 3 == 0]
    hit[starts // 3] = True
    return hit


def classify_code_points(code_points: Sequence[int]) -> np.ndarray:
    """The class (CLASS_*) of each code point, from four probes of the library's pre-tokenizers: behind a letter under both patterns,
    behind a digit, behind a full stop.  The four character sets of the pattern — whitespace, letters, digits, everything else —
    partition the code space, and marks are what joins a letter only when the pattern says so.  Surrogates cannot stand in a str:
    class O."""
    cps = np.asarray(code_points, dtype=np.int64)
    out = np.zeros(len(cps), dtype=np.uint8)
    ok = (cps < 0xD800) | (cps > 0xDFFF)
    marks, plain = _pre_tokenizers()
    for a in range(0, len(cps), _CHUNK):
        idx = np.flatnonzero(ok[a:a + _CHUNK]) + a
        if not len(idx):
            continue
        c = cps[idx]
        letter = _joined(plain, "a", c)
        mark = _joined(marks, "a", c) & ~letter
        digit = _joined(plain, "1", c)
        other = _joined(plain, ".", c)
        cls = np.full(len(c), CLASS_S, dtype=np.uint8)
        cls[other] = CLASS_O
        cls[digit] = CLASS_N
        cls[mark] = CLASS_M
        cls[letter] = CLASS_L
        out[idx] = cls
    return out


_CLASS_TABLE: Optional[np.ndarray] = None


def class_table() -> np.ndarray:
    """uint8 [0x110000]: the class of every code point as the installed ``tokenizers`` sees it, built once per process (a few
    seconds).  One sweep of the whole code space with the library's regex engine (the engine of both pre-tokenizers) finds the
    code points that are whitespace, letter, mark or digit to it; ``classify_code_points`` — the pre-tokenizers themselves —
    classifies those, and a seeded sample of the others, which must come out as class O."""
    global _CLASS_TABLE
    if _CLASS_TABLE is not None:
        return _CLASS_TABLE
    import tokenizers
    from tokenizers import pre_tokenizers
    cps = np.concatenate([np.arange(0, 0xD800), np.arange(0xE000, N_CODE_POINTS)])
    sweep = pre_tokenizers.Split(tokenizers.Regex(r"[\s\p{L}\p{M}\p{N}]+"), "removed", invert=True)
    found = np.zeros(N_CODE_POINTS, dtype=bool)
    for _, (lo, hi) in sweep.pre_tokenize_str("".join(map(chr, cps.tolist()))):
        found[cps[lo:hi]] = True
    found[:0x80] = True
    rest = cps[~found[cps]]
    todo = np.concatenate([np.flatnonzero(found), np.random.default_rng(0).choice(rest, size=1024, replace=False)])
    table = np.zeros(N_CODE_POINTS, dtype=np.uint8)
    table[todo] = classify_code_points(todo)
    if table[todo[-1024:]].any():
        raise RuntimeError("the pre-tokenizers give a class to a code point the regex engine's classes do not hold")
    table.setflags(write=False)
    _CLASS_TABLE = table
    return table


def pack_class_table(table: np.ndarray) -> np.ndarray:
    """4 bits per code point, code point c in bits 4 * (c & 1) .. of byte c >> 1: what zett_encode_texts takes."""
    t = np.asarray(table, dtype=np.uint8)
    if len(t) % 2:
        t = np.concatenate([t, np.zeros(1, dtype=np.uint8)])
    return (t[0::2] | (t[1::2] << 4)).astype(np.uint8)


_DEVICE_CLASS_TABLES: Dict[object, object] = {}


def device_class_table(device):
    """``pack_class_table(class_table())`` on ``device``, uploaded once per device: the encoder, the sampler and the sampled vocabulary
    share it (a caller's own ``table`` gets its own upload)."""
    import torch
    device = torch.device(device)
    if device.index is None:
        device = torch.device(device.type, torch.cuda.current_device())
    if device not in _DEVICE_CLASS_TABLES:
        _DEVICE_CLASS_TABLES[device] = torch.from_numpy(pack_class_table(class_table())).to(device)
    return _DEVICE_CLASS_TABLES[device]


def packed_table_on(device, table: Optional[np.ndarray], d_table=None):
    """(class table, its packed copy on ``device``): the shared default pair for ``table=None``; ``d_table``: the packed copy, where
    the caller keeps one"""
    import torch
    if table is None and d_table is None:
        return class_table(), device_class_table(device)
    table = class_table() if table is None else np.asarray(table, dtype=np.uint8)
    return table, torch.from_numpy(pack_class_table(table)).to(device) if d_table is None else d_table


def flatten_texts(texts: Sequence[str], joined: Optional[str] = None) -> Tuple[bytes, np.ndarray]:
    """``(blob, offsets)``: the UTF-8 bytes of the texts end to end and int64 ``[len(texts) + 1]`` byte offsets, text ``i`` at
    ``blob[offsets[i]:offsets[i + 1]]`` — what zett_encode_texts and zett_sampler_sample take.  One join and one encode; the byte
    offsets are the character offsets for ASCII and come from the character starts of the blob otherwise.  ``joined``: ``"".join(texts)``
    where the caller has it already."""
    b = len(texts)
    if joined is None:
        joined = "".join(texts)
    blob = joined.encode("utf-8")
    chars = np.zeros(b + 1, dtype=np.int64)          # character offsets of the texts
    np.cumsum(np.fromiter(map(len, texts), dtype=np.int64, count=b), out=chars[1:])
    if len(blob) == len(joined):
        return blob, chars
    raw = np.frombuffer(blob, dtype=np.uint8)
    return blob, np.append(np.flatnonzero((raw & 0xC0) != 0x80), len(raw))[chars]


# ---- what the kernels need to know about a tokenizer -------------------------------------------------------------------------------
class AddedToken(NamedTuple):
    """An entry of the backend's ``added_tokens`` list, as ``tokenizer._tokenizer.to_str()`` serialises it."""
    content: str
    id: int
    normalized: bool = False
    lstrip: bool = False
    rstrip: bool = False
    single_word: bool = False


@dataclass
class EncodeSpec:
    """Normalizer, pre-tokenizer, post-processor and padding of a tokenizer, as the arguments of zett_encode_texts."""
    prefix_mode: int
    marks_are_letters: bool
    resplit: bool                             # every word is split again with the plain pattern (the Sequence's ByteLevel has use_regex)
    prefix_ids: Tuple[int, ...]
    suffix_ids: Tuple[int, ...]
    pad_id: int
    special_strings: Tuple[str, ...]          # contents of the added tokens: a text that holds one is refused
    added_tokens: Tuple[AddedToken, ...] = ()   # the backend's added tokens; looked at with split_added_tokens alone
    split_added_tokens: bool = False          # the plain added tokens are split out on the device, and special_strings refuses nothing

    @staticmethod
    def _template(post: Optional[dict]) -> Tuple[Tuple[int, ...], Tuple[int, ...]]:
        if post is None or post.get("type") == "ByteLevel":
            return (), ()
        if post.get("type") == "RobertaProcessing":
            return (int(post["cls"][1]),), (int(post["sep"][1]),)
        if post.get("type") == "TemplateProcessing":
            prefix: List[int] = []
            suffix: List[int] = []
            seen = False
            for item in post["single"]:
                if "Sequence" in item:
                    if seen or item["Sequence"]["id"] != "A":
                        raise NotImplementedError("a TemplateProcessing whose single template is not specials, $A, specials")
                    seen = True
                elif "SpecialToken" in item:
                    ids = post["special_tokens"][item["SpecialToken"]["id"]]["ids"]
                    (suffix if seen else prefix).extend(int(i) for i in ids)
                else:
                    raise NotImplementedError(f"template item {item!r}")
            if not seen:
                raise NotImplementedError("a TemplateProcessing without $A")
            return tuple(prefix), tuple(suffix)
        raise NotImplementedError(f"post-processor {post.get('type')!r} (TemplateProcessing, RobertaProcessing, ByteLevel or none)")

    @classmethod
    def from_tokenizer_json(cls, data: Mapping, pad_id: Optional[int], padding_side: str = "right", truncation_side: str = "right",
                            split_added_tokens: bool = False) -> "EncodeSpec":
        if padding_side != "right" or truncation_side != "right":
            raise NotImplementedError(f"padding_side = {padding_side!r}, truncation_side = {truncation_side!r}: rows are cut and padded on the right")
        for key in ("padding", "truncation"):          # what an earlier call left switched on in the backend
            if (data.get(key) or {}).get("direction", "Right") != "Right":
                raise NotImplementedError(f"{key} direction {data[key]['direction']!r}: rows are cut and padded on the right")
        if pad_id is None:
            raise ValueError("the tokenizer has no pad token: padding=\"max_length\" needs one")
        model = data.get("model") or {}
        kind = model.get("type") or ("BPE" if "merges" in model else None)
        if kind not in ("BPE", "Unigram"):
            raise NotImplementedError(f"text encoding with a {kind!r} model (BPE and Unigram; WordPiece targets need another pre-tokenizer)")
        norm, pre = data.get("normalizer"), data.get("pre_tokenizer")
        prefix_mode = PREFIX_NONE
        if norm is not None:
            if norm.get("type") != "Prepend" or norm.get("prepend") != " ":
                raise NotImplementedError(f"normalizer {norm!r} (none or Prepend(\" \"))")
            prefix_mode = PREFIX_ALWAYS
        if pre is None:
            raise NotImplementedError("a tokenizer without a pre-tokenizer")
        if pre.get("type") == "ByteLevel":
            if not pre.get("use_regex", True):
                raise NotImplementedError("ByteLevel(use_regex=False) alone: the text is not split into words")
            marks, resplit = False, False
            if pre.get("add_prefix_space"):
                if norm is not None:
                    raise NotImplementedError("Prepend(\" \") together with ByteLevel(add_prefix_space=True)")
                prefix_mode = PREFIX_UNLESS_SPACE
        elif pre.get("type") == "Sequence":
            steps = pre.get("pretokenizers") or []
            ok = (len(steps) == 2 and steps[0].get("type") == "Split" and steps[0].get("pattern") == {"Regex": SPLIT_PATTERN_MARKS}
                  and steps[0].get("behavior") == "Removed" and steps[0].get("invert") is True and steps[1].get("type") == "ByteLevel"
                  and not steps[1].get("add_prefix_space"))
            if not ok:
                raise NotImplementedError(f"pre-tokenizer {pre!r} (Split(the split pattern, removed, invert) then ByteLevel(add_prefix_space=False), or ByteLevel(use_regex=True))")
            marks, resplit = True, bool(steps[1].get("use_regex", True))
        else:
            raise NotImplementedError(f"pre-tokenizer {pre.get('type')!r}")
        prefix, suffix = cls._template(data.get("post_processor"))
        if len(prefix) > _lib.ENCODE_MAX_TEMPLATE or len(suffix) > _lib.ENCODE_MAX_TEMPLATE:
            raise NotImplementedError(f"more than {_lib.ENCODE_MAX_TEMPLATE} template ids on one side")
        strings = tuple(a["content"] for a in data.get("added_tokens") or [] if a.get("content"))
        spec = cls(prefix_mode, marks, resplit, prefix, suffix, int(pad_id), strings)
        if split_added_tokens:
            spec.split_added_tokens = True
            spec.added_tokens = tuple(AddedToken(a["content"], int(a["id"]), bool(a.get("normalized")), bool(a.get("lstrip")), bool(a.get("rstrip")), bool(a.get("single_word")))
                                      for a in data.get("added_tokens") or [] if a.get("content"))
            spec.added_table()          # (the cap refusals, before any device work)
        return spec

    @classmethod
    def from_tokenizer(cls, tokenizer, split_added_tokens: bool = False) -> "EncodeSpec":
        """From a transformers fast tokenizer (what ``Collator.sample_tokenizer`` returns, zett/collator.py:414-431)."""
        data = json.loads(tokenizer._tokenizer.to_str())
        strings = {a["content"] for a in data.get("added_tokens") or []} | set(getattr(tokenizer, "all_special_tokens", ()))
        spec = cls.from_tokenizer_json(data, tokenizer.pad_token_id, getattr(tokenizer, "padding_side", "right"), getattr(tokenizer, "truncation_side", "right"),
                                       split_added_tokens)
        spec.special_strings = tuple(sorted(s for s in strings if s))
        return spec

    def is_plain(self, token: AddedToken) -> bool:
        """Does the device split this token out?  Matched on the raw bytes, nothing swallowed around it: no ``lstrip`` / ``rstrip`` /
        ``single_word``, at least two bytes, and ``normalized`` only where there is no normalizer to look through."""
        if token.lstrip or token.rstrip or token.single_word or len(token.content.encode("utf-8")) < 2:
            return False
        return not (token.normalized and self.prefix_mode == PREFIX_ALWAYS)          # (PREFIX_ALWAYS is the Prepend(" ") normalizer)

    def added_table(self) -> Tuple[bytes, np.ndarray, np.ndarray]:
        """(bytes, int32 offsets [n + 1], int32 ids [n]) of the plain added tokens in ascending byte order: the table of
        zett_encode_texts_added.  Empty without ``split_added_tokens``."""
        plain: Dict[bytes, int] = {}
        for token in self.added_tokens if self.split_added_tokens else ():
            if self.is_plain(token):
                plain.setdefault(token.content.encode("utf-8"), token.id)
        if len(plain) > MAX_ADDED_TOKENS:
            raise NotImplementedError(f"{len(plain)} added tokens to split out: the device table holds {MAX_ADDED_TOKENS}")
        for raw, token_id in plain.items():
            if len(raw) > MAX_ADDED_TOKEN_BYTES:
                raise NotImplementedError(f"the added token {raw.decode('utf-8')!r} has {len(raw)} bytes, the device table carries {MAX_ADDED_TOKEN_BYTES}")
            if not -2 ** 31 <= token_id < 2 ** 31:
                raise ValueError(f"the added token {raw.decode('utf-8')!r} has an id outside int32")
        keys = sorted(plain)
        offsets = np.zeros(len(keys) + 1, dtype=np.int32)
        np.cumsum(np.array([len(k) for k in keys], dtype=np.int32), out=offsets[1:])
        return b"".join(keys), offsets, np.array([plain[k] for k in keys], dtype=np.int32)

    @property
    def refused_strings(self) -> Tuple[str, ...]:
        """What a text must not hold: every added or special string, or with ``split_added_tokens`` the backend tokens that are not plain."""
        if not self.split_added_tokens:
            return self.special_strings
        return tuple(a.content for a in self.added_tokens if not self.is_plain(a))

    @property
    def flags(self) -> int:
        return (_lib.ENCODE_MARKS_ARE_LETTERS if self.marks_are_letters else 0) | (_lib.ENCODE_RESPLIT if self.resplit else 0)

    def check_call(self, texts: Sequence[str], block_size: int, special_ids_map) -> Tuple[str, List[Tuple[int, int]]]:
        """The host's part of a call: the joined text and the id pairs; raises for what the kernels would answer differently."""
        t = int(block_size)
        if t <= len(self.prefix_ids) + len(self.suffix_ids):
            raise ValueError(f"block_size = {t} leaves no room for the text behind {len(self.prefix_ids) + len(self.suffix_ids)} template ids")
        if t > MAX_BLOCK_SIZE:
            raise ValueError(f"block_size = {t} is more than {MAX_BLOCK_SIZE}")
        pairs = [(int(k), int(v)) for k, v in (special_ids_map or {}).items()]
        if len(pairs) > _lib.SPLICE_MAX_ROWS:
            raise ValueError(f"special_ids_map holds {len(pairs)} pairs, at most {_lib.SPLICE_MAX_ROWS} travel with a launch")
        if any(not -2 ** 31 <= x < 2 ** 31 for p in pairs for x in p):
            raise ValueError("special_ids_map holds an id outside int32")
        joined = "".join(texts)
        for s in self.refused_strings:          # one str.find per refused string; the texts themselves only where the joined text has a hit
            if joined.find(s) >= 0 and any(s in x for x in texts):
                raise NotImplementedError(f"a text holds the added token {s!r}: the library would split it out")
        return joined, pairs


class DeviceTextEncoder:
    """``tokenizer(texts, max_length=block_size, truncation=True, padding="max_length", add_special_tokens=True)`` on one GPU."""

    def __init__(self, model_spec, encode_spec: EncodeSpec, device=None, table: Optional[np.ndarray] = None):
        from .surface_forms import DeviceRetokenizer
        self.device = default_device(device)
        if model_spec.kind not in (_lib.RETOK_BPE, _lib.RETOK_UNIGRAM):
            raise NotImplementedError("text encoding with a WordPiece model")
        self._adopt(DeviceRetokenizer(model_spec, self.device), encode_spec, table, None, True)

    def _adopt(self, retok, encode_spec: EncodeSpec, table, d_table, owns_handle: bool) -> None:
        self.spec = encode_spec
        self.retok = retok
        self.lib = retok.lib
        self.table, self._d_table = packed_table_on(self.device, table, d_table)
        k = _lib.ENCODE_MAX_TEMPLATE
        self._prefix = (C.c_int32 * k)(*encode_spec.prefix_ids)
        self._suffix = (C.c_int32 * k)(*encode_spec.suffix_ids)
        self._added = None          # the device table of zett_encode_texts_added: (bytes, offsets, ids, n, n_bytes)
        if encode_spec.split_added_tokens:
            raw, offsets, ids = encode_spec.added_table()
            if len(ids):
                import torch
                up = lambda a: torch.from_numpy(np.ascontiguousarray(a).copy()).to(self.device)          # noqa: E731
                self._added = (up(np.frombuffer(raw, dtype=np.uint8)), up(offsets), up(ids), len(ids), len(raw))
        self._owns_handle = owns_handle

    @classmethod
    def from_handle(cls, retok, encode_spec: EncodeSpec, table: Optional[np.ndarray] = None, d_table=None, split_added_tokens: Optional[bool] = None) -> "DeviceTextEncoder":
        """On a retokenizer handle that is already there and stays its owner's — ``DeviceSampledVocabulary`` rebuilds the tables of one
        handle every step (zett_amd/sampled_vocab.py).  ``retok``: a ``DeviceRetokenizer``; ``d_table``: the packed class table on its
        device, if the caller keeps one.  ``close()`` leaves the handle alone.  ``split_added_tokens``: the spec's switch, set anew
        (the spec's ``added_tokens`` are what is split)."""
        self = cls.__new__(cls)
        if split_added_tokens is not None and bool(split_added_tokens) != encode_spec.split_added_tokens:
            encode_spec = dataclasses.replace(encode_spec, split_added_tokens=bool(split_added_tokens))
        self.device = retok.device
        self._adopt(retok, encode_spec, table, d_table, False)
        return self

    @classmethod
    def from_tokenizer(cls, tokenizer, device=None, split_added_tokens: bool = False) -> "DeviceTextEncoder":
        from .surface_forms import HnTokenizerSpec
        encode_spec = EncodeSpec.from_tokenizer(tokenizer, split_added_tokens)          # (refusals first: no device work for a tokenizer that is not carried)
        return cls(HnTokenizerSpec.from_tokenizer(tokenizer), encode_spec, device)

    @classmethod
    def from_tokenizer_json(cls, data: Mapping, pad_token_id: int, special_tokens: Sequence[str] = (), special_ids: Sequence[int] = (), padding_side: str = "right",
                            truncation_side: str = "right", device=None, split_added_tokens: bool = False) -> "DeviceTextEncoder":
        """From a ``tokenizer.json`` dict and what transformers adds to it: the pad id, ``all_special_tokens`` / ``all_special_ids``, the sides."""
        from .surface_forms import HnTokenizerSpec
        encode_spec = EncodeSpec.from_tokenizer_json(data, pad_token_id, padding_side, truncation_side, split_added_tokens)
        encode_spec.special_strings = tuple(sorted(set(encode_spec.special_strings) | {s for s in special_tokens if s}))
        return cls(HnTokenizerSpec.from_model_json(data["model"], list(special_tokens), list(special_ids), pad_token_id), encode_spec, device)

    def workspace_bytes(self, n_text: int, n_texts: int) -> int:
        out = C.c_int64(0)
        if self.spec.split_added_tokens:
            n_added = self._added[3] if self._added else 0
            _lib.check(self.lib.zett_encode_added_workspace_bytes(int(n_text), int(n_texts), n_added, C.byref(out)), "zett_encode_added_workspace_bytes")
        else:
            _lib.check(self.lib.zett_encode_workspace_bytes(int(n_text), int(n_texts), C.byref(out)), "zett_encode_workspace_bytes")
        return out.value

    def __call__(self, texts: Sequence[str], block_size: int, special_ids_map: Optional[Dict[int, int]] = None, dtype=None, check: bool = True, out=None):
        """{"input_ids", "attention_mask"}: ``[len(texts), block_size]`` device tensors of ``dtype`` (int64, or int32).  ``out``: a pair
        of preallocated tensors of that shape (any row stride).  check=True reads the status word once and raises what the library
        raises (an unknown piece and no unk id: Exception); check=False never waits for the host."""
        import torch
        dtype = torch.int64 if dtype is None else dtype
        if dtype not in (torch.int32, torch.int64):
            raise ValueError("dtype must be torch.int32 or torch.int64")
        texts = list(texts)
        joined, pairs = self.spec.check_call(texts, block_size, special_ids_map)
        b, t = len(texts), int(block_size)
        blob, offsets = flatten_texts(texts, joined)
        with torch.cuda.device(self.device):
            if out is None:
                ids = torch.empty((b, t), dtype=dtype, device=self.device)
                mask = torch.empty((b, t), dtype=dtype, device=self.device)
            else:
                ids, mask = out
                for x in (ids, mask):
                    if x.dtype != dtype or tuple(x.shape) != (b, t) or x.device != self.device or (b and x.stride(1) != 1) or (b > 1 and x.stride(0) != ids.stride(0)):
                        raise ValueError(f"out must be two [{b}, {t}] tensors of {dtype} on {self.device} with unit column stride and one row stride")
            status = torch.empty(1, dtype=torch.int32, device=self.device)
            d_text = self.retok._to_device(np.frombuffer(blob or b"\0", dtype=np.uint8))
            d_off = self.retok._to_device(offsets)
            work = torch.empty(max(self.workspace_bytes(len(blob), b), 16), dtype=torch.uint8, device=self.device)          # (released on return: the allocator reuses it in stream order)
            n_map = len(pairs)
            m_from = (C.c_int32 * max(n_map, 1))(*[p[0] for p in pairs])
            m_to = (C.c_int32 * max(n_map, 1))(*[p[1] for p in pairs])
            ld = ids.stride(0) if b > 1 else t
            head = (self.retok.handle, ptr(d_text), ptr(d_off), b, len(blob), ptr(self._d_table), len(self.table), self.spec.flags, self.spec.prefix_mode, t,
                    self._prefix, len(self.spec.prefix_ids), self._suffix, len(self.spec.suffix_ids), m_from, m_to, n_map, self.spec.pad_id, ptr(ids if b else None),
                    ptr(mask if b else None), ids.element_size(), ld)
            tail = (ptr(work), work.numel(), ptr(status), stream(self.device))
            if self.spec.split_added_tokens:
                a_bytes, a_off, a_ids, n_added, n_added_bytes = self._added or (None, None, None, 0, 0)
                _lib.check(self.lib.zett_encode_texts_added(*head, ptr(a_bytes), ptr(a_off), ptr(a_ids), n_added, n_added_bytes, *tail), "zett_encode_texts_added")
            else:
                _lib.check(self.lib.zett_encode_texts(*head, *tail), "zett_encode_texts")
        if check:
            bits = int(status.item())          # (the one host read of this call)
            if bits & ENCODE_BAD_OFFSETS:
                raise ValueError("encode_texts: the text offsets are not non-decreasing from 0 to the text length")
            if bits & ENCODE_BAD_TABLE:
                raise ValueError("encode_texts: the table of added tokens is not sorted, or holds a token of fewer than 2 or more than 64 bytes")
            if bits & ENCODE_NO_UNK:
                raise Exception("Encountered an unknown token but `unk_id` is missing")          # tokenizers raises a bare Exception here
        self.last_status = status          # device int32 [1]: what a caller with check=False may look at later
        return {"input_ids": ids, "attention_mask": mask}

    def close(self) -> None:
        if self._owns_handle:
            self.retok.close()


def encode_texts(tokenizer_or_encoder, texts: Sequence[str], block_size: int, special_ids_map: Optional[Dict[int, int]] = None, dtype=None, check: bool = True,
                 device=None, split_added_tokens: bool = False):
    """``DeviceTextEncoder.from_tokenizer(tokenizer)(texts, block_size, ...)``; pass the encoder itself to keep its tables (and its
    ``split_added_tokens``: the switch is for a tokenizer)."""
    enc = tokenizer_or_encoder if isinstance(tokenizer_or_encoder, DeviceTextEncoder) else DeviceTextEncoder.from_tokenizer(tokenizer_or_encoder, device, split_added_tokens)
    return enc(texts, block_size, special_ids_map, dtype=dtype, check=check)
