"""A sampled tokenizer's vocabulary and encoder tables, built on the device — the host half of the reference's ``Collator.sample_tokenizer``
(zett/collator.py:371-452) without the list surgery, the ``tokenizers.Tokenizer`` and the per-piece host work.

    vocabulary = DeviceSampledVocabulary(reference, add_prefix_space=True, hn_tokenizer=hn_tokenizer, hn_surface_maxlen=7)      # once per reference
    encoder, special_ids_map, surface_forms, priors, byte_lengths = sample_tokenizer_device(
        texts, sampler, vocabulary, n_total=32768, noise_std=0.0)
    batch = encoder(texts, block_size=128, special_ids_map=special_ids_map)

``tokenizer_sampling.sample_tokenizer`` reads the sampler's list back, rebuilds it with Python lists, constructs a Tokenizer, and
``DeviceTextEncoder.from_tokenizer`` turns that into device tables again.  Here the list never leaves the device (csrc/sampled_vocab.hip,
DESIGN.md section 7i); the one host read of a step is a 32-byte record.

The first half of this file is the DEFINITION, plain numpy and no GPU: which id every piece gets, as a closed form.  With the
reference's special tokens ``(string_k, s_k)`` sorted by ``s_k`` and ``m`` pieces left after the removal of every piece that is a
special token's string, special ``k`` lands at ``pos_k = min(s_k, m + k)`` (``list.insert`` clamps to the end) and the kept pieces fill
the other ids in the sampler's order.  tests/test_sampled_vocab_host.py holds it to ``build_sampled_tokenizer``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from ._glue import default_device, ptr, stream
from .surface_forms import BYTES_TO_CHARS_LIST, CHARS_TO_BYTES, _raw
from .tokenizer_sampling import MAX_LENGTH, N_ALPHABET, DeviceTokenizerSampler, SampledPieces, build_sampled_tokenizer, n_fixed_pieces, raise_for_status

VOCAB_NOT_A_SAMPLE, VOCAB_DUPLICATE, VOCAB_TABLE_FULL, VOCAB_OUT_FULL = _lib.VOCAB_NOT_A_SAMPLE, _lib.VOCAB_DUPLICATE, _lib.VOCAB_TABLE_FULL, _lib.VOCAB_OUT_FULL
MAX_SPECIALS = _lib.SPLICE_MAX_ROWS
MAX_SPECIAL_BYTES = _lib.SAMPLED_VOCAB_KEY_BYTES
WHITESPACE_BYTES = (0x20, 0x0A, 0x09)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------
def byte_level_code_points() -> np.ndarray:
    """int32 [256]: the code point of the byte-level character of every byte — a byte b with 33 <= b <= 126, 161 <= b <= 172 or
    b >= 174 is code point b, every other byte 256 + its rank among those others (the ``cp_to_byte`` table of zett_retok_create,
    inverted)."""
    out = np.zeros(256, dtype=np.int32)
    rank = 0
    for b in range(256):
        if 33 <= b <= 126 or 161 <= b <= 172 or b >= 174:
            out[b] = b
        else:
            out[b] = 256 + rank
            rank += 1
    return out


def json_round_trip(x: float) -> float:
    """What a score becomes when the tokenizers library writes it to JSON and reads it back: the shortest decimal that identifies the
    double, digits ``D`` and ``s`` decimal places, read as ``float(D) / 10**s`` — two roundings where a correctly rounded reader has
    one, so about one score in nine moves by an ulp.  csrc/score_json.hip.h is this function for the kernels, which copy a score of more than 22
    decimal places (below 1e-6 in magnitude) unchanged."""
    from decimal import Decimal
    x = float(x)
    if x == 0.0 or x != x or x in (float("inf"), float("-inf")):
        return x
    _, digits, exp = Decimal(repr(abs(x))).as_tuple()
    d = int("".join(map(str, digits)))
    while d % 10 == 0:
        d //= 10
        exp += 1
    if exp >= 0:
        return x
    if -exp > 308:
        return x
    f = float(d) / float("1e%d" % -exp)
    return -f if x < 0 else f


def sorted_specials(special_tokens: Sequence[str], special_ids: Sequence[int]) -> Tuple[List[str], List[int]]:
    """The special tokens in the order the reference inserts them (``np.argsort`` of the ids), after the refusals."""
    tokens, ids = [str(t) for t in special_tokens], [int(i) for i in special_ids]
    if len(tokens) != len(ids):
        raise ValueError(f"{len(tokens)} special tokens and {len(ids)} special ids")
    if len(ids) > MAX_SPECIALS:
        raise ValueError(f"{len(ids)} special tokens, at most {MAX_SPECIALS} are carried")
    if any(i < 0 for i in ids):
        raise ValueError(f"a negative special id in {ids}: list.insert would count it from the end")
    if any(i >= 2 ** 31 for i in ids):
        raise ValueError("a special id outside int32")
    if len(set(ids)) != len(ids):
        raise ValueError(f"duplicate special ids in {ids}")
    if len(set(tokens)) != len(tokens):
        raise ValueError(f"duplicate special tokens in {tokens}")
    order = np.argsort(ids)
    return [tokens[i] for i in order], [ids[i] for i in order]


def sampled_vocabulary_layout(m: int, special_ids: Sequence[int]) -> Tuple[np.ndarray, Dict[int, int]]:
    """``(positions, special_ids_map)`` for ``m`` kept pieces: ``positions[k]`` is the final id of the special token with the k-th
    smallest id, ``min(s_k, m + k)``; the map holds ``s_k: positions[k]`` where they differ, keys in ascending order."""
    m = int(m)
    if m < 0:
        raise ValueError(f"m = {m} must not be negative")
    _, ids = sorted_specials([str(i) for i in range(len(special_ids))], special_ids)
    positions = np.array([min(s, m + k) for k, s in enumerate(ids)], dtype=np.int64)
    return positions, {s: int(p) for s, p in zip(ids, positions) if p != s}


class VocabularyLayout(NamedTuple):
    pieces: List[str]              # byte-level strings in id order
    scores: np.ndarray             # float64 [V]
    byte_lengths: np.ndarray       # int64 [V]
    special_ids_map: Dict[int, int]
    positions: np.ndarray          # int64 [S]: the final ids of the special tokens, by ascending special id
    n_removed: int


def prepend_unknown_chars(pieces_and_scores: Sequence[Tuple[str, float]]) -> List[Tuple[str, float]]:
    """zett/collator.py:373-376: the byte-level characters the list lacks, sorted, in front of it at the lowest score.  Nothing for a
    list of the device sampler, which always holds the 256 alphabet pieces; the kernels do not do this (ZETT_VOCAB_NOT_A_SAMPLE)."""
    pieces_and_scores = [(p, float(s)) for p, s in pieces_and_scores]
    unknown = sorted(set(CHARS_TO_BYTES) - {p for p, _ in pieces_and_scores})
    if not unknown:
        return pieces_and_scores
    low = min(s for _, s in pieces_and_scores)
    return [(c, low) for c in unknown] + pieces_and_scores


def layout_reference(pieces_and_scores: Sequence[Tuple[str, float]], special_tokens: Sequence[str], special_ids: Sequence[int]) -> VocabularyLayout:
    """The whole vocabulary of zett/collator.py:371-400 from the closed form: what csrc/sampled_vocab.hip must give for the list with
    its unknown characters prepended (``prepend_unknown_chars``; ``n_removed`` counts against that list)."""
    tokens, ids = sorted_specials(special_tokens, special_ids)
    pieces_and_scores = prepend_unknown_chars(pieces_and_scores)
    pieces = [p for p, _ in pieces_and_scores]
    scores = np.array([s for _, s in pieces_and_scores], dtype=np.float64)
    special = set(tokens)
    kept = [i for i, p in enumerate(pieces) if p not in special]
    m, s = len(kept), len(tokens)
    positions, special_ids_map = sampled_vocabulary_layout(m, ids)
    out_pieces: List[Optional[str]] = [None] * (m + s)
    out_scores = np.zeros(m + s, dtype=np.float64)
    lengths = np.zeros(m + s, dtype=np.int64)
    for k, pos in enumerate(positions):
        out_pieces[pos], lengths[pos] = tokens[k], len(tokens[k])
    for q, i in enumerate(kept):
        p = q
        for pos in positions:
            if pos <= p:
                p += 1
        assert out_pieces[p] is None
        out_pieces[p], out_scores[p], lengths[p] = pieces[i], scores[i], len(pieces[i])
    for v in range(m + s):          # the inverse, as the kernels use it
        before = int((positions < v).sum())
        assert (v in positions) or out_pieces[v] == pieces[kept[v - before]]
    return VocabularyLayout(out_pieces, out_scores, lengths, special_ids_map, positions, len(pieces) - m)


def fixed_pieces(max_length: int = MAX_LENGTH) -> List[Tuple[str, float]]:
    """The pieces every list of the sampler starts with: the 256 alphabet pieces in byte order (with scores -1.0 - 0.37 b here, a probe
    of how the library stores a score) and the whitespace runs (0.0)."""
    out = [(BYTES_TO_CHARS_LIST[b], -1.0 - 0.37 * b) for b in range(N_ALPHABET)]
    for c1 in WHITESPACE_BYTES:
        for i in range(1, int(max_length)):
            for c2 in WHITESPACE_BYTES:
                out.append((BYTES_TO_CHARS_LIST[c2] + BYTES_TO_CHARS_LIST[c1] * i, 0.0))
    assert len(out) == n_fixed_pieces(max_length)
    return out


def raise_for_vocab_status(bits: int) -> None:
    if bits & VOCAB_NOT_A_SAMPLE:
        raise NotImplementedError("sampled vocabulary: fewer than 256 pieces — the list lacks alphabet pieces, which the reference would prepend")
    if bits & VOCAB_DUPLICATE:
        raise ValueError("sampled vocabulary: the list holds a piece twice")
    if bits & VOCAB_TABLE_FULL:
        raise RuntimeError("sampled vocabulary: the piece table is full")
    if bits & VOCAB_OUT_FULL:
        raise RuntimeError("sampled vocabulary: more pieces than seed_size, or more ids or token text than the outputs hold")


# ---- the device ---------------------------------------------------------------------------------------------------------------------------
class SampledVocabulary(NamedTuple):
    """What ``DeviceSampledVocabulary.build`` returns.  The encoder works on the vocabulary's one handle: the next ``build`` replaces its
    tables."""
    encoder: "object"                          # DeviceTextEncoder
    special_ids_map: Dict[int, int]
    surface_forms: "object"                    # device int32 [V, hn_surface_maxlen], or None
    priors: "object"                           # device float64 [V]
    byte_lengths: "object"                     # device int64 [V]
    n_vocab: int
    n_removed: int
    min_score: float                           # over priors
    status: int
    table_min_score: float                     # over the scores as the encoder's table holds them: its unknown score is this - 10


class DeviceSampledVocabulary:
    """Everything that depends on the ``reference`` tokenizer alone, once: its special tokens (sorted, as raw bytes, with their hn ids),
    the hn retokenizer, how texts are split and framed (``EncodeSpec``), the class table, and the handle whose tables every ``build``
    fills again.  All allocation that does not depend on the step's size happens here."""

    def __init__(self, reference, add_prefix_space: bool, hn_tokenizer=None, hn_surface_maxlen: Optional[int] = None, max_vocab: int = 1 << 16, device=None):
        import torch

        from .surface_forms import DeviceRetokenizer, device_retokenizer
        from .text_encode import EncodeSpec, packed_table_on
        if hn_tokenizer is not None and hn_surface_maxlen is None:
            raise ValueError("hn_surface_maxlen is required with an hn_tokenizer")
        tokens, ids = sorted_specials(list(reference.all_special_tokens), [int(i) for i in reference.all_special_ids])
        raws: List[bytes] = []
        hn_specials = set(hn_tokenizer.all_special_tokens) if hn_tokenizer is not None else set()
        hn_ids = []
        for token in tokens:
            raw = _raw(token)
            is_hn = token in hn_specials
            if raw is None and hn_tokenizer is not None and not is_hn:          # get_surface_form_matrix would raise (zett/utils.py:675)
                raise KeyError(next(ch for ch in token if ch not in CHARS_TO_BYTES))
            if raw is not None and len(raw) > MAX_SPECIAL_BYTES:
                raise NotImplementedError(f"the special token {token!r} has {len(raw)} raw bytes, the device table carries {MAX_SPECIAL_BYTES}")
            raws.append(raw or b"")
            hn_ids.append(int(hn_tokenizer.convert_tokens_to_ids(token)) if is_hn else -1)
        self.device = default_device(device)
        if self.device.type != "cuda":
            raise RuntimeError("zett_amd computes on MI355X only: the sampled vocabulary needs a cuda (ROCm) device; there is no CPU path")
        self.special_tokens, self.special_ids, self.special_raw, self.special_hn_ids = tokens, ids, raws, hn_ids
        self.max_vocab = int(max_vocab)
        self.hn_surface_maxlen = None if hn_surface_maxlen is None else int(hn_surface_maxlen)
        # normalizer, pre-tokenizer, post-processor and special strings as the installed library serialises them for a tokenizer built the
        # reference's way — read, never guessed; the pad id alone depends on the step (the pad token may sit beyond the end)
        fixed_tokenizer = build_sampled_tokenizer(fixed_pieces(), reference, add_prefix_space)[0]
        self.encode_spec = EncodeSpec.from_tokenizer(fixed_tokenizer, split_added_tokens=True)          # (its backend holds no added token: a special's string is text)
        self._pad_k = tokens.index(reference.pad_token)
        self.scores_through_json = self._probe_scores(fixed_tokenizer, tokens)
        self.hn = device_retokenizer(hn_tokenizer, self.device) if hn_tokenizer is not None else None
        self.lib = _lib.load()
        with torch.cuda.device(self.device):
            self.table, self._d_table = packed_table_on(self.device, None)
            offsets = np.zeros(len(raws) + 1, dtype=np.int32)
            np.cumsum(np.array([len(r) for r in raws], dtype=np.int32), out=offsets[1:])
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)          # noqa: E731
            self._d_ids = up(np.array(ids + [0], dtype=np.int32))          # (never an empty tensor: its pointer would be null)
            self._d_raw_off = up(offsets)
            self._d_raw = up(np.frombuffer(b"".join(raws) + b"\0", dtype=np.uint8).copy())
            self._d_chars = up(np.array([len(t) for t in tokens] + [0], dtype=np.int32))
            self._d_hn = up(np.array(hn_ids + [-1], dtype=np.int32))
            self._raw_bytes = int(offsets[-1])
            self._max_raw = max([len(r) for r in raws], default=0)
            need = C.c_int64(0)
            _lib.check(self.lib.zett_sampled_vocab_workspace_bytes(self.max_vocab, len(ids), C.byref(need)), "zett_sampled_vocab_workspace_bytes")
            self._work = torch.empty(max(need.value, 16), dtype=torch.uint8, device=self.device)
            self.retok = DeviceRetokenizer.unigram_on_device(self.device, self.max_vocab)

    @staticmethod
    def _probe_scores(fixed_tokenizer, special_tokens: Sequence[str] = ()) -> bool:
        """Does the model of a tokenizer built the reference's way hold the sampler's scores, or what the library's JSON round trip makes
        of them (transformers 5 rebuilds the backend from JSON)?  Read from the 256 probe scores of ``fixed_pieces``, never guessed."""
        import json
        held = {p: float(s) for p, s in json.loads(fixed_tokenizer._tokenizer.to_str())["model"]["vocab"]}
        given = [(p, s) for p, s in fixed_pieces()[:N_ALPHABET] if p in held and p not in special_tokens]
        if all(held[p] == s for p, s in given):
            return False
        if all(held[p] == json_round_trip(s) for p, s in given):
            return True
        raise NotImplementedError("the installed tokenizers / transformers store a Unigram score neither as given nor as their JSON round trip gives it")

    @property
    def n_special(self) -> int:
        return len(self.special_ids)

    def build(self, sampled: SampledPieces, seed_size: int, check: bool = True) -> SampledVocabulary:
        """From the sampler's device list to the step's vocabulary.  ``seed_size``: what the sampler was asked for (it bounds the list).
        Reads the 32-byte record once — the map, the text length and the unknown score depend on it; ``check`` raises for its status
        bits, for the sampler's and for what the hn retokenizer reports."""
        import torch
        cap = int(sampled.pieces.shape[0])
        bound = max(int(seed_size), min(cap, n_fixed_pieces(MAX_LENGTH) + 1), 1)          # the sampler always lets one piece of the table through
        s = self.n_special
        if bound + s > self.max_vocab:
            raise ValueError(f"seed_size + specials = {bound} + {s} is more than max_vocab = {self.max_vocab}")
        for name, t, dt in (("pieces", sampled.pieces, torch.uint8), ("lengths", sampled.lengths, torch.uint8), ("scores", sampled.scores, torch.float64), ("n", sampled.n, torch.int32)):
            if t.dtype != dt or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"sampled.{name} must be a contiguous {dt} tensor on {self.device}")
        if sampled.pieces.dim() != 2 or sampled.pieces.shape[1] != 16 or sampled.lengths.numel() < cap or sampled.scores.numel() < cap or cap < 1:
            raise ValueError("sampled: pieces [capacity, 16], lengths [capacity], scores [capacity]")
        v_cap = min(cap, bound) + s
        text_cap = 2 * 16 * min(cap, bound) + 2 * self._raw_bytes + 16
        with torch.cuda.device(self.device):
            priors = torch.empty(v_cap, dtype=torch.float64, device=self.device)
            byte_lengths = torch.empty(v_cap, dtype=torch.int64, device=self.device)
            text_offsets = torch.empty(v_cap + 1, dtype=torch.int32, device=self.device)
            text = torch.empty(text_cap, dtype=torch.uint8, device=self.device)
            record = torch.empty(4 + (1 if check else 0), dtype=torch.int64, device=self.device)
            st = stream(self.device)
            rc = self.lib.zett_sampled_vocab_build(self.retok.handle, ptr(sampled.pieces), ptr(sampled.lengths), ptr(sampled.scores), ptr(sampled.n), cap, bound,
                                                   ptr(self._d_ids), ptr(self._d_raw_off), ptr(self._d_raw), ptr(self._d_chars), ptr(self._d_hn), s, self._raw_bytes, self._max_raw,
                                                   ptr(priors), ptr(byte_lengths), ptr(text_offsets), v_cap, ptr(text), text_cap, ptr(record), _lib.VOCAB_SCORES_THROUGH_JSON if self.scores_through_json else 0, ptr(self._work), self._work.numel(), st)
            _lib.check(rc, "zett_sampled_vocab_build")
            if check:          # the sampler's status word rides along: still one read
                record[4:5] = sampled.status.to(torch.int64)
            host = record.cpu().numpy()          # (the one host read of a step)
        rec = _lib.ZettSampledVocabRecord.from_buffer_copy(host[:4].tobytes())
        if check:
            raise_for_status(int(host[4]))
            raise_for_vocab_status(rec.status)
        _lib.check(self.lib.zett_sampled_vocab_commit(self.retok.handle, C.byref(rec)), "zett_sampled_vocab_commit")
        n_vocab = int(rec.n_vocab)
        positions, special_ids_map = sampled_vocabulary_layout(max(n_vocab - s, 0), self.special_ids)
        surface_forms = None
        if self.hn is not None:
            n_out = min(n_vocab, v_cap)
            with torch.cuda.device(self.device):
                if self.hn._outstanding:
                    self.hn.result()
                text._zett_n_text = int(rec.n_text)
                surface_forms = self.hn.run_async(text, text_offsets, n_out, self.hn_surface_maxlen)
                _lib.check(self.lib.zett_sampled_vocab_patch_rows(self.retok.handle, ptr(record), ptr(self._d_ids), ptr(self._d_hn), s, ptr(surface_forms), n_out,
                                                                  self.hn_surface_maxlen, self.hn.spec.pad_token_id, st), "zett_sampled_vocab_patch_rows")
                if check:
                    self.hn.result()
        from .text_encode import DeviceTextEncoder
        spec = dataclasses.replace(self.encode_spec, pad_id=int(positions[self._pad_k]))
        encoder = DeviceTextEncoder.from_handle(self.retok, spec, self.table, self._d_table)
        return SampledVocabulary(encoder, special_ids_map, surface_forms, priors[:min(n_vocab, v_cap)], byte_lengths[:min(n_vocab, v_cap)], n_vocab, int(rec.n_removed),
                                 float(rec.min_score), int(rec.status), float(rec.table_min_score))

    def piece_table(self) -> Tuple[List[bytes], np.ndarray, np.ndarray, np.ndarray]:
        """Debug read-out of the handle's piece table after a build: (keys as raw bytes, ids int32, scores float64) of the occupied
        slots in no particular order, and single_id int32 [256]."""
        import torch
        cap = self.max_vocab
        with torch.cuda.device(self.device):
            keys = torch.zeros((cap, MAX_SPECIAL_BYTES), dtype=torch.uint8, device=self.device)
            lengths = torch.zeros(cap, dtype=torch.int32, device=self.device)
            ids = torch.zeros(cap, dtype=torch.int32, device=self.device)
            scores = torch.zeros(cap, dtype=torch.float64, device=self.device)
            single = torch.zeros(256, dtype=torch.int32, device=self.device)
            n = torch.zeros(1, dtype=torch.int32, device=self.device)
            _lib.check(self.lib.zett_sampled_vocab_table(self.retok.handle, ptr(keys), ptr(lengths), ptr(ids), ptr(scores), ptr(single), cap, ptr(n),
                                                         stream(self.device)), "zett_sampled_vocab_table")
            count = min(int(n.item()), cap)
            k, ln = keys[:count].cpu().numpy(), lengths[:count].cpu().numpy()
        return [bytes(k[i, :ln[i]]) for i in range(count)], ids[:count].cpu().numpy(), scores[:count].cpu().numpy(), single.cpu().numpy()

    def close(self) -> None:
        if getattr(self, "retok", None) is not None:
            self.retok.close()
            self.retok = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def sample_tokenizer_device(texts: Sequence[str], sampler: DeviceTokenizerSampler, vocabulary: DeviceSampledVocabulary, *, n_total: int, noise_std: float,
                            is_validation: bool = False, seed: int = 0, check: bool = True):
    """The device twin of ``tokenizer_sampling.sample_tokenizer``: the reference's 5-tuple with a ``DeviceTextEncoder`` in place of the
    tokenizer, and surface forms, priors and byte lengths as device tensors.  ``add_prefix_space``, the hn tokenizer and its
    ``hn_surface_maxlen`` are the vocabulary's."""
    if not isinstance(sampler, DeviceTokenizerSampler):
        raise TypeError("sample_tokenizer_device takes a DeviceTokenizerSampler: its list stays on the device")
    sampled = sampler.sample_tokenizer({text: 1 for text in texts}, int(n_total), MAX_LENGTH, 4, noise_std, True, not is_validation, seed=seed, check=False)
    built = vocabulary.build(sampled, int(n_total), check=check)
    return built.encoder, built.special_ids_map, built.surface_forms, built.priors, built.byte_lengths
