"""A step's Unigram tokenizer sampled from the batch, on the device — the reference's ``do_tokenizer_sampling`` mode
(zett/collator.py:341-452, 503-514) without ``rust_utils``.

    sampler = DeviceTokenizerSampler()                                   # once per pool: owns the queue of earlier batches
    sampler.sample_tokenizer(texts, 30_000, 16, 4, 0.0, False)           # fill the queue (collator.py:142-149)
    tokenizer, special_ids_map, surface_forms, priors, byte_lengths = sample_tokenizer(
        texts, sampler, reference, n_total=32768, noise_std=0.0, add_prefix_space=True, hn_tokenizer=hn_tokenizer, hn_surface_maxlen=7)

``DeviceTokenizerSampler`` has the surface of ``rust_utils.TokenizerSampler`` (rust_utils/src/lib.rs:70-249): it counts the substrings
of the batch's pre-tokens, keeps a queue of earlier batches' counts and returns the ``seed_size`` best ``(piece, log-probability)``
pairs — csrc/tokenizer_sample.hip; tests/sampler_ref.py is the plain-Python definition.  Per call the host joins and
encodes the texts once; the result stays on the device unless ``as_list`` asks for the Rust class's list.

``sample_tokenizer`` is the host half of ``Collator.sample_tokenizer``: from the ``(piece, score)`` list to the ``tokenizers.Tokenizer``
and the reference's 5-tuple.  Drawing ``n_total`` and ``noise_std`` from ``np.random`` stays with the caller.  There is no CPU path for
the sampler itself.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Mapping, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np

from . import _lib
from ._glue import default_device, ptr, stream
from .surface_forms import BYTES_TO_CHARS_LIST, CHARS_TO_BYTES
from .text_encode import SPLIT_PATTERN_MARKS, flatten_texts, packed_table_on

SAMPLE_BAD_OFFSETS, SAMPLE_TABLE_FULL, SAMPLE_LIST_FULL = _lib.SAMPLE_BAD_OFFSETS, _lib.SAMPLE_TABLE_FULL, _lib.SAMPLE_LIST_FULL
SAMPLE_SUM_OVERFLOW, SAMPLE_OUT_FULL = _lib.SAMPLE_SUM_OVERFLOW, _lib.SAMPLE_OUT_FULL
N_ALPHABET = 256
MAX_LENGTH = 16


def n_fixed_pieces(max_length: int) -> int:
    """the 256 alphabet pieces and the whitespace runs in front of the table's pieces"""
    return N_ALPHABET + 9 * (int(max_length) - 1)


class SampledPieces(NamedTuple):
    """Device results of a call.  Rows [0, n) are valid: ``pieces`` uint8 [capacity, 16] raw key bytes, zero padded; ``lengths`` uint8
    [capacity]; ``scores`` float64 [capacity]; ``n`` int32 [1]; ``status`` int32 [1] (zett_sample_status bits)."""
    pieces: "object"
    lengths: "object"
    scores: "object"
    n: "object"
    status: "object"

    def to_list(self) -> List[Tuple[str, float]]:
        """``[(byte-level string, score)]``: what ``rust_utils.TokenizerSampler.sample_tokenizer`` returns (one host read)."""
        n = int(self.n.item())
        pieces, lengths, scores = self.pieces[:n].cpu().numpy(), self.lengths[:n].cpu().numpy(), self.scores[:n].cpu().numpy()
        return [("".join(BYTES_TO_CHARS_LIST[b] for b in pieces[i, :lengths[i]]), float(scores[i])) for i in range(n)]


def _texts_of(texts_or_counts) -> List[str]:
    if isinstance(texts_or_counts, Mapping):
        for text, count in texts_or_counts.items():
            if count != 1:
                raise NotImplementedError(f"a text with count {count!r}: the reference passes every text with count 1 (zett/collator.py:351-353)")
        texts = list(texts_or_counts)
    else:
        if isinstance(texts_or_counts, (str, bytes)):
            raise TypeError("texts must be a sequence of str or a mapping from str to 1, not one string")
        texts = list(dict.fromkeys(texts_or_counts))          # the reference takes the texts as dictionary keys: a duplicate counts once
    for text in texts:
        if not isinstance(text, str):
            raise TypeError(f"a text must be a str, not {type(text).__name__}")
    return texts


class DeviceTokenizerSampler:
    """``rust_utils.TokenizerSampler`` on one GPU.  The capacities are fixed at creation, where all allocation happens:
    ``max_depth`` batches in the queue, ``table_capacity`` slots for the distinct substrings of the whole queue, ``list_capacity``
    distinct substrings of one batch (default: half the table), ``max_pieces`` pieces of the table in one result."""

    def __init__(self, device=None, max_depth: int = 16, table_capacity: int = 1 << 22, list_capacity: Optional[int] = None, max_pieces: int = 1 << 16,
                 table: Optional[np.ndarray] = None):
        import torch
        self.device = default_device(device)
        if self.device.type != "cuda":
            raise RuntimeError("zett_amd computes on MI355X only: the sampler needs a cuda (ROCm) device; there is no CPU path")
        self.lib = _lib.load()
        self.max_depth, self.table_capacity, self.max_pieces = int(max_depth), int(table_capacity), int(max_pieces)
        self.list_capacity = int(list_capacity) if list_capacity is not None else max(1, self.table_capacity // 2)
        self.table, self._d_table = packed_table_on(self.device, table)
        handle = C.c_void_p()
        index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        _lib.check(self.lib.zett_sampler_create(index, self.max_depth, self.list_capacity, self.table_capacity, self.max_pieces, C.byref(handle)), "zett_sampler_create")
        self.handle = handle
        self.last_status = None

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.zett_sampler_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def depth(self) -> int:
        out = C.c_int32(0)
        _lib.check(self.lib.zett_sampler_depth(self.handle, C.byref(out)), "zett_sampler_depth")
        return out.value

    def sample_tokenizer(self, texts_or_counts: Union[Sequence[str], Mapping[str, int]], seed_size: int, max_length: int = MAX_LENGTH, stride: int = 1,
                         noise_std: float = 0.0, pop_prev: bool = True, push_current: bool = True, *, seed: int = 0, check: bool = True, as_list: bool = False):
        """The arguments of the Rust class's method, then ``seed`` (64 bits: the noise is a function of seed and piece), ``check`` (read
        the status word once and raise) and ``as_list`` (read the result back as the Rust class's ``[(str, float)]``).  Returns
        ``SampledPieces`` (``n == 0`` without ``pop_prev``)."""
        import torch
        texts = _texts_of(texts_or_counts)
        seed_size, max_length, stride = int(seed_size), int(max_length), int(stride)
        if not 1 <= max_length <= MAX_LENGTH:
            raise ValueError(f"max_length = {max_length} must be in [1, {MAX_LENGTH}]: a key is at most {MAX_LENGTH - 1} bytes")
        if stride < 1:
            raise ValueError(f"stride = {stride} must be at least 1")
        if seed_size < 0:
            raise ValueError(f"seed_size = {seed_size} must not be negative")
        noise_std = float(noise_std)
        if not 0.0 <= noise_std < float("inf"):
            raise ValueError(f"noise_std = {noise_std} must be a finite number >= 0")
        fixed = n_fixed_pieces(max_length)
        k = max(1, seed_size - fixed)
        if pop_prev and k > self.max_pieces:
            raise ValueError(f"seed_size = {seed_size} asks for {k} pieces of the table, the sampler was created with max_pieces = {self.max_pieces}")
        if not pop_prev and push_current and self.depth >= self.max_depth:
            raise RuntimeError(f"the queue holds {self.depth} batches, the sampler was created with max_depth = {self.max_depth}")
        b = len(texts)
        blob, offsets = flatten_texts(texts)
        cap = fixed + k if pop_prev else 1
        with torch.cuda.device(self.device):
            pieces = torch.zeros((cap, 16), dtype=torch.uint8, device=self.device)
            lengths = torch.zeros(cap, dtype=torch.uint8, device=self.device)
            scores = torch.zeros(cap, dtype=torch.float64, device=self.device)
            n = torch.zeros(1, dtype=torch.int32, device=self.device)
            status = torch.zeros(1, dtype=torch.int32, device=self.device)
            d_text = torch.from_numpy(np.frombuffer(blob or b"\0", dtype=np.uint8).copy()).to(self.device)
            d_off = torch.from_numpy(np.ascontiguousarray(offsets)).to(self.device)
            need = C.c_int64(0)
            _lib.check(self.lib.zett_sampler_workspace_bytes(len(blob), b, C.byref(need)), "zett_sampler_workspace_bytes")
            work = torch.empty(max(need.value, 16), dtype=torch.uint8, device=self.device)
            rc = self.lib.zett_sampler_sample(self.handle, ptr(d_text), ptr(d_off), b, len(blob), ptr(self._d_table), len(self.table), seed_size, max_length, stride,
                                              noise_std, int(seed) & (2 ** 64 - 1), int(bool(pop_prev)), int(bool(push_current)), ptr(pieces), ptr(lengths), ptr(scores),
                                              cap, ptr(n), ptr(work), work.numel(), ptr(status), stream(self.device))
            _lib.check(rc, "zett_sampler_sample")
        self.last_status = status
        if check:
            raise_for_status(int(status.item()))
        out = SampledPieces(pieces, lengths, scores, n, status)
        return out.to_list() if as_list else out

    def merged_table(self) -> Tuple[List[bytes], np.ndarray, np.ndarray]:
        """Debug read-out after a call with ``pop_prev``: (keys as raw bytes, counts uint32, z float64 of that call's seed), in no
        particular order."""
        import torch
        cap = self.table_capacity
        with torch.cuda.device(self.device):
            keys = torch.zeros((cap, 16), dtype=torch.uint8, device=self.device)
            lengths = torch.zeros(cap, dtype=torch.uint8, device=self.device)
            counts = torch.zeros(cap, dtype=torch.int32, device=self.device)
            z = torch.zeros(cap, dtype=torch.float64, device=self.device)
            n = torch.zeros(1, dtype=torch.int32, device=self.device)
            _lib.check(self.lib.zett_sampler_table(self.handle, ptr(keys), ptr(lengths), ptr(counts), ptr(z), cap, ptr(n), stream(self.device)), "zett_sampler_table")
        m = min(int(n.item()), cap)
        k, ln = keys[:m].cpu().numpy(), lengths[:m].cpu().numpy()
        return [bytes(k[i, :ln[i]]) for i in range(m)], counts[:m].cpu().numpy().view(np.uint32), z[:m].cpu().numpy()


def raise_for_status(bits: int) -> None:
    if bits & SAMPLE_BAD_OFFSETS:
        raise ValueError("sample_tokenizer: the text offsets are not non-decreasing from 0 to the text length")
    if bits & SAMPLE_TABLE_FULL:
        raise RuntimeError("sample_tokenizer: the substring table is full (table_capacity at creation)")
    if bits & SAMPLE_LIST_FULL:
        raise RuntimeError("sample_tokenizer: the batch has more distinct substrings than list_capacity")
    if bits & SAMPLE_SUM_OVERFLOW:
        raise OverflowError("sample_tokenizer: the sum of the scores reached 2**32, where the reference's u32 wraps")
    if bits & SAMPLE_OUT_FULL:
        raise RuntimeError("sample_tokenizer: more pieces than the output holds")


# ---- the host half of Collator.sample_tokenizer (zett/collator.py:363-452) ----------------------------------------------------------------
def build_sampled_tokenizer(pieces_and_scores: Sequence[Tuple[str, float]], reference, add_prefix_space: bool):
    """From the sampler's list to (PreTrainedTokenizerFast, special_ids_map, scores float64 [V]): unknown characters filled in at the
    lowest score, the reference's special-token strings removed from the pieces and inserted at their ids."""
    import tokenizers
    from tokenizers import Tokenizer, decoders, models, normalizers, pre_tokenizers
    from transformers import PreTrainedTokenizerFast
    if not pieces_and_scores:
        raise ValueError("the sampler returned no pieces (a call without pop_prev returns none)")
    pieces = [p for p, _ in pieces_and_scores]
    scores = [float(s) for _, s in pieces_and_scores]
    piece_set = set(pieces)
    unknown_chars = set(CHARS_TO_BYTES.keys()) - piece_set
    min_score = min(scores)
    pieces = sorted(unknown_chars) + pieces
    scores = [min_score] * len(unknown_chars) + scores
    special_tokens, special_ids = list(reference.all_special_tokens), [int(i) for i in reference.all_special_ids]
    for token in set(special_tokens) & piece_set:
        idx = pieces.index(token)
        pieces.pop(idx)
        scores.pop(idx)
    special_ids_map: Dict[int, int] = {}
    for i in np.argsort(special_ids):
        pieces.insert(special_ids[i], special_tokens[i])
        scores.insert(special_ids[i], 0.0)
        at = pieces.index(special_tokens[i])
        if at != special_ids[i]:
            special_ids_map[special_ids[i]] = at
    scores_arr = np.array(scores)
    tk = Tokenizer(models.Unigram([(piece, score) for piece, score in zip(pieces, scores_arr)]))
    if add_prefix_space:
        tk.normalizer = normalizers.Prepend(" ")
    tk.pre_tokenizer = pre_tokenizers.Sequence([pre_tokenizers.Split(tokenizers.Regex(SPLIT_PATTERN_MARKS), "removed", invert=True),
                                                pre_tokenizers.ByteLevel(False, False)])
    tk.decoder = decoders.ByteLevel()
    tokenizer = PreTrainedTokenizerFast(tokenizer_object=tk, clean_up_tokenization_spaces=False)
    if reference._tokenizer.post_processor is not None:
        tokenizer._tokenizer.post_processor = reference._tokenizer.post_processor
    for name in ("eos_token", "pad_token", "sep_token", "unk_token", "bos_token", "cls_token", "mask_token"):
        setattr(tokenizer, name, getattr(reference, name))
    return tokenizer, special_ids_map, scores_arr


def sample_tokenizer(texts: Sequence[str], sampler, reference, *, n_total: int, noise_std: float, add_prefix_space: bool, is_validation: bool = False,
                     hn_tokenizer=None, hn_surface_maxlen: Optional[int] = None, seed: int = 0):
    """``Collator.sample_tokenizer(texts, sampler)`` with what it draws from ``np.random`` as arguments.  ``sampler``: a
    ``DeviceTokenizerSampler``, or anything with the Rust class's ``sample_tokenizer(map, seed_size, max_length, stride, noise_std,
    pop_prev, push_current)``.  Returns the reference's 5-tuple: (tokenizer, special_ids_map, surface forms or None, priors, byte_lengths)."""
    if hn_tokenizer is not None and hn_surface_maxlen is None:
        raise ValueError("hn_surface_maxlen is required with an hn_tokenizer")
    counts = {text: 1 for text in texts}
    if isinstance(sampler, DeviceTokenizerSampler):
        found = sampler.sample_tokenizer(counts, int(n_total), 16, 4, noise_std, True, not is_validation, seed=seed, as_list=True)
    else:
        found = sampler.sample_tokenizer(counts, int(n_total), 16, 4, noise_std, True, not is_validation)
    tokenizer, special_ids_map, scores = build_sampled_tokenizer(found, reference, add_prefix_space)
    tokens = tokenizer.convert_ids_to_tokens(range(len(tokenizer)))
    byte_lengths = np.array([len(token) for token in tokens])
    surface_forms = None
    if hn_tokenizer is not None:
        from .surface_forms import get_surface_form_matrix
        surface_forms = get_surface_form_matrix(tokens, hn_surface_maxlen, hn_tokenizer, verbose=False)[0]
    return tokenizer, special_ids_map, surface_forms, scores, byte_lengths
