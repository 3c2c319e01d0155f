"""The rest of the reference's ``Collator`` (zett/collator.py) on the device: the inner collator (MLM or CLM labels), ``byte_lengths`` and
the two metrics of ``encode`` (collator.py:180-205), the padded-vocabulary branch (collator.py:283-337), and ``DeviceCollator``, which
orders these and the pieces of ``zett_amd.training`` into ``Collator.__call__``'s dict.

    lb = label_batch(input_ids, tokenizer.all_special_ids, byte_lengths, vocab_len=len(tokenizer), loss="mlm", mask_token_id=tokenizer.mask_token_id,
                     unk_token_id=tokenizer.unk_token_id, seed=step)
    pv = pad_vocabulary(surface_forms, priors, n_rows)

    collate = DeviceCollator(reference, hn_tokenizer, data_args, loss="mlm", tokenizer=tokenizer)
    batch = collate([{"texts": texts, "lang_code": "en"}], seed=step)

The labelling pass and the padding are HIP kernels (csrc/train_batch.hip: zett_op_label_batch, zett_op_pad_vocabulary).  One deviation from
the reference: the MLM draws are a counter-based hash of ``(seed, position)`` defined in include/zett_hip.h, not numpy's global generator;
the arithmetic on the draws is the installed ``DataCollatorForLanguageModeling.numpy_mask_tokens``'s, element for element.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._glue import default_device, ptr, stream

LABEL_BAD_ID = _lib.LABEL_BAD_ID
NEGATIVE_INF_FILL_VALUE = -100000.0          # zett/utils.py
MAX_CHARS_PER_TOKEN = 16                     # zett/utils.py
_MASK64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_LOSSES = {"clm": _lib.LABEL_CLM, "mlm": _lib.LABEL_MLM}


def mlm_thresholds(mlm_probability: float = 0.15, mask_replace_prob: float = 0.8, random_replace_prob: float = 0.1) -> Tuple[int, int, int]:
    """``(t_mask, t_replace, t_random)`` for ``label_batch``: ``t = ceil(prob * 2^53)`` in float64, so that a 53-bit draw k satisfies
    ``k < t`` exactly when ``k * 2^-53 < prob``.  The probabilities are those of ``DataCollatorForLanguageModeling``: a position that
    is not special is masked with ``mlm_probability``; a masked one becomes the mask token with ``mask_replace_prob``; one that does
    not becomes a random id with ``random_replace_prob / (1 - mask_replace_prob)``, evaluated as the library evaluates it (the defaults
    give 0.5000000000000001).  ``t_random = 0`` when ``mask_replace_prob == 1`` or ``random_replace_prob == 0`` (the library returns
    before it draws).  The library's ValueErrors for a probability outside [0, 1] or ``mask_replace_prob + random_replace_prob > 1``."""
    if mlm_probability is None or mlm_probability < 0 or mlm_probability > 1:
        raise ValueError("mlm_probability should be between 0 and 1.")
    if mask_replace_prob + random_replace_prob > 1:
        raise ValueError("The sum of mask_replace_prob and random_replace_prob should not exceed 1")
    if mask_replace_prob < 0 or mask_replace_prob > 1:
        raise ValueError("mask_replace_prob should be between 0 and 1.")
    if random_replace_prob < 0 or random_replace_prob > 1:
        raise ValueError("random_replace_prob should be between 0 and 1.")
    p_mask, p_replace, p_random = float(mlm_probability), float(mask_replace_prob), float(random_replace_prob)
    scale = float(1 << 53)
    if p_replace == 1 or p_random == 0:
        t_random = 0
    else:
        t_random = min(int(math.ceil(p_random / (1 - p_replace) * scale)), 1 << 53)
    return int(math.ceil(p_mask * scale)), int(math.ceil(p_replace * scale)), t_random


class LabelledBatch(NamedTuple):
    """What ``label_batch`` returns, all on the device."""
    input_ids: torch.Tensor          # [B, S], dtype of the input: the ids after masking (the given tensor with inplace=True)
    labels: torch.Tensor             # [B, S], same dtype: clm — the ids; mlm — the id where masked, else -100
    byte_lengths: torch.Tensor       # [B, S] int64: byte_lengths_per_token[input_ids]
    metrics: torch.Tensor            # [2] float64: avg_byte_length, unk_ratio
    record: torch.Tensor             # [8] int64: positions, non-special, their byte sum, unk, masked, replaced, random, status


def label_batch(input_ids, special_ids: Sequence[int], byte_lengths_per_token, *, vocab_len: int, loss: str = "clm", mask_token_id: Optional[int] = None,
                unk_token_id: Optional[int] = None, seed: int = 0, thresholds: Optional[Tuple[int, int, int]] = None, inplace: bool = False,
                check: bool = True) -> LabelledBatch:
    """What ``Collator.encode`` does between the tokenizer call and the vocabulary (collator.py:180-205), on the device: the inner
    collator, then ``byte_lengths`` and ``metrics`` on the ids it left.

    input_ids: ``[B, S]`` int32 / int64 on the device, unit column stride, any row stride >= S — the encoder's output with
    ``special_ids_map`` applied.  special_ids: the tokenizer's ``all_special_ids``, a host list of at most 256 ids of ``[0, V)``; a
    position is special when its id is in the list.  byte_lengths_per_token: ``[V]`` int32 / int64 on the device.  vocab_len =
    ``len(tokenizer)`` <= V: a random replacement is an id below it.

    loss="clm": ``labels = input_ids``, nothing is drawn.  loss="mlm" (needs mask_token_id): with p = b * S + j, ``key_i = mix64(seed +
    (i + 1) * 0x9E3779B97F4A7C15)``, ``h_i(p) = mix64(key_i ^ p)`` (mix64: the finalizer of splitmix64, arithmetic mod 2^64) and
    ``k_i = h_i >> 11``: masked = not special and ``k_0 < t_mask``; replaced = masked and ``k_1 < t_replace``; random = masked, not
    replaced and ``k_2 < t_random``; ``labels`` = the id where masked, else -100; the id becomes mask_token_id where replaced and
    ``h_3(p) mod vocab_len`` where random.  thresholds: ``mlm_thresholds(...)``, the defaults when None.  That is
    ``DataCollatorForLanguageModeling.numpy_mask_tokens`` with a generator whose ``binomial`` returns ``k_i * 2^-53 < p`` and whose
    ``integers`` returns the words of the selected positions in row-major order.

    ``metrics`` = (avg_byte_length, unk_ratio) = (sum of byte_lengths over non-special positions / their number, positions equal to
    unk_token_id / B * S), float64, on the ids after masking as in the reference.  Both are quotients of exact integers: numpy's
    ``mean`` bit for bit; no non-special position gives NaN, as numpy does.  unk_token_id=None counts nothing.

    ``record[7]`` has LABEL_BAD_ID (1) set when an id is outside ``[0, V)``; such an id is never an address, is never masked, counts as
    non-special with byte length 0.  check=True reads the record once and raises IndexError; check=False never waits for the host.
    inplace=True writes the masked ids into ``input_ids`` itself (a strided view is written through its stride).  Two launches, integer
    sums in a fixed order: the same inputs give the same bits.  Positions and ids are indexed with 32 bits: B * S and V above 0x7fffff00
    are a ValueError.  No gradient flows anywhere."""
    if loss not in _LOSSES:
        raise ValueError(f"loss must be \"clm\" or \"mlm\", got {loss!r}")
    ints = (torch.int32, torch.int64)
    if not isinstance(input_ids, torch.Tensor) or input_ids.dtype not in ints or input_ids.dim() != 2 or input_ids.numel() == 0:
        raise ValueError("input_ids must be a non-empty [B, S] int32 / int64 tensor")
    if not input_ids.is_cuda:
        raise ValueError("zett_amd computes on the GPU only: input_ids must be a cuda (ROCm) tensor; there is no CPU path")
    b, s = input_ids.shape
    if s > 1 and input_ids.stride(1) != 1 or b > 1 and input_ids.stride(0) < s:
        raise ValueError("input_ids needs unit column stride and a row stride >= S")
    table = byte_lengths_per_token
    if not isinstance(table, torch.Tensor) or table.dtype not in ints or table.dim() != 1 or table.numel() == 0 or table.device != input_ids.device:
        raise ValueError("byte_lengths_per_token must be a non-empty [V] int32 / int64 tensor on the device of input_ids")
    table = table.detach().contiguous()
    v = table.numel()
    vocab_len = int(vocab_len)
    if vocab_len < 1 or vocab_len > v:
        raise ValueError(f"vocab_len = {vocab_len} must be in [1, V = {v}]")
    special = [int(x) for x in special_ids]
    if len(special) > _lib.SPLICE_MAX_ROWS:
        raise ValueError(f"special_ids holds {len(special)} entries, at most {_lib.SPLICE_MAX_ROWS} travel with a launch")
    bad = [x for x in special if x < 0 or x >= v]
    if bad:
        raise IndexError(f"special id {bad[0]} is outside [0, {v})")
    if loss == "mlm":
        if mask_token_id is None:
            raise ValueError("This tokenizer does not have a mask token which is necessary for masked language modeling.")
        if not 0 <= int(mask_token_id) < v:
            raise IndexError(f"mask_token_id {mask_token_id} is outside [0, {v})")
        t_mask, t_replace, t_random = (int(x) for x in (mlm_thresholds() if thresholds is None else thresholds))
        if min(t_mask, t_replace, t_random) < 0 or max(t_mask, t_replace, t_random) > 1 << 53:
            raise ValueError("a threshold is ceil(probability * 2^53): an integer of [0, 2^53]")
    else:
        t_mask = t_replace = t_random = 0
    unk = -1 if unk_token_id is None else int(unk_token_id)
    if unk < -1:
        raise ValueError("unk_token_id is an id or None")
    device = input_ids.device
    ids = input_ids.detach()
    ld_in = ids.stride(0) if b > 1 else max(s, ids.stride(0))
    with torch.cuda.device(device):
        out = ids if inplace else torch.empty((b, s), dtype=ids.dtype, device=device)
        ld_out = ld_in if inplace else s
        labels = torch.empty((b, s), dtype=ids.dtype, device=device)
        byte_lengths = torch.empty((b, s), dtype=torch.int64, device=device)
        record = torch.empty(8, dtype=torch.int64, device=device)
        metrics = torch.empty(2, dtype=torch.float64, device=device)
        work = torch.empty(_lib.LABEL_WORKSPACE_BYTES // 8, dtype=torch.int64, device=device)          # (released on return: the allocator reuses it in stream order)
        k = len(special)
        _lib.check(_lib.load().zett_op_label_batch(ptr(ids), ids.element_size(), ld_in, b, s, (C.c_int32 * max(k, 1))(*special), k, ptr(table), table.element_size(), v,
                                                   vocab_len, -1 if mask_token_id is None else int(mask_token_id), unk, _LOSSES[loss], t_mask, t_replace, t_random,
                                                   int(seed) & _MASK64, ptr(out), ld_out, ptr(labels), ptr(byte_lengths), ptr(record), ptr(metrics), ptr(work),
                                                   work.numel() * 8, stream(device)), "label_batch")
    if check and int(record[7].item()) & LABEL_BAD_ID:          # (the one host read of this call)
        raise IndexError(f"label_batch: an id of input_ids is outside [0, {v})")
    return LabelledBatch(input_ids if inplace else out, labels, byte_lengths, metrics, record)


class PaddedVocabulary(NamedTuple):
    """What ``pad_vocabulary`` returns, all on the device."""
    target_surface_forms: torch.Tensor       # [R, L], dtype of the input; zero rows behind V
    target_priors: torch.Tensor              # [R] fp32; -100000 behind V
    mask: torch.Tensor                       # [R] bool: row < V
    ids_to_embed: torch.Tensor               # [R] int64: arange(V), then zeros


def padded_rows(length: int, pad_to_multiple_of: int, tokenizer_sample_max: Optional[int] = None) -> int:
    """The row count of the padded vocabulary (collator.py:284-303): with tokenizer sampling ``tokenizer_sample_max +
    pad_to_multiple_of`` whatever the step's length is (the reference asserts that the first is a multiple of the second: ValueError
    here, and for a vocabulary that does not fit), otherwise ``length`` rounded up to a multiple of ``pad_to_multiple_of``."""
    length, m = int(length), int(pad_to_multiple_of)
    if m <= 0 or length <= 0:
        raise ValueError("length and pad_to_multiple_of must be positive")
    if tokenizer_sample_max is None:
        return -(-length // m) * m
    if int(tokenizer_sample_max) % m != 0:
        raise ValueError(f"tokenizer_sample_max = {tokenizer_sample_max} must be a multiple of pad_to_multiple_of = {m}")
    rows = int(tokenizer_sample_max) + m
    if rows < length:
        raise ValueError(f"a vocabulary of {length} rows does not fit tokenizer_sample_max + pad_to_multiple_of = {rows}")
    return rows


def pad_vocabulary(surface_forms, priors, n_rows: int) -> PaddedVocabulary:
    """The branch of ``Collator.encode`` without ``n_token_subsample`` (collator.py:283-337): the whole vocabulary padded to ``n_rows``
    rows (``padded_rows``), in one launch.  surface_forms: ``[V, L]`` int32 / int64 on the device, unit column stride, row stride >= L.
    priors: ``[V]`` float32 or float64 (``SampledVocabulary.priors`` is float64): a float64 prior is rounded once to float32, to nearest
    even, in the kernel — the reference's float64 priors reach the model as float32 too.  Rows behind V: zero surface forms, prior
    -100000, mask false, id 0.  At most 65 536 columns and 0x7fffff00 rows (ValueError beyond).  Nothing is read back; no gradient flows
    anywhere."""
    sf = surface_forms
    if not isinstance(sf, torch.Tensor) or sf.dim() != 2 or sf.dtype not in (torch.int32, torch.int64) or sf.shape[0] == 0 or sf.shape[1] == 0:
        raise ValueError("surface_forms must be a non-empty [V, L] int32 / int64 tensor")
    v, l = sf.shape
    if l > 1 and sf.stride(1) != 1 or v > 1 and sf.stride(0) < l:
        raise ValueError("surface_forms needs unit column stride and a row stride >= L")
    if not sf.is_cuda:
        raise ValueError("zett_amd computes on the GPU only: surface_forms must be a cuda (ROCm) tensor; there is no CPU path")
    if not isinstance(priors, torch.Tensor) or priors.dtype not in (torch.float32, torch.float64) or priors.shape != (v,) or priors.device != sf.device:
        raise ValueError(f"priors must be a float32 / float64 [{v}] tensor on the device of surface_forms")
    r = int(n_rows)
    if r < v:
        raise ValueError(f"n_rows = {r} is less than the vocabulary's {v} rows")
    sf, priors = sf.detach(), priors.detach().contiguous()
    device = sf.device
    with torch.cuda.device(device):
        out_sf = torch.empty((r, l), dtype=sf.dtype, device=device)
        out_priors = torch.empty(r, dtype=torch.float32, device=device)
        mask = torch.empty(r, dtype=torch.bool, device=device)
        ids_to_embed = torch.empty(r, dtype=torch.int64, device=device)
        _lib.check(_lib.load().zett_op_pad_vocabulary(ptr(sf), sf.element_size(), sf.stride(0) if v > 1 else max(l, sf.stride(0)), l, v, r, ptr(priors),
                                                      priors.element_size(), ptr(out_sf), ptr(out_priors), ptr(mask), ptr(ids_to_embed), stream(device)),
                   "pad_vocabulary")
    return PaddedVocabulary(out_sf, out_priors, mask, ids_to_embed)


# ---- Collator.__call__ (collator.py:454-537) ----------------------------------------------------------------------------------------------------
def _mix64(x: int) -> int:
    x &= _MASK64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK64
    return x ^ (x >> 31)


def derived_seed(seed: int, stream: int) -> int:
    """The 64-bit seed of stream 0 (labels), 1 (the tokenizer sampler), 2 (negative_order), 3 (the identity batch) of a call's ``seed``."""
    return _mix64(_mix64(int(seed)) + (int(stream) + 1) * _GOLDEN)


class DeviceCollator:
    """The reference's ``Collator`` with a device behind it: ``__call__`` returns the reference's dict — ``input_ids``, ``attention_mask``,
    ``labels``, ``metrics``, ``byte_lengths``, ``target_priors``, ``target_surface_forms``, ``mask``, ``ids_to_embed``, ``special_indices``,
    ``special_indices_in_reference``, ``lang_code``, ``lang_index`` — with device tensors for the arrays (``metrics``: a dict of two 0-dim
    float64 tensors), host lists for the two special-index lists and a 0-dim HOST tensor for ``lang_index`` (the hypernetwork's forward
    reads it as a Python integer).  Two more keys carry what ``check=False`` leaves unread:
    ``label_record`` ([8] int64) and ``vocab_status`` (the status word of ``subsample_batch_vocabulary``, or None).

    It only orders existing pieces: the text span cut (host, drawn from ``rng``); ``sample_tokenizer_device`` (``n_total``, ``noise_std`` and
    the sampler index drawn from ``rng`` as ``Collator.sample_tokenizer`` draws them) or the fixed tokenizer's ``DeviceTextEncoder`` with
    surface forms, scores and byte lengths prepared once as ``Collator.__init__`` prepares them; the encoder; ``label_batch``;
    ``subsample_batch_vocabulary`` or ``pad_vocabulary``.

    reference, hn_tokenizer, data_args: as the reference's.  ``tokenizer``: the LOADED tokenizer that ``tokenizer_name`` would name (given
    exactly when ``data_args.do_tokenizer_sampling`` is false).  ``samplers``: ``{lang_code: [DeviceTokenizerSampler, ...]}``, warmed up
    by the caller as ``Collator.__init__`` does with ``initial_texts``.  loss: "clm" or "mlm" — the reference's ``inner_collator`` is None or
    ``DataCollatorForLanguageModeling``; ``mlm_probabilities`` are the latter's three.

    The device randomness all derives from ``seed`` (``derived_seed``): the label seed, the sampler seed, and ``negative_order`` /
    the identity batch's indices, which are ``torch.randperm`` with a device ``torch.Generator`` seeded from it (``negative_order(seed, v)``) — plumbing, not a kernel of
    this library.  The host draws come from ``rng`` (a ``numpy.random.Generator``; ``default_rng(seed)`` when None).  The same ``(data,
    seed, rng state)`` gives the same bits.

    Deviations from the reference: the generators (numpy's global one there); what ``subsample_batch_vocabulary`` documents (a label of
    -100 is not an id; no duplicate negatives); ``target_priors`` are float32 (they reach the model as float32 there too).  What the pieces
    refuse stays refused; ``use_passthrough_hypernet`` and ``subsample_mode="highest_scores"`` raise NotImplementedError.  With
    check=False no piece reads anything back except ``DeviceSampledVocabulary.build``, whose one read of its record sizes the step."""

    def __init__(self, reference, hn_tokenizer, data_args, *, loss: str, tokenizer=None, samplers=None, is_validation: bool = False, lang_code: Optional[str] = None,
                 device=None, mlm_probabilities: Tuple[float, float, float] = (0.15, 0.8, 0.1)):
        if loss not in _LOSSES:
            raise ValueError(f"loss must be \"clm\" or \"mlm\", got {loss!r}")
        a = data_args
        if getattr(a, "use_passthrough_hypernet", False):
            raise NotImplementedError("use_passthrough_hypernet")
        self.n_token_subsample = getattr(a, "n_token_subsample", None)
        if self.n_token_subsample is not None:
            if a.subsample_mode == "highest_scores":
                raise NotImplementedError("subsample_mode=\"highest_scores\" (the reference raises here too)")
            if a.subsample_mode not in ("random", "positives_only"):
                raise ValueError(f"unknown subsample_mode {a.subsample_mode!r}")
            if self.n_token_subsample % a.pad_to_multiple_of != 0:
                raise ValueError("n_token_subsample must be a multiple of pad_to_multiple_of")
        elif a.do_tokenizer_sampling:
            padded_rows(1, a.pad_to_multiple_of, a.tokenizer_sample_max)          # (the reference's assert, once)
        if (tokenizer is None) != bool(a.do_tokenizer_sampling):
            raise ValueError("a tokenizer is given exactly when data_args.do_tokenizer_sampling is false")
        self.device = default_device(device)
        self.reference, self.hn_tokenizer, self.data_args, self.loss = reference, hn_tokenizer, a, loss
        self.is_validation, self.lang_code = bool(is_validation), lang_code
        self.thresholds = mlm_thresholds(*mlm_probabilities) if loss == "mlm" else None
        if loss == "mlm" and reference.mask_token is None:
            raise ValueError("This tokenizer does not have a mask token which is necessary for masked language modeling.")
        self.special_tokens = list(reference.all_special_tokens)
        self.special_indices_in_reference = [int(reference.convert_tokens_to_ids(t)) for t in self.special_tokens]
        self.samplers = dict(samplers or {})
        if a.do_tokenizer_sampling:
            from .sampled_vocab import DeviceSampledVocabulary
            self.vocabulary = DeviceSampledVocabulary(reference, a.add_prefix_space, hn_tokenizer=hn_tokenizer,
                                                      hn_surface_maxlen=a.hn_surface_maxlen if hn_tokenizer is not None else None,
                                                      max_vocab=int(a.tokenizer_sample_max) + 256, device=self.device)
            return
        from tokenizers import decoders, pre_tokenizers

        from .byte_level import convert_to_byte_level
        from .surface_forms import surface_form_matrix_device
        from .text_encode import DeviceTextEncoder
        self.original_length = len(tokenizer)
        tokenizer = convert_to_byte_level(tokenizer, match_special_tokens_to=reference, make_whitespace_consistent=True)[0]
        tokenizer._tokenizer.pre_tokenizer = pre_tokenizers.ByteLevel(use_regex=True, add_prefix_space=a.add_prefix_space)          # (assume consistent pretokenizer)
        tokenizer._tokenizer.decoder = decoders.ByteLevel()
        if list(tokenizer.all_special_tokens) != self.special_tokens:
            raise ValueError("the tokenizer's special tokens are not the reference's")
        self.tokenizer = tokenizer
        self.encoder = DeviceTextEncoder.from_tokenizer(tokenizer, self.device, split_added_tokens=True)          # (packed texts hold the eos string)
        v = len(tokenizer)
        tokens = tokenizer.convert_ids_to_tokens(range(v))
        import numpy as np
        with torch.cuda.device(self.device):
            if hn_tokenizer is None or hn_tokenizer.get_vocab() == tokenizer.get_vocab():
                self.surface_forms = torch.arange(v, dtype=torch.int64, device=self.device)[:, None]
            else:
                self.surface_forms = surface_form_matrix_device(tokens, a.hn_surface_maxlen, hn_tokenizer, self.device)[0]
            model = tokenizer._tokenizer.model
            scores = list(model.get_scores()) if hasattr(model, "get_scores") else []          # (no installed model has it; the reference asks the same way)
            scores = np.array(scores + [0.0] * (v - len(scores)), dtype=np.float64)
            self.scores = torch.from_numpy(scores).to(self.device)
            self.scores_f32 = self.scores.float()
            self.byte_lengths = torch.tensor([len(x) for x in tokens], dtype=torch.int64, device=self.device)
        self.special_ids = [int(i) for i in tokenizer.all_special_ids]
        self.mask_token_id, self.unk_token_id = tokenizer.mask_token_id, tokenizer.unk_token_id

    def _permutation(self, n: int, seed: int, stream: int) -> torch.Tensor:
        g = torch.Generator(device=self.device)
        g.manual_seed(derived_seed(seed, stream) >> 1)
        with torch.cuda.device(self.device):
            return torch.randperm(int(n), generator=g, device=self.device)

    def negative_order(self, seed: int, v: int) -> torch.Tensor:
        """The permutation of ``range(v)`` that a call with this ``seed`` hands to ``subsample_batch_vocabulary(mode="random")``: a pure
        function of ``(seed, v)`` on this device (``torch.randperm`` with a device generator: plumbing)."""
        return self._permutation(v, seed, 2)

    def _lang(self, lang_code):
        """0-dim int64 on the HOST, as the reference's ``np.array``: ``ZettHypernet.forward`` reads it as a Python integer, and a device
        scalar there would be a wait for the host in every step."""
        return torch.tensor(self.data_args.langs.index(lang_code) if lang_code is not None else 0, dtype=torch.int64)

    def identity_batch(self, seed: int) -> Dict:
        """``for_identity_step=True``: ``n_token_subsample`` distinct rows of the ORIGINAL vocabulary, uniformly — the first entries of a
        device permutation —, their surface forms (rows copied bit for bit by ``token_embeddings``'s lookup kernel) and zero priors."""
        if self.data_args.do_tokenizer_sampling:
            raise ValueError("the identity batch needs the fixed tokenizer (the reference's Collator has no original_length otherwise)")
        if self.n_token_subsample is None:
            raise ValueError("the identity batch holds n_token_subsample rows: data_args.n_token_subsample is None")
        from .training import token_embeddings
        n = int(self.n_token_subsample)
        if n > self.original_length:
            raise ValueError(f"n_token_subsample = {n} distinct rows cannot be drawn from the original vocabulary's {self.original_length}")
        with torch.cuda.device(self.device):
            indices = self._permutation(self.original_length, seed, 3)[:n].contiguous()
            sf = self.surface_forms.contiguous()
            rows = token_embeddings(sf.view(torch.float32), indices, check_ids=False).view(sf.dtype)
            return {"target_surface_forms": rows, "target_priors": torch.zeros(n, dtype=torch.float32, device=self.device), "ids_to_embed": indices,
                    "lang_code": self.lang_code, "lang_index": self._lang(self.lang_code)}

    def __call__(self, data, for_identity_step: bool = False, *, seed: int, rng=None, check: bool = True) -> Dict:
        import numpy as np
        a = self.data_args
        if for_identity_step:
            return self.identity_batch(seed)
        rng = np.random.default_rng(int(seed) & _MASK64) if rng is None else rng
        if "texts" in data[0]:
            examples, lang_code = [{"text": text} for text in data[0]["texts"]], data[0]["lang_code"]
        else:
            examples, lang_code = data, None
        if self.lang_code is not None:
            lang_code = self.lang_code
        max_length = MAX_CHARS_PER_TOKEN * a.block_size
        texts = []
        for e in examples:
            start = int(rng.integers(0, max(len(e["text"]) - max_length, 0) + 1)) if a.sample_text_span else 0
            texts.append(e["text"][start:start + max_length])
        if a.do_tokenizer_sampling:
            from .sampled_vocab import sample_tokenizer_device
            samplers = self.samplers[lang_code]
            sampler = samplers[int(rng.integers(0, len(samplers)))]
            n_total = int(rng.normal(a.tokenizer_sample_mean, a.tokenizer_sample_std))
            n_total = min(a.tokenizer_sample_max, max(a.tokenizer_sample_min, n_total))
            noise_std = float(rng.lognormal(mean=math.log(a.tokenizer_noise_mean), sigma=a.tokenizer_noise_std)) if a.tokenizer_noise_mean > 0 else 0.0
            encoder, special_ids_map, surface_forms, priors, byte_lengths = sample_tokenizer_device(
                texts, sampler, self.vocabulary, n_total=n_total, noise_std=noise_std, is_validation=self.is_validation, seed=derived_seed(seed, 1), check=check)
            if surface_forms is None:          # (no hn tokenizer: the reference hands None on and fails at len(); here the rows' own numbers, as for a fixed tokenizer)
                surface_forms = torch.arange(priors.shape[0], dtype=torch.int64, device=self.device)[:, None]
            place = lambda i: None if i is None else int(special_ids_map.get(int(i), int(i)))          # noqa: E731
            special_ids = [place(self.reference.convert_tokens_to_ids(t)) for t in self.special_tokens]
            mask_token_id, unk_token_id = place(self.reference.mask_token_id), place(self.reference.unk_token_id)
            priors_f32 = None
        else:
            encoder, special_ids_map = self.encoder, {}
            surface_forms, priors, priors_f32, byte_lengths = self.surface_forms, self.scores, self.scores_f32, self.byte_lengths
            special_ids, mask_token_id, unk_token_id = self.special_ids, self.mask_token_id, self.unk_token_id
        v = int(priors.shape[0])
        if surface_forms.shape[0] != v:
            raise ValueError("the surface forms and the priors have different lengths")
        enc = encoder(texts, a.block_size, special_ids_map, check=check)
        lb = label_batch(enc["input_ids"], special_ids, byte_lengths, vocab_len=v, loss=self.loss, mask_token_id=mask_token_id, unk_token_id=unk_token_id,
                         seed=derived_seed(seed, 0), thresholds=self.thresholds, inplace=True, check=check)
        out = {"input_ids": lb.input_ids, "attention_mask": enc["attention_mask"], "labels": lb.labels,
               "metrics": {"avg_byte_length": lb.metrics[0], "unk_ratio": lb.metrics[1]}, "byte_lengths": lb.byte_lengths, "label_record": lb.record,
               "vocab_status": None}
        if self.n_token_subsample is not None:
            from .training import subsample_batch_vocabulary
            order = None
            with torch.cuda.device(self.device):
                if a.subsample_mode == "random":
                    order = self.negative_order(seed, v)
                if priors_f32 is None:
                    priors_f32 = priors.float()
            bv = subsample_batch_vocabulary(lb.input_ids, lb.labels, special_ids, self.n_token_subsample, surface_forms, priors_f32, mode=a.subsample_mode,
                                            negative_order=order, check=check)
            out.update(input_ids=bv.input_ids, labels=bv.labels, target_priors=bv.target_priors, target_surface_forms=bv.target_surface_forms, mask=bv.mask,
                       ids_to_embed=bv.ids_to_embed, special_indices=bv.special_indices, vocab_status=bv.status)
        else:
            pv = pad_vocabulary(surface_forms, priors, padded_rows(v, a.pad_to_multiple_of, a.tokenizer_sample_max if a.do_tokenizer_sampling else None))
            out.update(target_priors=pv.target_priors, target_surface_forms=pv.target_surface_forms, mask=pv.mask, ids_to_embed=pv.ids_to_embed,
                       special_indices=list(special_ids))
        out["special_indices_in_reference"] = list(self.special_indices_in_reference)
        out["lang_code"] = lang_code
        out["lang_index"] = self._lang(lang_code)
        return out
