"""Lexical (FVT / BFVT) embedding transfer on MI355X — the surface of the reference's scripts/transfer_lexical.py.

    python scripts/transfer_lexical.py --output out/ --tokenizer_name <target tokenizer> \
        --model_name_or_path <LM> --model_class AutoModelForCausalLM --fvt_mode fvt

Every target token gets the source model's embedding row of the same string where the source vocabulary has one, else the
mean of the rows of its decomposition under the source tokenizer (``fvt`` / ``bfvt``), else a fallback row
(scripts/transfer_lexical.py:50-91).  The reference's per-token Python loop — one ``model.tokenize`` and one ``torch.mean`` per
token — is three stages behind the C ABI (include/zett_hip.h, zett_amd/csrc/lexical.hip):

    LexicalTransfer(source_tokenizer, device)      the lexicon: bare model + the whole get_vocab() as a device hash table
    .plan(tokens, n_source_rows, fvt_mode)         one retokenization + lookup + mode filter  -> ids, count, overlap
    .rows_into(plan, source_in, ...)               one streaming gather-mean kernel into the destination matrices

The mean is defined as: add the rows in ids order in fp32, then one IEEE division by float(n).  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from ._glue import ptr, stream, zett_dtypes
from .surface_forms import CHARS_TO_BYTES, HnTokenizerSpec, _raw

FVT_MODES = {"no": _lib.LEXICAL_NO, "fvt": _lib.LEXICAL_FVT, "bfvt": _lib.LEXICAL_BFVT}
FALLBACK_MODES = ("unk", "random")
DEFAULT_WIDTH = 16          # ids per row of the first plan; rows that need more are planned again at the width they need
RANDOM_BLOCK_ROWS = 1024    # rows per draw of fallback_mode="random" (bounds host memory; the stream is that of one whole draw)
_NO_CPU = "zett_amd computes on MI355X only: pass a cuda (ROCm) device / cuda tensors; there is no CPU path"


@dataclass
class Args:
    """scripts/transfer_lexical.py:13-21, same names and defaults."""
    output: str
    tokenizer_name: str
    model_name_or_path: str = "FacebookAI/xlm-roberta-base"
    model_class: str = "AutoModelForMaskedLM"
    fvt_mode: str = "no"  # "fvt", "bfvt"
    fallback_mode: str = "unk"  # "random", "unk"
    save_flax: bool = False


@dataclass
class LexicalPlan:
    """What every target row is a mean of (zett_lexical_plan): ``ids[i, :count[i]]`` source rows, ``count[i] == 0`` = fallback."""
    ids: torch.Tensor            # int32 [n_tokens, width] on the device
    count: torch.Tensor          # int32 [n_tokens] on the device
    overlap: int                 # rows with count > 0: the reference's "Overlapping tokens"
    n_ids: int                   # sum of the counts
    n_source_rows: int
    fvt_mode: str
    n_replanned: int = 0         # rows whose decomposition did not fit the first width

    @property
    def n_tokens(self) -> int:
        return int(self.count.shape[0])

    @property
    def width(self) -> int:
        return int(self.ids.shape[1])


def _require_cuda(*tensors) -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(_NO_CPU)


def _rows_view(t: torch.Tensor, what: str):
    """(pointer, leading dimension in elements) of a 2-D tensor whose rows are contiguous."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise ValueError(f"{what}: a 2-D tensor with contiguous rows is required")
    return t.data_ptr(), int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), int(t.shape[1]))


class LexicalTransfer:
    """A ``zett_lexical`` handle: the source tokenizer's lexicon resident on one GPU."""

    def __init__(self, source_tokenizer, device, vocab: Optional[Dict[str, int]] = None, unk_token_id: Optional[int] = None):
        """``source_tokenizer``: a (byte-level) transformers fast tokenizer, or an ``HnTokenizerSpec`` of its bare model together
        with ``vocab`` (its whole ``get_vocab()``) and ``unk_token_id``."""
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(_NO_CPU)
        self.lib = _lib.load()
        self.device = device
        if isinstance(source_tokenizer, HnTokenizerSpec):
            spec = source_tokenizer
            if vocab is None:
                raise ValueError("an HnTokenizerSpec needs the tokenizer's whole vocabulary (vocab=...)")
        else:
            # the BARE model (scripts/transfer_lexical.py:77): no special token is matched by string
            model = json.loads(source_tokenizer._tokenizer.to_str())["model"]
            spec = HnTokenizerSpec.from_model_json(model, (), (), -1)
            vocab = source_tokenizer.get_vocab() if vocab is None else vocab
            unk_token_id = source_tokenizer.unk_token_id if unk_token_id is None else unk_token_id
        self.spec = spec
        self.unk_token_id = unk_token_id
        # get_vocab() whole, added and special tokens included (:50, :69); an entry with a character outside the byte table can
        # never equal a byte-level token
        entries = [(r, int(i)) for r, i in ((_raw(s), i) for s, i in vocab.items()) if r]
        vb, vo = HnTokenizerSpec._pack([r for r, _ in entries])
        vi = np.asarray([i for _, i in entries], dtype=np.int32)

        def host_ptr(a):
            return None if a is None else a.ctypes.data_as(C.c_void_p)

        m = _lib.ZettRetokModel(
            kind=spec.kind, n_pieces=len(spec.piece_ids), piece_bytes=host_ptr(spec.piece_bytes),
            piece_offsets=host_ptr(spec.piece_offsets), piece_ids=host_ptr(spec.piece_ids), piece_scores=host_ptr(spec.piece_scores),
            unigram_min_score=spec.unigram_min_score, n_merges=len(spec.merges), merges=host_ptr(spec.merges),
            unk_id=spec.unk_id, fuse_unk=int(spec.fuse_unk), byte_fallback=int(spec.byte_fallback),
            byte_fallback_ids=host_ptr(spec.byte_fallback_ids), ignore_merges=int(spec.ignore_merges),
            n_special=0, special_bytes=None, special_offsets=None, special_ids=None,
            piece_continuing=host_ptr(spec.piece_continuing), max_input_chars_per_word=int(spec.max_input_chars_per_word))
        handle = C.c_void_p()
        index = device.index if device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", index)
        _lib.check(self.lib.zett_lexical_create(C.byref(m), len(entries), host_ptr(vb), host_ptr(vo), host_ptr(vi), index, C.byref(handle)), "zett_lexical_create")
        self.handle = handle

    # ---- stage 2 ---------------------------------------------------------------------------------------------------
    def _plan_call(self, tokens: Sequence[str], n_source_rows: int, mode: int, width: int):
        n = len(tokens)
        blob = "\0".join(tokens).encode("utf-8")
        if blob.count(b"\0") != n - 1:
            bad = next(i for i, t in enumerate(tokens) if "\0" in t)
            raise KeyError(f"token {bad} ({tokens[bad]!r}) holds a NUL: a character outside the byte-level table")
        if len(blob) >= 2 ** 31 - 1:
            raise ValueError("more than 2 GiB of token text in one call")
        ids = torch.empty((n, width), dtype=torch.int32, device=self.device)
        count = torch.empty((n,), dtype=torch.int32, device=self.device)
        overlap, wide, n_ids, bad = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(-1)
        with torch.cuda.device(self.device):
            text = torch.from_numpy(np.frombuffer(blob or b"\0", dtype=np.uint8).copy()).to(self.device)
            rc = self.lib.zett_lexical_plan(self.handle, ptr(text), n, len(blob), int(n_source_rows), mode, int(width), ptr(ids), ptr(count),
                                            C.byref(overlap), C.byref(wide), C.byref(n_ids), C.byref(bad), stream(self.device))
        if rc == _lib.E_KEY and 0 <= bad.value < n:
            token = tokens[bad.value]
            chars = [ch for ch in token if ch not in CHARS_TO_BYTES]
            raise KeyError(f"token {bad.value} ({token!r}) holds a character outside the byte-level table: {chars[:1]!r}")
        if rc == _lib.E_STATE:
            raise Exception(self.lib.zett_last_error().decode())      # tokenizers raises a bare Exception here
        _lib.check(rc, "zett_lexical_plan")
        return ids, count, int(overlap.value), int(wide.value), int(n_ids.value)

    def plan(self, tokens_or_tokenizer, n_source_rows: int, fvt_mode: str = "no", width: int = DEFAULT_WIDTH) -> LexicalPlan:
        """scripts/transfer_lexical.py:65-91 without the arithmetic.  ``n_source_rows`` is the source MATRIX's row count (the
        reference's ``len(source_embeddings)``), not the tokenizer's length."""
        if fvt_mode not in FVT_MODES:
            raise ValueError(f"fvt_mode {fvt_mode!r}: expected one of {sorted(FVT_MODES)}")
        if isinstance(tokens_or_tokenizer, (list, tuple)):
            tokens = list(tokens_or_tokenizer)
        else:
            tokens = tokens_or_tokenizer.convert_ids_to_tokens(range(len(tokens_or_tokenizer)))      # :68
        mode = FVT_MODES[fvt_mode]
        n = len(tokens)
        if n == 0:
            return LexicalPlan(torch.empty((0, width), dtype=torch.int32, device=self.device),
                               torch.empty((0,), dtype=torch.int32, device=self.device), 0, 0, int(n_source_rows), fvt_mode)
        ids, count, overlap, wide, n_ids = self._plan_call(tokens, n_source_rows, mode, width)
        if wide:
            # the rows whose decomposition did not fit: planned again, alone, at the width the longest of them needs — no
            # decomposition is ever cut.  Their counts are already the true ones.
            rows = torch.nonzero(count > width).flatten()
            need = int(count.index_select(0, rows).max().item())
            host_rows = rows.cpu().tolist()
            ids2, count2, _, wide2, _ = self._plan_call([tokens[i] for i in host_rows], n_source_rows, mode, need)
            assert wide2 == 0 and torch.equal(count2, count.index_select(0, rows))
            grown = torch.full((n, need), -1, dtype=torch.int32, device=self.device)
            grown[:, :width] = ids
            grown[rows] = ids2
            ids = grown
        return LexicalPlan(ids, count, overlap, n_ids, int(n_source_rows), fvt_mode, n_replanned=wide)

    # ---- stage 3 ---------------------------------------------------------------------------------------------------
    def _rows_call(self, plan: LexicalPlan, source_in, source_out, fallback_id: int, dest_in, dest_out, rows) -> None:
        _require_cuda(plan.ids, plan.count, source_in, source_out, dest_in, dest_out, rows)
        if source_in.dtype not in zett_dtypes():
            raise ValueError(f"source dtype {source_in.dtype}: float32, float16 or bfloat16")
        if dest_in.dtype not in zett_dtypes():
            raise ValueError(f"destination dtype {dest_in.dtype}: float32, float16 or bfloat16")
        if (source_out is None) != (dest_out is None):
            raise ValueError("source_out and dest_out go together (untied embeddings) or are both None (tied)")
        if source_out is not None and (source_out.dtype != source_in.dtype or source_out.shape != source_in.shape):
            raise ValueError("source_out must have source_in's dtype and shape")
        if dest_out is not None and (dest_out.dtype != dest_in.dtype or dest_out.shape != dest_in.shape):
            raise ValueError("dest_out must have dest_in's dtype and shape")
        if int(source_in.shape[0]) != plan.n_source_rows:
            raise ValueError(f"the plan was made for {plan.n_source_rows} source rows, the matrix has {source_in.shape[0]}")
        n_embd = int(source_in.shape[1])
        if int(dest_in.shape[1]) != n_embd:
            raise ValueError(f"destination rows have {dest_in.shape[1]} columns, source rows {n_embd}")
        p_si, ld_si = _rows_view(source_in, "source_in")
        p_so, ld_so = _rows_view(source_out, "source_out") if source_out is not None else (0, 0)
        p_di, ld_di = _rows_view(dest_in, "dest_in")
        p_do, ld_do = _rows_view(dest_out, "dest_out") if dest_out is not None else (0, 0)
        if rows is not None:
            if rows.dtype != torch.int64 or rows.shape != (plan.n_tokens,):
                raise ValueError("rows: an int64 tensor with one destination row per planned token")
            rows = rows.contiguous()
        ids = plan.ids.contiguous()
        d = _lib.ZettDest(in_=p_di, out=p_do or None, bias=None, dtype=zett_dtypes()[dest_in.dtype], bias_dtype=_lib.DTYPE_F32, ld_in=ld_di, ld_out=ld_do,
                          rows=rows.data_ptr() if rows is not None else None, n_dest_rows=int(dest_in.shape[0]))
        with torch.cuda.device(self.device):
            rc = self.lib.zett_lexical_rows_into(self.handle, ptr(ids), ptr(plan.count), plan.n_tokens, plan.width,
                                                 C.c_void_p(p_si), ld_si, C.c_void_p(p_so or None), ld_so, zett_dtypes()[source_in.dtype], plan.n_source_rows,
                                                 n_embd, int(fallback_id), C.byref(d), stream(self.device))
        _lib.check(rc, "zett_lexical_rows_into")

    def rows_into(self, plan: LexicalPlan, source_in: torch.Tensor, source_out: Optional[torch.Tensor] = None, fallback_mode: str = "unk",
                  dest_in: torch.Tensor = None, dest_out: Optional[torch.Tensor] = None, rows: Optional[torch.Tensor] = None,
                  unk_token_id: Optional[int] = None) -> None:
        """The arithmetic of scripts/transfer_lexical.py:50-63, 75, 84, 91, 97-104: row ``rows[i]`` (None: ``i``; < 0: skipped) of
        ``dest_in`` / ``dest_out`` from ``source_in`` / ``source_out`` ([R, E] each; the reference's ``cat`` is never made), stored in
        the destination's dtype.  ``fallback_mode="unk"``: rows without constituents get source row ``unk_token_id`` (default: the
        source tokenizer's); ``"random"``: they get draws of ``np.random.normal(S.mean(0), S.std(0))`` from numpy's global
        generator, consumed as the reference's single whole-matrix draw consumes it."""
        if dest_in is None:
            raise ValueError("dest_in is required")
        _require_cuda(source_in, source_out, dest_in, dest_out, rows)
        if fallback_mode not in FALLBACK_MODES:
            raise ValueError(f"fallback_mode {fallback_mode!r}: expected one of {list(FALLBACK_MODES)}")
        if fallback_mode == "unk":
            unk = self.unk_token_id if unk_token_id is None else unk_token_id
            if unk is None:
                raise ValueError('fallback_mode="unk" needs a source tokenizer with an unk_token_id (it has none): use fallback_mode="random"')
            self._rows_call(plan, source_in, source_out, int(unk), dest_in, dest_out, rows)
            return
        # the rows of the plan go first: ZETT_E_INDEX is raised before anything is written
        self._rows_call(plan, source_in, source_out, -1, dest_in, dest_out, rows)
        self._random_fallback(plan, source_in, source_out, dest_in, dest_out, rows)

    def _random_fallback(self, plan, source_in, source_out, dest_in, dest_out, rows) -> None:
        """scripts/transfer_lexical.py:52-57.  loc / scale are a host-side statistic of the source matrix, computed with torch on
        the CPU exactly as the reference computes them (so they are its bits); the draws cover ALL target rows in order, in
        blocks, and only the rows whose count is 0 are uploaded."""
        S = source_in.detach().cpu() if source_out is None else torch.cat([source_in.detach().cpu(), source_out.detach().cpu()], dim=1)
        loc, scale = S.mean(0), S.std(0)
        E = int(source_in.shape[1])
        empty = (plan.count == 0).cpu().numpy()
        dest_rows = None if rows is None else rows.cpu().numpy()
        for r0 in range(0, plan.n_tokens, RANDOM_BLOCK_ROWS):
            r1 = min(plan.n_tokens, r0 + RANDOM_BLOCK_ROWS)
            draw = np.random.normal(loc=loc, scale=scale, size=(r1 - r0, S.shape[1]))
            pick = np.flatnonzero(empty[r0:r1])
            if dest_rows is not None:
                pick = pick[dest_rows[r0 + pick] >= 0]
            if len(pick) == 0:
                continue
            index = torch.from_numpy((r0 + pick) if dest_rows is None else dest_rows[r0 + pick]).to(self.device)
            block = torch.from_numpy(draw[pick]).to(torch.float32).to(self.device)        # float32(float64 draw), as weight.data[:] = from_numpy(...)
            dest_in[index] = block[:, :E].to(dest_in.dtype)
            if dest_out is not None:
                dest_out[index] = block[:, E:].to(dest_out.dtype)

    def close(self) -> None:
        if getattr(self, "handle", None):
            self.lib.zett_lexical_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def lexical_embeddings(source_tokenizer, tokens_or_tokenizer, source_in: torch.Tensor, source_out: Optional[torch.Tensor] = None,
                       fvt_mode: str = "no", fallback_mode: str = "unk", vocab: Optional[Dict[str, int]] = None, unk_token_id: Optional[int] = None):
    """One call: fp32 ``(target_in, target_out or None, overlap)`` for the target tokens, on ``source_in``'s device."""
    _require_cuda(source_in, source_out)
    lt = LexicalTransfer(source_tokenizer, source_in.device, vocab=vocab, unk_token_id=unk_token_id)
    try:
        plan = lt.plan(tokens_or_tokenizer, int(source_in.shape[0]), fvt_mode)
        out_in = torch.empty((plan.n_tokens, source_in.shape[1]), dtype=torch.float32, device=source_in.device)
        out_out = None if source_out is None else torch.empty_like(out_in)
        lt.rows_into(plan, source_in, source_out, fallback_mode, dest_in=out_in, dest_out=out_out)
        torch.cuda.synchronize(source_in.device)
    finally:
        lt.close()
    return out_in, out_out, plan.overlap


def main(argv=None):
    import transformers
    from transformers import AutoTokenizer, HfArgumentParser

    import zett_amd
    from zett_amd.byte_level import convert_to_byte_level

    (args,) = HfArgumentParser([Args]).parse_args_into_dataclasses(argv)
    if args.save_flax:
        raise NotImplementedError("--save_flax: this package has no Flax; convert the saved PyTorch model where Flax is installed")
    if args.fvt_mode not in FVT_MODES:
        raise ValueError(f"--fvt_mode {args.fvt_mode!r}: expected one of {sorted(FVT_MODES)}")
    if args.fallback_mode not in FALLBACK_MODES:
        raise ValueError(f"--fallback_mode {args.fallback_mode!r}: expected one of {list(FALLBACK_MODES)}")
    if int(os.environ.get("WORLD_SIZE", "1")) > 1 and int(os.environ.get("RANK", "0")) != 0:
        print(f"scripts/transfer_lexical.py: rank {os.environ.get('RANK')} has nothing to do (the lexical transfer runs in one process)")
        return
    zett_amd.configure_hw_queues()
    if not torch.cuda.is_available():
        raise SystemExit("scripts/transfer_lexical.py needs an MI355X: torch.cuda.is_available() is False")
    device = torch.device("cuda", torch.cuda.current_device())

    source_tokenizer = convert_to_byte_level(AutoTokenizer.from_pretrained(args.model_name_or_path))[0]                 # :27-29
    target_tokenizer = convert_to_byte_level(AutoTokenizer.from_pretrained(args.tokenizer_name), match_special_tokens_to=source_tokenizer,
                                             make_whitespace_consistent=True)[0]                                        # :30-34
    if args.fallback_mode == "unk" and source_tokenizer.unk_token_id is None:
        raise ValueError('--fallback_mode unk: the source tokenizer has no unk_token_id; pass --fallback_mode random')
    source_model = getattr(transformers, args.model_class).from_pretrained(args.model_name_or_path)                      # :36-38
    tied = bool(source_model.config.tie_word_embeddings)
    source_in = source_model.get_input_embeddings().weight.data.to(device)                                              # :39-48
    source_out = None if tied else source_model.get_output_embeddings().weight.data.to(device)

    lt = LexicalTransfer(source_tokenizer, device)
    plan = lt.plan(target_tokenizer, int(source_in.shape[0]), args.fvt_mode)
    print(f"Overlapping tokens: {plan.overlap}/{len(target_tokenizer)}")                                                # :93
    source_model.resize_token_embeddings(len(target_tokenizer))                                                         # :94-95
    source_model.config.vocab_size = len(target_tokenizer)
    # straight into the resized weights, in the model's dtype: the rows are written on the device and copied back once
    w_in = source_model.get_input_embeddings().weight.data
    d_in = torch.empty(w_in.shape, dtype=w_in.dtype, device=device)
    d_out = None
    if not tied:
        w_out = source_model.get_output_embeddings().weight.data
        d_out = torch.empty(w_out.shape, dtype=w_out.dtype, device=device)
    lt.rows_into(plan, source_in, source_out, args.fallback_mode, dest_in=d_in, dest_out=d_out)
    w_in.copy_(d_in)                                                                                                    # :97-104
    if not tied:
        w_out.copy_(d_out)
    lt.close()

    source_model.save_pretrained(args.output)                                                                           # :106-110
    source_tokenizer.save_pretrained(args.output)  # to get tokenizer_config.json and other metadata
    target_tokenizer.save_pretrained(args.output)


if __name__ == "__main__":
    main()
