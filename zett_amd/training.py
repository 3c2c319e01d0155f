"""The hypernetwork side of the reference's trainer around the differentiable forward (zett_amd/autograd.py): the identity
warm-up loss (train.py:914-975), the lexical loss (train.py:1074-1141) and the parameter update of
``optax.chain(clip_by_global_norm(max_grad_norm), multi_transform({train: adamw | adafactor, freeze: set_to_zero}))`` (train.py:591-656).

    opt = HypernetAdamW(model, lr=6e-5)                      # or HypernetAdafactor(model, lr=3e-4), or make_optimizer(model, training_args)
    pred_in, pred_out, _ = model(ids, source_embeddings=src, lang_index=lang)       # model.train(), parameters require grad
    loss = identity_loss(pred_in, pred_out, src, ids_to_embed)
    loss.backward()
    opt.step(lr=schedule(step), zero_grad=True)

    loss, stats = lm_head_loss(hidden, pred_out, labels, attention_mask, mode="clm", vocab_mask=mask)      # the language-model loss (train.py:1039-1056)

    pred_in, pred_out = splice_special_rows(pred_in, pred_out, src, special_indices, special_indices_in_reference, inplace=True)      # train.py:1014-1030
    inputs_embeds = token_embeddings(pred_in, input_ids, dtype=torch.bfloat16)      # for a backbone that takes inputs_embeds; d pred_in comes back through it

    bv = subsample_batch_vocabulary(input_ids, labels, special_ids, n_token_subsample, surface_forms, priors, negative_order=perm)      # collator.py:207-282: what feeds all of the above

    init_hypernet_state(model, source_embeddings, example_surface_forms, pretrained_state=sd)      # once, before the first step: the Rescaler fit (column_moments, rescaler_fit) and the overlay of pretrained parameters (train.py:689-725)

Losses, update, splice, lookup, the batch's sub-vocabulary and the column moments behind the Rescaler fit are HIP kernels (csrc/train_dist.hip, csrc/train_step.hip, csrc/train_adafactor.hip, csrc/train_loss.hip, csrc/train_embed.hip, csrc/train_batch.hip, csrc/train_init.hip); torch holds the tensors and the tape.  Nothing in this module waits for
the host except ``last_step_stats()``, ``state_dict()``, ``token_embeddings(check_ids=True)`` and ``subsample_batch_vocabulary(check=True)`` (the model's forward in front of it still reads its id range back once per
step).  Results are bit-reproducible from run to run.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Mapping, NamedTuple, Optional, Sequence, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._glue import ptr, stream, zett_dtypes

_KINDS = {"mse": _lib.DIST_MSE, "rmse": _lib.DIST_RMSE, "huber": _lib.DIST_HUBER}


# ---- the three kernels of an embedding distance ---------------------------------------------------------------------------
def _dist_args(pred, src, col0, ids, ids_stride, mask, kind):
    if kind not in _KINDS:
        raise ValueError(f"kind must be one of {sorted(_KINDS)}, got {kind!r}")
    if pred.dim() != 2 or pred.dtype != torch.float32 or pred.stride(1) != 1 or not pred.is_cuda:
        raise ValueError("predicted embeddings must be a [n, E] fp32 device tensor with unit column stride")
    if src.dim() != 2 or src.dtype not in zett_dtypes() or src.stride(1) != 1 or src.device != pred.device:
        raise ValueError("source_embeddings must be a 2-D fp32 / f16 / bf16 tensor on the device of the predictions")
    if ids.dtype not in (torch.int32, torch.int64) or ids.device != pred.device:
        raise ValueError("ids must be an int32 / int64 tensor on the device of the predictions")
    n, e = pred.shape
    if n == 0:
        raise ValueError("the loss of zero rows is undefined (the reference's mean over an empty axis)")
    if col0 < 0 or col0 + e > src.shape[1]:
        raise ValueError(f"columns [{col0}, {col0 + e}) are outside source_embeddings {tuple(src.shape)}")
    if mask is not None and (mask.dtype != torch.float32 or mask.shape != (n,) or not mask.is_contiguous()):
        raise ValueError("mask must be a contiguous fp32 [n] tensor")
    return (ptr(pred), pred.stride(0), ptr(src), zett_dtypes()[src.dtype], src.stride(0), src.shape[0], int(col0), ptr(ids), ids.element_size(), int(ids_stride),
            ptr(mask)), n, e


def embed_distance_forward(pred, src, col0, ids, ids_stride=1, mask=None, kind="mse", mode=_lib.LOSS_MEAN):
    """Rows pass + finalise.  Returns (record, row_dist, row_tnorm): record = [loss, gradient scale, masked-row fraction, 0] on the
    device; the target of row r is ``src[clamp(ids[r * ids_stride], 0, len(src) - 1), col0 : col0 + E]``."""
    lib = _lib.load()
    head, n, e = _dist_args(pred, src, col0, ids, ids_stride, mask, kind)
    with torch.cuda.device(pred.device):
        rows = torch.empty((2, n), dtype=torch.float32, device=pred.device)
        record = torch.empty(4, dtype=torch.float32, device=pred.device)
        st = stream(pred.device)
        _lib.check(lib.zett_op_embed_dist_rows(*head, n, e, _KINDS[kind], ptr(rows[0]), ptr(rows[1]), st), "embed_dist_rows")
        _lib.check(lib.zett_op_embed_dist_finalize(ptr(rows[0]), ptr(rows[1]), ptr(mask), n, int(mode), ptr(record), st), "embed_dist_finalize")
    return record, rows[0], rows[1]


def embed_distance_backward(pred, src, col0, ids, ids_stride, mask, kind, row_dist, record, upstream, out=None, accumulate=False):
    """``out`` (=, or with accumulate +=) upstream * record[1] * mask[r] * d distance / d pred.  ``upstream`` is a device scalar."""
    lib = _lib.load()
    head, n, e = _dist_args(pred, src, col0, ids, ids_stride, mask, kind)
    if out is None:
        if accumulate:
            raise ValueError("accumulate needs the tensor to add to")
        out = torch.empty((n, e), dtype=torch.float32, device=pred.device)
    if out.shape != (n, e) or out.dtype != torch.float32 or out.stride(1) != 1 or out.device != pred.device:
        raise ValueError("out must be a [n, E] fp32 tensor with unit column stride on the device of the predictions")
    upstream = upstream.detach().to(device=pred.device, dtype=torch.float32).reshape(1)
    with torch.cuda.device(pred.device):
        _lib.check(lib.zett_op_embed_dist_grad(*head, ptr(row_dist), n, e, _KINDS[kind], ptr(record), ptr(upstream), ptr(out), out.stride(0),
                                               int(bool(accumulate)), stream(pred.device)), "embed_dist_grad")
    return out


def single_token_mask(target_surface_forms: torch.Tensor, pad_token_id: int) -> torch.Tensor:
    """fp32 [n]: 1 where every position after the first is pad (lexical_overlap_mask, train.py:1092-1094), on the device."""
    ids = target_surface_forms
    if ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64) or ids.stride(1) != 1 or not ids.is_cuda:
        raise ValueError("target_surface_forms must be a [n, L] int32 / int64 device tensor with unit column stride")
    mask = torch.empty(ids.shape[0], dtype=torch.float32, device=ids.device)
    with torch.cuda.device(ids.device):
        _lib.check(_lib.load().zett_op_single_token_mask(ptr(ids), ids.element_size(), ids.shape[0], ids.shape[1], ids.stride(0), int(pad_token_id), ptr(mask),
                                                         stream(ids.device)), "single_token_mask")
    return mask


class _EmbedDistance(torch.autograd.Function):
    """(pred, src, ids, mask) -> (loss, masked-row fraction), both 0-dim on the device.  Gradient for pred only: the source
    embeddings are frozen targets (the reference differentiates with respect to the hypernetwork's parameters)."""

    @staticmethod
    def forward(ctx, pred, src, col0, ids, ids_stride, mask, kind, mode):
        p = pred.detach()
        if p.dtype != torch.float32 or p.stride(-1) != 1:
            p = p.float().contiguous()
        record, row_dist, _ = embed_distance_forward(p, src, col0, ids, ids_stride, mask, kind, mode)
        ctx.save_for_backward(p, src, ids, mask, row_dist, record)
        ctx.args = (int(col0), int(ids_stride), kind)
        ctx.pred_dtype = pred.dtype
        loss, fraction = record[0].clone(), record[2].clone()          # (own storage: autograd outputs must not alias the saved record)
        ctx.mark_non_differentiable(fraction)
        return loss, fraction

    @staticmethod
    def backward(ctx, d_loss, _d_fraction):
        p, src, ids, mask, row_dist, record = ctx.saved_tensors
        col0, ids_stride, kind = ctx.args
        d = embed_distance_backward(p, src, col0, ids, ids_stride, mask, kind, row_dist, record, d_loss)
        return d.to(ctx.pred_dtype), None, None, None, None, None, None, None


def _pair(pred_in, pred_out, source_embeddings, ids, ids_stride, mask, kind, mode):
    if pred_in.dim() != 2:
        raise ValueError("predicted embeddings must be [n, E]")
    e = pred_in.shape[1]
    src = source_embeddings if source_embeddings.dtype in zett_dtypes() else source_embeddings.float()
    need = e if pred_out is None else 2 * e
    if src.dim() != 2 or src.shape[1] < need:
        raise ValueError(f"source_embeddings must be [V, >= {need}] (input half{'' if pred_out is None else ' + output half'}), got {tuple(src.shape)}")
    loss, fraction = _EmbedDistance.apply(pred_in, src, 0, ids, ids_stride, mask, kind, mode)
    if pred_out is not None:
        if pred_out.shape != pred_in.shape:
            raise ValueError("pred_in and pred_out must have the same shape")
        loss_out, _ = _EmbedDistance.apply(pred_out, src, e, ids, ids_stride, mask, kind, mode)
        loss = (loss + loss_out) / 2.0
    return loss, fraction


def identity_loss(pred_in, pred_out, source_embeddings, ids_to_embed):
    """The loss of the reference's identity warm-up (identity_train_step, train.py:941-960): the mean over rows of
    ``sum((pred - source_embeddings[ids_to_embed]) ** 2, -1)``, for the input half ``source_embeddings[:, :E]`` and, when
    ``pred_out`` is not None, the mean of that and the same on the output half ``[:, E:2E]``.  Returns a 0-dim device tensor;
    differentiable in pred_in / pred_out.  Ids outside the matrix are clamped to its first / last row (JAX's gather)."""
    if ids_to_embed.dim() != 1 or ids_to_embed.shape[0] != pred_in.shape[0]:
        raise ValueError("ids_to_embed must hold one id per predicted row")
    loss, _ = _pair(pred_in, pred_out, source_embeddings, ids_to_embed, ids_to_embed.stride(0), None, "mse", _lib.LOSS_MEAN)
    return loss


def lexical_loss(pred_in, pred_out, source_embeddings, target_surface_forms, pad_token_id, kind="mse"):
    """The lexical loss of train.py:1086-1142: rows whose surface form is ONE token (every later position is pad) are pulled
    towards the source row of that token,

        sum(distance(pred, target) * mask) / (sum(mask) + 1e-8) / mean(||target||)         (mean over all rows, train.py:1124)

    with ``target = source_embeddings[target_surface_forms[:, 0]]`` (out-of-range ids — a fallback id — clamped to the last row,
    JAX's gather) and kind "mse" | "rmse" | "huber" (delta 1e-3, / 1e-3 / 30).  With pred_out, the mean of the input-half and
    output-half losses.  Returns ``(loss, mean_lexical_overlap)``, 0-dim device tensors; the caller applies lexical_loss_weight.
    Deviation: the "rmse" gradient of a row that equals its target is 0 (the reference's is NaN)."""
    tsf = target_surface_forms
    if tsf.dim() != 2 or tsf.shape[0] != pred_in.shape[0]:
        raise ValueError("target_surface_forms must be [n, L] with one row per predicted row")
    mask = single_token_mask(tsf, pad_token_id)
    return _pair(pred_in, pred_out, source_embeddings, tsf, tsf.stride(0), mask, kind, _lib.LOSS_LEXICAL)


# ---- the language-model loss over predicted output embeddings ----------------------------------------------------------------
_LM_PRECISIONS = {"f32": (None, torch.float32, 32), "bf16": (_lib.PREC_BF16, torch.bfloat16, 64), "f16": (_lib.PREC_F16, torch.float16, 64)}      # (prec, operand dtype, K step)
_LM_PATHS = {None: _lib.CE_AUTO, "auto": _lib.CE_AUTO, "once": _lib.CE_ONCE, "twice": _lib.CE_TWICE}
LM_LOGITS_BYTES = 1 << 30          # the logits chunk of lm_head_loss stays at or below this


def lm_label_arrays(labels, attention_mask=None, mode=None, weight=None):
    """The reference's loss_fn (train.py:874-912) as one label and one weight per position, ``(labels' int32 [T], weight fp32 [T] | None)``:

    - "clm": position s is scored against ``labels[..., s + 1]`` with weight ``attention_mask[..., s]``; the last position of a sequence has
      weight 0 (``logits[..., :-1, :]``, ``labels[..., 1:]``, ``attention_mask[..., :-1]``, train.py:883-885) — no view of the logits or the
      hidden state is shifted;
    - "mlm": ``weight = (labels != -100) & (attention_mask == 1)`` (train.py:902);
    - None: the given `weight`, or None for all ones.

    Small integer arrays, prepared with torch on the device the labels are on."""
    if mode not in ("clm", "mlm", None):
        raise ValueError(f'mode must be "clm", "mlm" or None, got {mode!r}')
    if labels.dtype not in (torch.int32, torch.int64) or labels.dim() < 1:
        raise ValueError("labels must be an int32 / int64 tensor with at least one dimension")
    if attention_mask is not None and attention_mask.shape != labels.shape:
        raise ValueError(f"attention_mask {tuple(attention_mask.shape)} must have the shape of labels {tuple(labels.shape)}")
    if weight is not None and weight.shape != labels.shape:
        raise ValueError(f"weight {tuple(weight.shape)} must have the shape of labels {tuple(labels.shape)}")
    if mode is not None and weight is not None:
        raise ValueError(f'mode "{mode}" derives the weights from labels and attention_mask: pass weight with mode=None only')
    if mode is None and attention_mask is not None:
        raise ValueError("attention_mask needs mode=\"clm\" or \"mlm\"; with mode=None pass the weights as weight")
    labels = labels.clamp(-(2 ** 31), 2 ** 31 - 1)
    if mode == "clm":
        lab = torch.full_like(labels, -100)
        lab[..., :-1] = labels[..., 1:]
        w = torch.zeros(labels.shape, dtype=torch.float32, device=labels.device)
        w[..., :-1] = 1.0 if attention_mask is None else attention_mask[..., :-1].to(torch.float32)
    elif mode == "mlm":
        lab = labels
        keep = labels != -100
        if attention_mask is not None:
            keep = keep & (attention_mask == 1)
        w = keep.to(torch.float32)
    else:
        lab, w = labels, None if weight is None else weight.to(torch.float32)
    return lab.to(torch.int32).reshape(-1).contiguous(), None if w is None else w.reshape(-1).contiguous()


def lm_default_chunk_rows(vocab: int, precision: str = "bf16") -> int:
    """Rows of one logits chunk: the largest multiple of 64 whose fp32 logits ``rows x V_padded x 4`` bytes fit LM_LOGITS_BYTES (1 GiB), at
    least 64.  V = 32 768: 8 192 rows; V = 262 144: 1 024 rows."""
    kstep = _LM_PRECISIONS[precision][2]
    vp = -(-int(vocab) // kstep) * kstep
    return max(64, (LM_LOGITS_BYTES // (4 * vp)) // 64 * 64)


def _lm_check(hidden, pred_out, labels, bias, priors, vocab_mask, precision, chunk_rows, path):
    """Everything that can be refused is refused here, before the first launch."""
    if precision not in _LM_PRECISIONS:
        raise ValueError(f"precision must be one of {sorted(_LM_PRECISIONS)}, got {precision!r}")
    if path not in _LM_PATHS:
        raise ValueError(f'rows_path must be None, "auto", "once" or "twice", got {path!r}')
    if hidden.dim() < 2 or hidden.dtype not in zett_dtypes():
        raise ValueError("hidden must be a [..., E] fp32 / f16 / bf16 tensor")
    if pred_out.dim() != 2 or pred_out.dtype != torch.float32 or pred_out.shape[1] != hidden.shape[-1]:
        raise ValueError(f"pred_out must be a [V, E] fp32 tensor with E = {hidden.shape[-1]}, got {tuple(pred_out.shape)} {pred_out.dtype}")
    v, e = pred_out.shape
    t = hidden.numel() // max(e, 1)
    if v == 0 or e == 0 or t == 0:
        raise ValueError("the loss of an empty hidden state or vocabulary is undefined")
    if tuple(labels.shape) != tuple(hidden.shape[:-1]):
        raise ValueError(f"labels {tuple(labels.shape)} must have the leading shape of hidden {tuple(hidden.shape[:-1])}")
    for name, x in (("bias", bias), ("priors", priors), ("vocab_mask", vocab_mask)):
        if x is None:
            continue
        if tuple(x.shape) != (v,):
            raise ValueError(f"{name} must be [V] = [{v}], got {tuple(x.shape)}")
        if name == "vocab_mask" and x.dtype != torch.bool:
            raise ValueError("vocab_mask must be a bool tensor (True: the column is in the vocabulary)")
        if name != "vocab_mask" and not x.dtype.is_floating_point:
            raise ValueError(f"{name} must be a floating-point tensor")
    if chunk_rows is not None and (int(chunk_rows) != chunk_rows or chunk_rows < 1):
        raise ValueError(f"chunk_rows must be a positive integer, got {chunk_rows!r}")
    if path == "once" and -(-v // _LM_PRECISIONS[precision][2]) * _LM_PRECISIONS[precision][2] > _lib.CE_ONCE_MAX_COLS:
        raise ValueError(f"the read-once rows pass holds at most {_lib.CE_ONCE_MAX_COLS} columns")


def _lm_check_device(pred_out, **others):
    if not pred_out.is_cuda:
        raise ValueError("zett_amd computes on the GPU only: pred_out must be a cuda (ROCm) tensor; there is no CPU path")
    for name, x in others.items():
        if x is not None and x.device != pred_out.device:
            raise ValueError(f"{name} must be on the device of pred_out ({pred_out.device}), got {x.device}")


def _lm_run(hidden, w_out, bias, priors, vocab_mask, lab, wgt, precision, chunk_rows, path, want_h, want_w, want_b):
    """The launches of lm_head_loss on flattened, detached inputs.  -> record [8], row_loss, lse, argmax, d hidden | None, d pred_out | None,
    d bias | None (the gradients unscaled: zett_op_ce_scale multiplies them by upstream / sum(w) in the backward)."""
    lib = _lib.load()
    dev = w_out.device
    prec, lo_dtype, kstep = _LM_PRECISIONS[precision]
    lo_code = zett_dtypes()[lo_dtype]
    t, e = hidden.shape
    v = w_out.shape[0]
    vp, ep = -(-v // kstep) * kstep, -(-e // kstep) * kstep
    tc = min(t, int(chunk_rows) if chunk_rows is not None else lm_default_chunk_rows(v, precision))
    tcp = -(-tc // kstep) * kstep
    want = want_h or want_w or want_b
    f32 = torch.float32

    def new(*shape, dtype=f32):
        return torch.empty(shape, dtype=dtype, device=dev)

    with torch.cuda.device(dev):
        st = stream(dev)

        def gemm(a, lda, w, ldw, m, n, k, out, ld_out, addend=None, residual=None, ld_res=0):
            if prec is None:
                _lib.check(lib.zett_op_gemm_f32(ptr(a), lda, ptr(w), ldw, m, n, k, ptr(addend), 0, ptr(residual), ld_res, ptr(out), ld_out, st), "zett_op_gemm_f32")
            else:
                _lib.check(lib.zett_op_gemm_lo(prec, ptr(a), lda, ptr(w), ldw, m, n, k, ptr(addend), 0, ptr(residual), ld_res, ptr(out), ld_out, st), "zett_op_gemm_lo")

        def transpose(x, ld_in, out, ld_out, rows, cols, rows_padded):          # out[c, r] = x[r, c], rows zero-padded: operands of the training GEMMs
            if prec is None:
                _lib.check(lib.zett_op_transpose_f32(ptr(x), ld_in, ptr(out), ld_out, rows, cols, rows_padded, st), "zett_op_transpose_f32")
            else:
                _lib.check(lib.zett_op_transpose_lo16(prec, ptr(x), ld_in, ptr(out), ld_out, rows, cols, rows_padded, st), "zett_op_transpose_lo16")

        # once per call: the addend vector and the operand forms of pred_out
        addend = None
        if bias is not None or priors is not None or vocab_mask is not None:
            addend = new(vp)
            _lib.check(lib.zett_op_ce_addend(ptr(bias), ptr(priors), ptr(None if vocab_mask is None else vocab_mask.view(torch.uint8)), v, vp, ptr(addend), st), "zett_op_ce_addend")
        if prec is None:
            if ep == e and w_out.stride(0) % 4 == 0 and w_out.data_ptr() % 16 == 0:
                w_op = w_out
            else:
                w_op = new(v, ep)
                _lib.check(lib.zett_op_ce_cast(ptr(w_out), _lib.DTYPE_F32, w_out.stride(0), ptr(w_op), _lib.DTYPE_F32, ep, v, e, ep, st), "zett_op_ce_cast")
        else:
            w_op = new(v, ep, dtype=lo_dtype)
            _lib.check(lib.zett_op_convert_lo(prec, ptr(w_out), w_out.stride(0), ptr(w_op), ep, v, e, ep, st), "zett_op_convert_lo")
        w_t = None
        if want_h:                                   # lo(W)^T [E, V'] (V zero-padded to the K step): the operand of d hidden = G . W
            w_t = new(e, vp, dtype=lo_dtype)
            if prec is None:
                _lib.check(lib.zett_op_transpose_f32(ptr(w_out), w_out.stride(0), ptr(w_t), vp, v, e, vp, st), "zett_op_transpose_f32")
            else:
                _lib.check(lib.zett_op_transpose_lo(prec, ptr(w_out), w_out.stride(0), ptr(w_t), vp, v, e, vp, st), "zett_op_transpose_lo")

        direct = hidden.dtype == lo_dtype and ep == e and hidden.stride(0) % 8 == 0 and hidden.data_ptr() % 16 == 0          # the hidden state is an operand as it is
        a_buf = None if direct else new(tc, ep, dtype=lo_dtype)
        logits = new(tc, vp)
        g = None if not want else (logits if prec is None else new(tc, vp, dtype=lo_dtype))
        row_loss, lse, argmax, record = new(t), new(t), new(t, dtype=torch.int32), new(8)
        d_hidden = new(t, e) if want_h else None
        d_bias = new(v) if want_b else None
        g_t = h_t = d_w = d_w_prev = None
        if want_w:
            g_t, h_t, d_w = new(v, tcp, dtype=lo_dtype), new(e, tcp, dtype=lo_dtype), new(v, e)
            if t > tc:
                d_w_prev = new(v, e)              # the accumulation goes through the GEMM's residual input, from one buffer into the other

        for i, r0 in enumerate(range(0, t, tc)):
            n = min(tc, t - r0)
            np_ = -(-n // kstep) * kstep
            if direct:
                a, lda = hidden[r0:r0 + n], hidden.stride(0)
            else:
                a, lda = a_buf, ep
                _lib.check(lib.zett_op_ce_cast(ptr(hidden[r0:r0 + n]), zett_dtypes()[hidden.dtype], hidden.stride(0), ptr(a), lo_code, ep, n, e, ep, st), "zett_op_ce_cast")
            gemm(a, lda, w_op, w_op.stride(0), n, v, ep, logits, vp, addend=addend)
            _lib.check(lib.zett_op_ce_rows(ptr(logits), vp, ptr(lab[r0:]), ptr(None if wgt is None else wgt[r0:]), n, v, vp, ptr(g), lo_code, vp,
                                           ptr(row_loss[r0:]), ptr(lse[r0:]), ptr(argmax[r0:]), _LM_PATHS[path], st), "zett_op_ce_rows")
            if want_b:
                _lib.check(lib.zett_op_ce_colsum(ptr(g), lo_code, vp, n, v, ptr(d_bias), int(i > 0), st), "zett_op_ce_colsum")
            if want_w:                               # dW += G^T . hidden_chunk
                transpose(g, vp, g_t, tcp, n, v, np_)
                transpose(a, lda, h_t, tcp, n, e, np_)
                if i > 0:
                    d_w, d_w_prev = d_w_prev, d_w
                gemm(g_t, tcp, h_t, tcp, v, e, np_, d_w, e, residual=d_w_prev if i > 0 else None, ld_res=e if i > 0 else 0)
            if want_h:                               # d hidden_chunk = G . W
                gemm(g, vp, w_t, vp, n, e, vp, d_hidden[r0:], e)
        _lib.check(lib.zett_op_ce_finalize(ptr(row_loss), ptr(wgt), ptr(lab), ptr(argmax), t, ptr(record), st), "zett_op_ce_finalize")
    return record, row_loss, lse, argmax, d_hidden, d_w if want_w else None, d_bias


def _lm_scale(x, record, upstream, dtype):
    """x * upstream / sum(w) as `dtype`; both factors are read on the device."""
    out = torch.empty(x.shape, dtype=dtype, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().zett_op_ce_scale(ptr(x), x.numel(), ptr(record), ptr(upstream), ptr(out), zett_dtypes()[dtype], stream(x.device)), "zett_op_ce_scale")
    return out


class _LMHeadLoss(torch.autograd.Function):
    """(hidden [T, E], pred_out, bias) -> (loss, row_loss, lse, argmax, record).  The gradients are computed in the forward — the logits
    are not kept — and stored unscaled; the backward multiplies them by upstream / sum(w)."""

    @staticmethod
    def forward(ctx, hidden, pred_out, bias, priors, vocab_mask, lab, wgt, precision, chunk_rows, path):
        want_h, want_w, want_b = hidden.requires_grad, pred_out.requires_grad, bias is not None and bias.requires_grad
        record, row_loss, lse, argmax, d_h, d_w, d_b = _lm_run(hidden.detach(), pred_out.detach(), None if bias is None else bias.detach(), priors, vocab_mask, lab, wgt,
                                                               precision, chunk_rows, path, want_h, want_w, want_b)
        ctx.save_for_backward(record, *(x for x in (d_h, d_w, d_b) if x is not None))
        ctx.have = (d_h is not None, d_w is not None, d_b is not None)
        ctx.hidden_dtype = hidden.dtype
        loss, stats_record = record[0].clone(), record.clone()          # (own storage: autograd outputs must not alias the saved record)
        ctx.mark_non_differentiable(row_loss, lse, argmax, stats_record)
        return loss, row_loss, lse, argmax, stats_record

    @staticmethod
    def backward(ctx, d_loss, *_):
        record, *grads = ctx.saved_tensors
        grads = iter(grads)
        upstream = d_loss.detach().to(device=record.device, dtype=torch.float32).reshape(1)
        out = []
        for have, dtype in zip(ctx.have, (ctx.hidden_dtype, torch.float32, torch.float32)):
            out.append(_lm_scale(next(grads), record, upstream, dtype) if have else None)
        return (*out, None, None, None, None, None, None, None)


def lm_head_loss(hidden, pred_out, labels, attention_mask=None, *, mode=None, weight=None, bias=None, priors=None, vocab_mask=None, precision="bf16",
                 chunk_rows=None, rows_path=None):
    """The language-model loss of the reference's train_step / eval_step over PREDICTED output embeddings (train.py:1039-1056, 874-912,
    1226-1255) — the term every gradient of ``pred_out`` and of the predicted bias comes from:

        logits = hidden @ pred_out.T                                  [T, V], V = the sampled vocabulary
        logits += where(vocab_mask, 0, -100000)                       NEGATIVE_INF_FILL_VALUE, zett/utils.py:23
        logits += bias                                                learnable_bias
        logits += priors                                              add_target_priors_to_bias
        loss = sum(softmax_cross_entropy(logits, onehot(labels)) * weight) / sum(weight)

    hidden: ``[..., E]`` fp32 / bf16 / f16, the backbone's final hidden state (leading dimensions are flattened to T; may require grad).
    pred_out: ``[V, E]`` fp32, what ``ZettHypernet.forward`` returns (``pred_in`` for tied models).  bias / priors (floating point) and
    vocab_mask (bool, True = in the vocabulary) are ``[V]``: one addend vector, built once per call on the device and added in the logits
    GEMM's epilogue.  labels: integers of hidden's leading shape; a label outside ``[0, V)`` — ``-100`` included — is an all-zero one-hot
    (jax.nn.one_hot): the row's loss is ``weight * logsumexp``.

    mode: "clm" takes UNSHIFTED ``[B, S]`` labels and attention mask (position s is scored against ``labels[b, s + 1]`` with weight
    ``attention_mask[b, s]``, the last position has weight 0: train.py:883-885 as a label and a weight array — hidden is never sliced);
    "mlm" uses ``weight = (labels != -100) & (attention_mask == 1)``; None uses `weight`, or all ones (lm_label_arrays).

    precision: the arithmetic of the three contractions — "bf16" / "f16" MFMA operands with fp32 accumulation, or exact "f32"; softmax,
    sums and gradients are fp32.  A 16-bit hidden of the operand type with ``E % 64 == 0`` is used as it is.

    T is processed in chunks of `chunk_rows` rows (default lm_default_chunk_rows: the largest multiple of 64 whose fp32 logits chunk
    ``chunk_rows x V_padded x 4`` bytes stays at or below 1 GiB — 8 192 rows at V = 32 768): the logits GEMM, the softmax rows pass
    (csrc/train_loss.hip) and, when any of hidden / pred_out / bias requires grad, ``dW += G^T . hidden_chunk`` and
    ``d hidden_chunk = G . W`` with ``G = weight * (softmax - onehot)`` in the operand type.  The full ``[T, V]`` logits never exist.  loss,
    row_loss, lse, argmax and d hidden do not depend on the chunk size (same bits); d pred_out and d bias are summed over T chunk by
    chunk, so their last bits do.  rows_path ("once" | "twice", tests): force the rows pass to keep a row in registers or to read it
    twice — same bits.

    Returns ``(loss, stats)``: loss 0-dim on the device, differentiable in hidden, pred_out and bias (the gradients are formed in the forward
    and stored unscaled; backward multiplies them by ``upstream / sum(weight)`` read from device memory and returns d hidden in hidden's
    dtype).  stats (device tensors, no gradient): ``row_loss [T]`` = weight * cross-entropy, ``lse [T]``, ``argmax [T]`` int32 (the first
    maximum), ``n_correct`` / ``n_counted`` (int32: rows with weight > 0, and those of them whose argmax is the label), ``weight_sum``.
    Under ``torch.no_grad()`` or when nothing requires grad — eval_step — only the logits GEMM and the rows pass run and nothing is saved; the
    reference's ``acc`` is ``n_correct / n_counted`` and its bits per byte (clm, train.py:894-898) are
    ``(stats["row_loss"].view(B, S).sum(-1) / byte_lengths.sum(-1)).mean()``.

    Nothing here waits for the host; two runs give the same bits.  Deviation: ``sum(weight) == 0`` gives loss 0 and zero gradients (the
    reference divides 0 by 0 and returns NaN), as the "rmse" gradient at distance 0 does in lexical_loss."""
    _lm_check(hidden, pred_out, labels, bias, priors, vocab_mask, precision, chunk_rows, rows_path)
    lab, wgt = lm_label_arrays(labels, attention_mask, mode, weight)
    _lm_check_device(pred_out, hidden=hidden, labels=labels, bias=bias, priors=priors, vocab_mask=vocab_mask, weights=wgt)
    e = hidden.shape[-1]
    h2 = hidden.reshape(-1, e)
    if h2.stride(1) != 1:
        h2 = h2.contiguous()
    bias32 = None if bias is None else bias.to(torch.float32)
    priors32 = None if priors is None else priors.detach().to(torch.float32).contiguous()
    mask = None if vocab_mask is None else vocab_mask.contiguous()
    if torch.is_grad_enabled() and (h2.requires_grad or pred_out.requires_grad or (bias32 is not None and bias32.requires_grad)):
        loss, row_loss, lse, argmax, record = _LMHeadLoss.apply(h2, pred_out, None if bias32 is None else bias32.contiguous(), priors32, mask, lab, wgt, precision,
                                                               chunk_rows, rows_path)
    else:
        record, row_loss, lse, argmax, _, _, _ = _lm_run(h2.detach(), pred_out.detach(), None if bias32 is None else bias32.detach().contiguous(), priors32, mask, lab, wgt,
                                                         precision, chunk_rows, rows_path, False, False, False)
        loss = record[0]
    counts = record.view(torch.int32)
    return loss, {"row_loss": row_loss, "lse": lse, "argmax": argmax, "n_correct": counts[3], "n_counted": counts[4], "weight_sum": record[1]}


# ---- the input side: special rows, token lookup ------------------------------------------------------------------------------
EMBED_BWD_CHUNK = _lib.EMBED_BWD_CHUNK          # positions of one partial sum of token_embeddings' backward: part of the definition of d pred_in


def _index_list(x, name):
    """A small index list (Python sequence, numpy array, CPU or device integer tensor) as a 1-D int64 numpy array on the host."""
    import numpy as np
    if isinstance(x, torch.Tensor):
        if x.dtype.is_floating_point or x.dtype == torch.bool:
            raise ValueError(f"{name} must hold integers, got {x.dtype}")
        x = x.detach().cpu().numpy()          # (a device tensor: one small copy to the host)
    a = np.asarray(x)
    if a.size == 0:
        return np.zeros(0, dtype=np.int64)
    if a.dtype.kind not in "iu":
        raise ValueError(f"{name} must hold integers, got dtype {a.dtype}")
    if a.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional, got shape {a.shape}")
    return a.astype(np.int64)


def check_special_indices(special_indices, special_indices_in_reference, n_rows: int, n_reference_rows: int):
    """The host-side validation of splice_special_rows, before the library is touched: -> (rows, reference rows) as int32 numpy arrays.
    Lists of different length or a duplicate in special_indices: ValueError; an index outside [0, n_rows) or a reference row outside
    [0, n_reference_rows): IndexError; more than 256 entries: ValueError."""
    import numpy as np
    rows, refs = _index_list(special_indices, "special_indices"), _index_list(special_indices_in_reference, "special_indices_in_reference")
    if rows.shape != refs.shape:
        raise ValueError(f"special_indices holds {rows.size} entries, special_indices_in_reference {refs.size}")
    bad = rows[(rows < 0) | (rows >= n_rows)]
    if bad.size:
        raise IndexError(f"special index {int(bad[0])} is outside the {n_rows} predicted rows")
    bad = refs[(refs < 0) | (refs >= n_reference_rows)]
    if bad.size:
        raise IndexError(f"reference row {int(bad[0])} is outside the {n_reference_rows} rows of source_embeddings")
    if rows.size > _lib.SPLICE_MAX_ROWS:
        raise ValueError(f"special_indices holds {rows.size} entries, at most {_lib.SPLICE_MAX_ROWS} travel with a launch")
    if np.unique(rows).size != rows.size:
        raise ValueError("special_indices holds a row twice: which source row wins would be unspecified (JAX leaves it open)")
    return rows.astype(np.int32), refs.astype(np.int32)


def _splice_launch(src_matrix, out, source, col0, rows, refs):
    """out[rows] = source[refs, col0 : col0 + E] (source None: zeros); every other row of out from src_matrix (None: left as it is)."""
    n = len(rows)
    r = (C.c_int32 * max(n, 1))(*rows.tolist())
    f = (C.c_int32 * max(n, 1))(*(refs.tolist() if refs is not None else []))
    v, e = out.shape
    with torch.cuda.device(out.device):
        _lib.check(_lib.load().zett_op_splice_rows(ptr(src_matrix), 0 if src_matrix is None else src_matrix.stride(0), ptr(out), out.stride(0), v, e, ptr(source),
                                                   _lib.DTYPE_F32 if source is None else zett_dtypes()[source.dtype], 0 if source is None else source.stride(0),
                                                   0 if source is None else source.shape[0], int(col0), r, f, n, stream(out.device)), "splice_rows")
    return out


class _SpliceRows(torch.autograd.Function):
    """pred -> pred with the listed rows replaced by source rows.  Gradient: the incoming one with those rows zero, written to a fresh matrix
    in one pass; the source is a frozen target."""

    @staticmethod
    def forward(ctx, pred, source, col0, rows, refs, inplace):
        ctx.rows = rows
        if inplace:
            ctx.mark_dirty(pred)
            return _splice_launch(None, pred, source, col0, rows, refs)
        return _splice_launch(pred.detach(), torch.empty(pred.shape, dtype=torch.float32, device=pred.device), source, col0, rows, refs)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        g = grad.detach()
        if g.dtype != torch.float32 or g.stride(1) != 1:
            g = g.float().contiguous()
        return _splice_launch(g, torch.empty(g.shape, dtype=torch.float32, device=g.device), None, 0, ctx.rows, None), None, None, None, None, None


def splice_special_rows(pred_in, pred_out, source_embeddings, special_indices, special_indices_in_reference, *, inplace=False):
    """The special rows of the predicted matrices (train.py:1014-1017, 1027-1030; eval 1198-1205): for every i, row
    ``special_indices[i]`` of pred_in becomes ``source_embeddings[special_indices_in_reference[i], 0:E]`` and the same row of pred_out
    becomes ``source_embeddings[.., E:2E]`` — the column split of identity_loss / lexical_loss.  Returns ``(pred_in', pred_out')``;
    pred_out may be None (tied embeddings), then pred_out' is None.  The lexical loss and the logits both take the spliced matrices.

    pred_in / pred_out: ``[V, E]`` fp32 device tensors with unit column stride.  source_embeddings: fp32 / f16 / bf16, converted exactly; a
    source with fewer than 2E columns and a pred_out is a ValueError.  The index lists are small (``tokenizer.all_special_ids``): Python
    sequences, numpy arrays, CPU or device integer tensors — a device tensor costs one small copy to the host, the collator produces
    numpy anyway.  They are validated on the host before any launch (duplicates in special_indices: ValueError — JAX leaves the winner
    unspecified; an index outside ``[0, V)`` or a reference row outside the source: IndexError) and travel to the kernel as kernel
    arguments, so nothing is staged in a buffer a later call could overwrite.

    inplace=False writes fresh matrices in ONE pass (copy, listed rows from the source).  inplace=True overwrites the listed rows of the
    given tensors and moves nothing else; autograd sees an in-place operation, which is safe on the outputs of the hypernetwork (its
    Function does not save them) and refused by torch on a leaf that requires grad.  Either way the gradient of each output is the
    incoming gradient with the listed rows zero — a fresh matrix, the incoming one is never modified — and source_embeddings gets none.
    With no special indices the inputs are returned as they are."""
    if pred_in.dim() != 2:
        raise ValueError("predicted embeddings must be [V, E]")
    v, e = pred_in.shape
    src = source_embeddings
    need = e if pred_out is None else 2 * e
    if src.dim() != 2 or src.shape[1] < need:
        raise ValueError(f"source_embeddings must be [R, >= {need}] (input half{'' if pred_out is None else ' + output half'}), got {tuple(src.shape)}")
    if pred_out is not None and pred_out.shape != pred_in.shape:
        raise ValueError("pred_in and pred_out must have the same shape")
    rows, refs = check_special_indices(special_indices, special_indices_in_reference, v, src.shape[0])
    if rows.size == 0:
        return pred_in, pred_out
    for name, p in (("pred_in", pred_in), ("pred_out", pred_out)):
        if p is not None and (p.dtype != torch.float32 or not p.is_cuda or p.device != pred_in.device or (inplace and p.stride(1) != 1)):
            raise ValueError(f"{name} must be a [V, E] fp32 device tensor{' with unit column stride' if inplace else ''}")
        if p is not None and inplace and torch.is_grad_enabled() and p.requires_grad and p.is_leaf:          # (torch would say so only after the rows are written)
            raise RuntimeError(f"{name} is a leaf that requires grad: it cannot be spliced in place (use inplace=False, or splice the hypernetwork's outputs)")
    if src.dtype not in zett_dtypes():
        src = src.float()
    if src.device != pred_in.device or src.stride(1) != 1:
        raise ValueError("source_embeddings must be on the device of the predictions, with unit column stride")
    src = src.detach()
    out = []
    for p, col0 in ((pred_in, 0), (pred_out, e)):
        if p is not None and not inplace and p.stride(1) != 1:
            p = p.contiguous()
        out.append(None if p is None else _SpliceRows.apply(p, src, col0, rows, refs, bool(inplace)))
    return out[0], out[1]


def _lookup(table, ids, dtype, check_ids):
    t, (v, e) = ids.numel(), table.shape
    out = torch.empty(tuple(ids.shape) + (e,), dtype=dtype, device=table.device)
    if t == 0:
        return out
    with torch.cuda.device(table.device):
        word = torch.zeros(1, dtype=torch.int32, device=table.device) if check_ids else None
        _lib.check(_lib.load().zett_op_embed_lookup(ptr(table), zett_dtypes()[table.dtype], table.stride(0), v, e, ptr(ids), ids.element_size(), t, ptr(out),
                                                    zett_dtypes()[dtype], ptr(word), stream(table.device)), "embed_lookup")
    if check_ids and int(word.item()):          # (the one host read of this call)
        raise IndexError(f"token_embeddings: an id in input_ids is outside [0, {v})")
    return out


def embed_lookup_workspace(t: int, v: int, e: int):
    """(bytes of the plan, bytes of the scratch buffer that only the plan call uses, bytes of the partial-sum rows) of token_embeddings'
    backward for t positions, v rows, e columns."""
    plan, scratch, partial = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.load().zett_op_embed_lookup_workspace_bytes(int(t), int(v), int(e), C.byref(plan), C.byref(scratch), C.byref(partial)), "embed_lookup_workspace_bytes")
    return plan.value, scratch.value, partial.value


def embed_lookup_plan(ids, v: int, id_base: int = 0):
    """The inverted index of `ids` over v rows (per id, its positions in ascending order) as an opaque int32 device tensor: a pure
    function of ids, built on the current stream without a host round trip.  What only the building needs (about 4T + 2V words) is a
    scratch tensor that is released on return — the caching allocator reuses it in stream order — so the plan that autograd holds until
    the backward is T + 2V + T/32 words.  id_base != 0: the index of ``ids - id_base`` (row r lists the positions of id_base + r)."""
    plan_bytes, scratch_bytes, _ = embed_lookup_workspace(ids.numel(), v, 1)
    plan = torch.empty(plan_bytes // 4, dtype=torch.int32, device=ids.device)
    scratch = torch.empty(max(scratch_bytes // 4, 1), dtype=torch.int32, device=ids.device)
    with torch.cuda.device(ids.device):
        if id_base:
            _lib.check(_lib.load().zett_op_embed_lookup_plan_base(ptr(ids), ids.element_size(), ids.numel(), int(id_base), int(v), ptr(plan), plan.numel() * 4,
                                                                  ptr(scratch), scratch.numel() * 4, stream(ids.device)), "embed_lookup_plan_base")
        else:
            _lib.check(_lib.load().zett_op_embed_lookup_plan(ptr(ids), ids.element_size(), ids.numel(), int(v), ptr(plan), plan.numel() * 4, ptr(scratch),
                                                             scratch.numel() * 4, stream(ids.device)), "embed_lookup_plan")
    return plan


def embed_lookup_backward(grad, plan, t: int, v: int, e: int):
    """d table ``[v, e]`` fp32 from the incoming gradient ``[t, e]`` (fp32 / f16 / bf16, contiguous) and the plan of the ids: every row written once."""
    d = torch.empty((v, e), dtype=torch.float32, device=grad.device)
    partials = torch.empty(embed_lookup_workspace(t, v, e)[2] // 4, dtype=torch.float32, device=grad.device)
    with torch.cuda.device(grad.device):
        _lib.check(_lib.load().zett_op_embed_lookup_bwd(ptr(grad), zett_dtypes()[grad.dtype], int(t), int(v), int(e), ptr(plan), plan.numel() * 4, ptr(partials),
                                                        partials.numel() * 4, ptr(d), e, stream(grad.device)), "embed_lookup_bwd")
    return d


class _TokenEmbeddings(torch.autograd.Function):
    """(pred_in fp32, ids) -> inputs_embeds.  The plan is built in the forward, behind the gather, and is all that is saved."""

    @staticmethod
    def forward(ctx, table, ids, dtype, check_ids):
        out = _lookup(table.detach(), ids, dtype, check_ids)
        ctx.save_for_backward(embed_lookup_plan(ids, table.shape[0]))
        ctx.shape = (ids.numel(), table.shape[0], table.shape[1])
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        plan, = ctx.saved_tensors
        t, v, e = ctx.shape
        g = grad.detach().reshape(t, e)
        if g.dtype not in zett_dtypes():
            g = g.float()
        return embed_lookup_backward(g.contiguous(), plan, t, v, e), None, None, None


def token_embeddings(pred_in, input_ids, *, dtype=None, check_ids=True):
    """The backbone's embedding lookup in the (spliced) predicted input matrix: ``out[..., :] = pred_in[input_ids[...], :]`` converted to
    `dtype` — shape ``input_ids.shape + (E,)``, dtype ``dtype or pred_in.dtype`` — for a backbone that takes ``inputs_embeds``.

    pred_in: ``[V, E]`` fp32 / f16 / bf16 on the device, row stride >= E, unit column stride.  input_ids: int32 / int64 of any shape.  dtype:
    one of the three; fp32 -> 16 bits rounds to nearest even (what ``tensor.to(dtype)`` gives), equal dtypes copy the bits.

    check_ids=True: the kernel ORs into a device error word when it meets an id outside ``[0, V)``; the host reads that word once after
    the launch and raises IndexError, as ``F.embedding`` does.  check_ids=False: no host read; an id outside ``[0, V)`` gives a zero row
    and contributes to no gradient (deviation: torch faults) — it is never used as an address, forward or backward.

    Gradient (an fp32 pred_in only; a 16-bit pred_in that requires grad is a ValueError): a dense fp32 ``[V, E]``.  With
    ``p_0 < p_1 < ...`` the flattened positions that hold id v, g the incoming gradient converted exactly to fp32 and C = EMBED_BWD_CHUNK = 64,

        partial_j    = ((g[p_jC] + g[p_jC+1]) + ...) + g[p_jC+C-1]          fp32, ascending positions, the last chunk ragged
        d pred_in[v] = ((partial_0 + partial_1) + ...) + partial_last       fp32, ascending chunks;  no position: zeros

    — a fixed order that depends on nothing but input_ids (for at most 64 positions the plain sequential sum, the bits of ``np.add.at``), so
    two runs give the same bits; no float atomics.  Every row of d pred_in is written exactly once, zeros included.  The forward builds the
    inverted index of input_ids on the stream (integers only) and saves nothing else.  Under ``torch.no_grad()`` or when pred_in does not
    require grad — eval_step — only the gather runs: no plan, nothing saved."""
    if pred_in.dim() != 2 or pred_in.dtype not in zett_dtypes() or pred_in.stride(1) != 1 or pred_in.shape[0] == 0 or pred_in.shape[1] == 0:
        raise ValueError("pred_in must be a non-empty [V, E] fp32 / f16 / bf16 tensor with unit column stride")
    if not pred_in.is_cuda:
        raise ValueError("zett_amd computes on the GPU only: pred_in must be a cuda (ROCm) tensor; there is no CPU path")
    if input_ids.dtype not in (torch.int32, torch.int64) or input_ids.device != pred_in.device:
        raise ValueError("input_ids must be an int32 / int64 tensor on the device of pred_in")
    dtype = pred_in.dtype if dtype is None else dtype
    if dtype not in zett_dtypes():
        raise ValueError(f"dtype must be torch.float32, torch.float16 or torch.bfloat16, got {dtype!r}")
    ids = input_ids.detach().contiguous()
    if torch.is_grad_enabled() and pred_in.requires_grad:
        if pred_in.dtype != torch.float32:
            raise ValueError("the gradient of token_embeddings is defined for an fp32 pred_in; a 16-bit pred_in must not require grad")
        return _TokenEmbeddings.apply(pred_in, ids, dtype, bool(check_ids))
    return _lookup(pred_in.detach(), ids, dtype, bool(check_ids))


# ---- the batch's sub-vocabulary (collator.py:207-282) ------------------------------------------------------------------------
class BatchVocabulary(NamedTuple):
    """What subsample_batch_vocabulary returns: the collator's arrays, on the device."""
    input_ids: torch.Tensor                  # remapped to rows of ids_to_embed; shape and dtype as given
    labels: torch.Tensor                     # likewise, -100 kept
    ids_to_embed: torch.Tensor               # [N], dtype of input_ids
    target_surface_forms: torch.Tensor       # [N, L]
    target_priors: torch.Tensor              # [N] fp32
    mask: torch.Tensor                       # [N] bool, all true
    special_indices: List[int]               # host list: the row of each special id, in special_ids' order (what splice_special_rows takes)
    n_positive: torch.Tensor                 # device int32 scalar: specials + distinct other ids of the batch
    status: torch.Tensor                     # device int32 scalar: 0, or an OR of the BATCH_* bits


BATCH_BAD_ID, BATCH_OVERFLOW, BATCH_BAD_ORDER, BATCH_REPEAT = _lib.BATCH_BAD_ID, _lib.BATCH_OVERFLOW, _lib.BATCH_BAD_ORDER, _lib.BATCH_REPEAT
_BATCH_MODES = {"positives_only": _lib.BATCH_POSITIVES_ONLY, "random": _lib.BATCH_RANDOM}


def special_row_moves(special_ids: Sequence[int], n: int) -> Tuple[List[Tuple[int, int]], List[int]]:
    """The collator's "try to preserve special token indices" loop (collator.py:251-254) as data: ``(moves, special_indices)``.

    The list starts with ``special_ids`` in their own order in rows ``0 .. len - 1``.  For each special id in ASCENDING order its row is
    deleted and the id inserted at row ``min(id, n - 1)`` (Python's ``del`` / ``insert`` on a list of n entries); ``moves[m] = (from, to)``
    is that step for the m-th smallest id, and ``special_indices[i]`` the final row of ``special_ids[i]``.  Both depend on nothing but
    ``special_ids`` and n: only the specials' own rows have to be followed, O(len^2).  ValueError for a negative or repeated id or
    more ids than rows."""
    ids = [int(s) for s in special_ids]
    n = int(n)
    if len(set(ids)) != len(ids):
        raise ValueError("special_ids holds an id twice")
    if any(s < 0 for s in ids):
        raise ValueError("special_ids holds a negative id")
    if len(ids) > n:
        raise ValueError(f"{len(ids)} special ids do not fit n_token_subsample = {n} rows")
    row = {s: i for i, s in enumerate(ids)}
    moves = []
    for s in sorted(ids):
        frm, to = row[s], min(s, n - 1)
        for other, r in row.items():
            r -= 1 if r > frm else 0
            r += 1 if r >= to else 0
            row[other] = r
        row[s] = to
        moves.append((frm, to))
    return moves, [row[s] for s in ids]


def batch_vocab_workspace(t: int, v: int, n: int) -> int:
    """bytes of the scratch buffer of subsample_batch_vocabulary for t positions, v ids, n rows"""
    out = C.c_int64(0)
    _lib.check(_lib.load().zett_op_batch_vocab_workspace_bytes(int(t), int(v), int(n), C.byref(out)), "batch_vocab_workspace_bytes")
    return out.value


def subsample_batch_vocabulary(input_ids, labels, special_ids, n_token_subsample, target_surface_forms, target_priors, *, mode="random", negative_order=None,
                               check=True) -> BatchVocabulary:
    """The ``n_token_subsample`` branch of the reference's collator (collator.py:207-282) on the device: from a batch of token ids to
    the N ids the hypernetwork embeds this step, with the batch remapped to rows of that list.

        bv = subsample_batch_vocabulary(input_ids, labels, tokenizer.all_special_ids, N, surface_forms, priors, negative_order=torch.randperm(V, device=dev))
        pred_in, pred_out, _ = model(bv.target_surface_forms, ...)
        pred_in, pred_out = splice_special_rows(pred_in, pred_out, src, bv.special_indices, special_indices_in_reference, inplace=True)
        hidden = backbone(token_embeddings(pred_in, bv.input_ids))
        loss, _ = lm_head_loss(hidden, pred_out, bv.labels, priors=bv.target_priors, ...)

    input_ids, labels: ``[B, S]`` or ``[T]`` int32 / int64 device tensors of one shape; a label of -100 is "no label".  special_ids: a host
    list, the tokenizer's ``all_special_ids`` in ITS order, at most 256 distinct ids of ``[0, V)``.  target_surface_forms: ``[V, L]`` int32 /
    int64, unit column stride, any row stride >= L.  target_priors: ``[V]`` fp32.  N = n_token_subsample <= V.  negative_order: ``[V]`` int32 /
    int64 on the device, a permutation of ``range(V)`` — the randomness of ``mode="random"``, taken as an argument so that the result is
    a pure function of its inputs.

    1. positives: ascending, the ids that occur in input_ids or in ``labels != -100`` and are not special.  ``tokens_in_batch =
       special_ids ++ positives``, ``n_positive`` its length; ``n_positive > N`` is an error (the reference asserts).
    2. ``N - n_positive`` negatives.  "positives_only": id 0 repeated.  "random": the first entries of negative_order that are not in
       tokens_in_batch, in negative_order's order — the reference's shuffle-then-truncate when negative_order is a uniform permutation.
    3. ``tokens_in_batch ++ negatives``, then the moves of ``special_row_moves(special_ids, N)``: each special id, ascending, goes to row
       ``min(id, N - 1)``.  ``special_indices`` is where each ended up.
    4. ``inv[id]`` = the LARGEST row that holds id (numpy's last write wins for "positives_only"'s repeated id 0); input_ids and the
       labels other than -100 become ``inv[.]``.
    5. target_surface_forms / target_priors: the rows of ids_to_embed; mask: ones.

    Deviations from the reference: a label of -100 is not an id (the reference lets -100 into ``np.unique`` under MLM); in "random" mode
    the negatives exclude ALL of tokens_in_batch (the reference excludes only ``unique(input_ids)``, so it can list a special or label-only
    id twice) — ids_to_embed has no duplicate in "random" mode.  Wherever the reference's own list has no duplicate and no -100 among its
    ids, every output equals the reference's element for element.

    ``status``: 0, or an OR of BATCH_BAD_ID (1: an id of input_ids / labels outside ``[0, V)``), BATCH_OVERFLOW (2: n_positive > N),
    BATCH_BAD_ORDER (4: an entry of negative_order outside ``[0, V)``), BATCH_REPEAT (8, "random": an id listed twice, or too few absent
    ids in negative_order — it is not a permutation).  An id outside ``[0, V)`` is never used as an address; with a bit set the outputs
    are unspecified but every write stays inside them.  check=True reads the word once (the one host read of this call) and raises
    IndexError for bits 1 and 4, ValueError for bits 2 and 8; check=False never waits for the host.

    Integers and a gather of constants: no gradient flows anywhere.  Seven small launches on the current stream (csrc/train_batch.hip), the only
    atomics integer OR and max: the same inputs give the same bits."""
    if mode not in _BATCH_MODES:
        raise ValueError(f"mode must be one of {sorted(_BATCH_MODES)}, got {mode!r} (the reference's \"highest_scores\" is not implemented there either)")
    ints = (torch.int32, torch.int64)
    for name, x in (("input_ids", input_ids), ("labels", labels)):
        if not isinstance(x, torch.Tensor) or x.dtype not in ints or x.dim() not in (1, 2):
            raise ValueError(f"{name} must be a [B, S] or [T] int32 / int64 tensor")
    if input_ids.shape != labels.shape:
        raise ValueError(f"input_ids {tuple(input_ids.shape)} and labels {tuple(labels.shape)} must have the same shape")
    sf, priors = target_surface_forms, target_priors
    if sf.dim() != 2 or sf.dtype not in ints or sf.shape[0] == 0 or sf.shape[1] == 0 or sf.stride(1) != 1 or sf.stride(0) < sf.shape[1]:
        raise ValueError("target_surface_forms must be a non-empty [V, L] int32 / int64 tensor with unit column stride")
    v, l = sf.shape
    if priors.dtype != torch.float32 or priors.shape != (v,):
        raise ValueError(f"target_priors must be an fp32 [{v}] tensor")
    n = int(n_token_subsample)
    if n <= 0 or n > v:
        raise ValueError(f"n_token_subsample = {n} must be in [1, V = {v}]")
    special = [int(s) for s in special_ids]
    if len(special) > _lib.SPLICE_MAX_ROWS:
        raise ValueError(f"special_ids holds {len(special)} entries, at most {_lib.SPLICE_MAX_ROWS} travel with a launch")
    bad = [s for s in special if s < 0 or s >= v]
    if bad:
        raise IndexError(f"special id {bad[0]} is outside [0, {v})")
    moves, special_indices = special_row_moves(special, n)
    if mode == "random":
        if negative_order is None:
            raise ValueError("mode=\"random\" needs negative_order: a permutation of range(V) on the device (torch.randperm)")
        if negative_order.dtype not in ints or negative_order.shape != (v,):
            raise ValueError(f"negative_order must be an int32 / int64 [{v}] tensor")
    device = input_ids.device
    if not input_ids.is_cuda:
        raise ValueError("zett_amd computes on the GPU only: input_ids must be a cuda (ROCm) tensor; there is no CPU path")
    for name, x in (("labels", labels), ("target_surface_forms", sf), ("target_priors", priors), ("negative_order", negative_order if mode == "random" else None)):
        if x is not None and x.device != device:
            raise ValueError(f"{name} must be on the device of input_ids")
    lib = _lib.load()
    ids, lab = input_ids.detach().contiguous(), labels.detach().contiguous()
    priors = priors.detach().contiguous()
    order = negative_order.detach().contiguous() if mode == "random" else None
    t, k = ids.numel(), len(special)
    arrays = [(C.c_int32 * max(k, 1))(*x) for x in (special, [m[0] for m in moves], [m[1] for m in moves])]
    with torch.cuda.device(device):
        out_ids, out_lab = torch.empty_like(ids), torch.empty_like(lab)
        ids_to_embed = torch.empty(n, dtype=ids.dtype, device=device)
        out_sf = torch.empty((n, l), dtype=sf.dtype, device=device)
        out_priors = torch.empty(n, dtype=torch.float32, device=device)
        mask = torch.empty(n, dtype=torch.bool, device=device)
        words = torch.empty(2, dtype=torch.int32, device=device)          # n_positive, status: both written by the call
        work = torch.empty(batch_vocab_workspace(t, v, n) // 4, dtype=torch.int32, device=device)          # (released on return: the allocator reuses it in stream order)
        _lib.check(lib.zett_op_batch_vocab(ptr(ids), ids.element_size(), ptr(lab), lab.element_size(), t, v, n, ptr(sf), sf.element_size(), sf.stride(0), l,
                                           ptr(priors), ptr(order), 0 if order is None else order.element_size(), _BATCH_MODES[mode], *arrays, k, ptr(out_ids),
                                           ptr(out_lab), ptr(ids_to_embed), ptr(out_sf), ptr(out_priors), ptr(mask), ptr(words[0]), ptr(words[1]), ptr(work),
                                           work.numel() * 4, stream(device)), "batch_vocab")
    if check:
        bits = int(words[1].item())          # (the one host read of this call)
        if bits & BATCH_BAD_ID:
            raise IndexError(f"subsample_batch_vocabulary: an id of input_ids / labels is outside [0, {v})")
        if bits & BATCH_BAD_ORDER:
            raise IndexError(f"subsample_batch_vocabulary: an entry of negative_order is outside [0, {v})")
        if bits & BATCH_OVERFLOW:
            raise ValueError(f"subsample_batch_vocabulary: the batch holds {int(words[0].item())} ids with the specials, more than n_token_subsample = {n}")
        if bits & BATCH_REPEAT:
            raise ValueError("subsample_batch_vocabulary: ids_to_embed lists an id twice: negative_order is not a permutation of range(V)")
    return BatchVocabulary(out_ids, out_lab, ids_to_embed, out_sf, out_priors, mask, special_indices, words[0], words[1])


# ---- from texts to the batch's ids (collator.py:166-178): zett_amd/text_encode.py, re-exported beside subsample_batch_vocabulary ---------
from .text_encode import DeviceTextEncoder, encode_texts  # noqa: E402,F401
# ---- a step's tokenizer sampled from the batch (collator.py:341-452): zett_amd/tokenizer_sampling.py ---------------------------------------
from .tokenizer_sampling import DeviceTokenizerSampler, sample_tokenizer  # noqa: E402,F401
# ---- that tokenizer's vocabulary and encoder tables without the host Tokenizer: zett_amd/sampled_vocab.py -------------------------------------
from .sampled_vocab import DeviceSampledVocabulary, SampledVocabulary, sample_tokenizer_device  # noqa: E402,F401
# ---- the rest of the collator (collator.py:180-205, 283-337, 454-537): zett_amd/collate.py --------------------------------------------------------
from .collate import DeviceCollator, LabelledBatch, PaddedVocabulary, label_batch, mlm_thresholds, pad_vocabulary, padded_rows  # noqa: E402,F401


# ---- the parameter update (train.py:591-656): labels, the step skeleton, AdamW, Adafactor, make_optimizer: zett_amd/optim.py ----------------------
from .optim import ADAFACTOR_MIN_DIM_TO_FACTOR, LABELS, HypernetAdafactor, HypernetAdamW, HypernetOptimizer, adafactor_state_shapes, make_optimizer, param_labels  # noqa: E402,F401


# ---- fitting a fresh hypernetwork's Rescalers (csrc/train_init.hip) ------------------------------------------------------------------
COL_MOMENTS_CHUNK = _lib.COL_MOMENTS_CHUNK          # rows of one partial of column_moments: part of the definition of its result


class ColumnMoments(NamedTuple):
    """Per-column count, mean and M2 = sum (x - mean)^2 of the rows fed so far: ``state`` is the device record of
    include/zett_hip.h, a contiguous float64 ``[C, 3]`` tensor (count, mean, M2 per column)."""
    state: torch.Tensor

    @property
    def cols(self) -> int:
        return self.state.shape[0]

    @property
    def count(self) -> torch.Tensor:
        return self.state[:, 0].to(torch.float32)

    def mean(self) -> torch.Tensor:
        return self.state[:, 1].to(torch.float32)

    def std(self) -> torch.Tensor:
        """the population std (ddof = 0), as ``jnp.std``"""
        return (self.state[:, 2].clamp_min(0.0) / self.state[:, 0]).sqrt().to(torch.float32)

    def columns(self, c0: int, c1: int) -> "ColumnMoments":
        """The moments of columns [c0, c1): a view, no pass over the matrix.  Accumulating into the view accumulates into this state."""
        if not 0 <= c0 < c1 <= self.cols:
            raise ValueError(f"columns [{c0}, {c1}) are outside the {self.cols} columns of the state")
        return ColumnMoments(self.state[c0:c1])


def _check_state(m, what):
    s = m.state if isinstance(m, ColumnMoments) else None
    if s is None or s.dim() != 2 or s.shape[1] != 3 or s.shape[0] < 1 or s.dtype != torch.float64 or not s.is_contiguous():
        raise ValueError(f"{what} must be a ColumnMoments over a contiguous float64 [C, 3] state")
    return s


def column_moments(x, *, col0: int = 0, cols: Optional[int] = None, state: Optional[ColumnMoments] = None) -> ColumnMoments:
    """Count, mean and M2 of columns [col0, col0 + cols) of the [R, C] fp32 / f16 / bf16 device matrix ``x`` in one read of it
    (zett_op_col_moments: chunks of COL_MOMENTS_CHUNK rows, merged in order; the same call gives the same bits on every run).
    ``state=``: the rows are merged into that state (Chan's update), which is returned: predicted rows can be fed chunk by chunk.
    R = 0 is allowed; a state that holds no row is refused by rescaler_fit."""
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype not in zett_dtypes() or not x.is_cuda or (x.shape[1] > 1 and x.stride(1) != 1):
        raise ValueError("x must be a [R, C] fp32 / f16 / bf16 device tensor with unit column stride")
    rows, width = x.shape
    cols = width - col0 if cols is None else int(cols)
    if col0 < 0 or cols < 1 or col0 + cols > width:
        raise ValueError(f"columns [{col0}, {col0 + cols}) are outside x {tuple(x.shape)}")
    ld = x.stride(0) if rows > 1 else max(x.stride(0), width)
    if ld < width:
        raise ValueError("x must be row-major: its row stride is below its width")
    if state is not None:
        s = _check_state(state, "state")
        if s.shape[0] != cols or s.device != x.device:
            raise ValueError(f"state holds {s.shape[0]} columns on {s.device}, the call is over {cols} columns on {x.device}")
    else:
        s = torch.empty((cols, 3), dtype=torch.float64, device=x.device)
    lib = _lib.load()
    need = C.c_int64(0)
    _lib.check(lib.zett_op_col_moments_workspace_bytes(rows, cols, C.byref(need)), "col_moments_workspace_bytes")
    with torch.cuda.device(x.device):
        workspace = torch.empty(need.value // 8, dtype=torch.float64, device=x.device)
        _lib.check(lib.zett_op_col_moments(ptr(x), zett_dtypes()[x.dtype], ld, rows, int(col0), cols, ptr(s), int(state is not None), ptr(workspace), need.value,
                                           stream(x.device)), "col_moments")
    return state if state is not None else ColumnMoments(s)


def rescaler_fit(x_moments: ColumnMoments, target: Optional[ColumnMoments] = None, *, target_std: Optional[float] = None,
                 target_mean: Optional[float] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """``Rescaler.scale_to`` (zett/utils.py:165-175) from moments: w = t_std / (std(x) + 1e-8), b = t_mean - w * mean(x), both fp32
    ``[1, C]``, ready to copy into a Rescaler.  The target is the moments of a matrix of the same width, or two scalars for every column
    (``target_std=embed_init_range, target_mean=0``: in_scaler).  Waits for the stream once: a state without rows raises ValueError."""
    xs = _check_state(x_moments, "x_moments")
    if (target is None) == (target_std is None and target_mean is None) or (target is None and (target_std is None or target_mean is None)):
        raise ValueError("give either target (ColumnMoments) or both target_std and target_mean")
    ts = None
    if target is not None:
        ts = _check_state(target, "target")
        if ts.shape[0] != xs.shape[0] or ts.device != xs.device:
            raise ValueError(f"target holds {ts.shape[0]} columns on {ts.device}, x_moments {xs.shape[0]} on {xs.device}")
    if not xs.is_cuda:
        raise ValueError("zett_amd computes on MI355X only: the states must live on a cuda (ROCm) device")
    out = torch.empty((2, 1, xs.shape[0]), dtype=torch.float32, device=xs.device)
    with torch.cuda.device(xs.device):
        _lib.check(_lib.load().zett_op_rescaler_fit(ptr(xs), xs.shape[0], ptr(ts), float(target_std or 0.0), float(target_mean or 0.0), ptr(out[0]), ptr(out[1]),
                                                    stream(xs.device)), "rescaler_fit")
    return out[0], out[1]


# The modules train.py:705-718 re-initialises with reinit_projectors: the first component of a parameter's name.  The reference's list
# has no out_scaler (and, matching on the whole component, no output_projection_out): a pretrained out_scaler survives.  Kept as it is.
REINIT_PROJECTOR_MODULES = ("fallback_embeddings", "input_projection", "output_projection", "bias_projection", "scaler", "in_scaler")


def split_pretrained_state(pretrained_state: Mapping[str, torch.Tensor], reinit_projectors: bool):
    """-> (the entries to overlay, the names dropped): with reinit_projectors the keys under REINIT_PROJECTOR_MODULES are dropped."""
    kept, dropped = {}, []
    for name, value in pretrained_state.items():
        if reinit_projectors and name.split(".", 1)[0] in REINIT_PROJECTOR_MODULES:
            dropped.append(name)
        else:
            kept[name] = value
    return kept, dropped


def init_hypernet_state(model, source_embeddings, example_surface_forms, *, pretrained_state: Optional[Mapping[str, torch.Tensor]] = None,
                        reinit_projectors: bool = False) -> List[str]:
    """The hypernetwork's half of the reference's ``init_state`` (train.py:689-725) on a freshly constructed ``model``: fit the Rescalers
    on ``example_surface_forms`` (ZettHypernet.init_rescaler, language 0 as the reference), then overlay ``pretrained_state`` — a state
    dict of hypernetwork parameters, which need not be complete — without the projector modules when ``reinit_projectors`` is set.
    Returns the names that were dropped.  A name the model does not have raises KeyError before anything is overlaid."""
    model.init_rescaler(example_surface_forms, source_embeddings)
    if not pretrained_state:
        return []
    kept, dropped = split_pretrained_state(pretrained_state, reinit_projectors)
    params = dict(model.named_parameters())
    unknown = [n for n in kept if n not in params]
    if unknown:
        raise KeyError(f"pretrained parameters the model does not have: {unknown}")
    for name, value in kept.items():
        if tuple(value.shape) != tuple(params[name].shape):
            raise ValueError(f"pretrained {name} has shape {tuple(value.shape)}, the model's is {tuple(params[name].shape)}")
    with torch.no_grad():
        for name, value in kept.items():
            params[name].copy_(value)          # (through the parameter: the engines notice, ZettHypernet.refresh_weights)
    return dropped
