"""The hypernetwork side of the reference's trainer around the differentiable forward (zett_amd/autograd.py): the identity
warm-up loss (train.py:914-975), the lexical loss (train.py:1074-1141) and the parameter update of
``optax.chain(clip_by_global_norm(max_grad_norm), multi_transform({train: adamw, freeze: set_to_zero}))`` (train.py:591-656).

    opt = HypernetAdamW(model, lr=6e-5)
    pred_in, pred_out, _ = model(ids, source_embeddings=src, lang_index=lang)       # model.train(), parameters require grad
    loss = identity_loss(pred_in, pred_out, src, ids_to_embed)
    loss.backward()
    opt.step(lr=schedule(step), zero_grad=True)

Losses and update are HIP kernels (csrc/train_step.hip); torch holds the tensors and the tape.  Nothing in this module waits for
the host except ``last_step_stats()`` and ``state_dict()`` (the model's forward in front of it still reads its id range back once per
step).  Results are bit-reproducible from run to run.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, Mapping, Optional, Union

import torch

from . import _lib

_KINDS = {"mse": _lib.DIST_MSE, "rmse": _lib.DIST_RMSE, "huber": _lib.DIST_HUBER}
_SRC_DTYPES = {torch.float32: _lib.DTYPE_F32, torch.float16: _lib.DTYPE_F16, torch.bfloat16: _lib.DTYPE_BF16}


def _ptr(t: Optional[torch.Tensor]):
    return C.c_void_p(0 if t is None else t.data_ptr())


def _stream(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ---- the three kernels of an embedding distance ---------------------------------------------------------------------------
def _dist_args(pred, src, col0, ids, ids_stride, mask, kind):
    if kind not in _KINDS:
        raise ValueError(f"kind must be one of {sorted(_KINDS)}, got {kind!r}")
    if pred.dim() != 2 or pred.dtype != torch.float32 or pred.stride(1) != 1 or not pred.is_cuda:
        raise ValueError("predicted embeddings must be a [n, E] fp32 device tensor with unit column stride")
    if src.dim() != 2 or src.dtype not in _SRC_DTYPES or src.stride(1) != 1 or src.device != pred.device:
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
    return (_ptr(pred), pred.stride(0), _ptr(src), _SRC_DTYPES[src.dtype], src.stride(0), src.shape[0], int(col0), _ptr(ids), ids.element_size(), int(ids_stride),
            _ptr(mask)), n, e


def embed_distance_forward(pred, src, col0, ids, ids_stride=1, mask=None, kind="mse", mode=_lib.LOSS_MEAN):
    """Rows pass + finalise.  Returns (record, row_dist, row_tnorm): record = [loss, gradient scale, masked-row fraction, 0] on the
    device; the target of row r is ``src[clamp(ids[r * ids_stride], 0, len(src) - 1), col0 : col0 + E]``."""
    lib = _lib.load()
    head, n, e = _dist_args(pred, src, col0, ids, ids_stride, mask, kind)
    with torch.cuda.device(pred.device):
        rows = torch.empty((2, n), dtype=torch.float32, device=pred.device)
        record = torch.empty(4, dtype=torch.float32, device=pred.device)
        st = _stream(pred.device)
        _lib.check(lib.zett_op_embed_dist_rows(*head, n, e, _KINDS[kind], _ptr(rows[0]), _ptr(rows[1]), st), "embed_dist_rows")
        _lib.check(lib.zett_op_embed_dist_finalize(_ptr(rows[0]), _ptr(rows[1]), _ptr(mask), n, int(mode), _ptr(record), st), "embed_dist_finalize")
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
        _lib.check(lib.zett_op_embed_dist_grad(*head, _ptr(row_dist), n, e, _KINDS[kind], _ptr(record), _ptr(upstream), _ptr(out), out.stride(0),
                                               int(bool(accumulate)), _stream(pred.device)), "embed_dist_grad")
    return out


def single_token_mask(target_surface_forms: torch.Tensor, pad_token_id: int) -> torch.Tensor:
    """fp32 [n]: 1 where every position after the first is pad (lexical_overlap_mask, train.py:1092-1094), on the device."""
    ids = target_surface_forms
    if ids.dim() != 2 or ids.dtype not in (torch.int32, torch.int64) or ids.stride(1) != 1 or not ids.is_cuda:
        raise ValueError("target_surface_forms must be a [n, L] int32 / int64 device tensor with unit column stride")
    mask = torch.empty(ids.shape[0], dtype=torch.float32, device=ids.device)
    with torch.cuda.device(ids.device):
        _lib.check(_lib.load().zett_op_single_token_mask(_ptr(ids), ids.element_size(), ids.shape[0], ids.shape[1], ids.stride(0), int(pad_token_id), _ptr(mask),
                                                         _stream(ids.device)), "single_token_mask")
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
    src = source_embeddings if source_embeddings.dtype in _SRC_DTYPES else source_embeddings.float()
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


# ---- which parameters train, and which decay -------------------------------------------------------------------------------
LABELS = ("decay", "no_decay", "frozen")


def param_labels(model, overrides: Union[None, Mapping[str, str], Callable[[str], Optional[str]]] = None) -> Dict[str, str]:
    """name -> "decay" | "no_decay" | "frozen" for every parameter of `model`: the reference's rule (train.py:591-622) on the
    checkpoint's PyTorch names.

    - frozen: ``scaler.*`` and ``in_scaler.*`` (get_labels: a path whose parent is "scaler" or "in_scaler").  ``out_scaler.*`` is
      NOT in the reference's freeze set, so it trains — and decays: its leaves are called "w" and "b", not "bias".  Kept as is.
    - no_decay: every ``.bias`` and every parameter of a LayerNorm (``LayerNorm.*``, ``ln.*``) (decay_mask_fn).
    - decay: everything else.

    overrides: a mapping (exact name, or a prefix ending in "." for a whole module) or a callable name -> label | None."""
    out = {}
    for name, _ in model.named_parameters():
        parts = name.split(".")
        if len(parts) >= 2 and parts[-2] in ("scaler", "in_scaler"):
            label = "frozen"
        elif parts[-1] == "bias" or (len(parts) >= 2 and parts[-2] in ("LayerNorm", "ln", "layer_norm", "layernorm")):
            label = "no_decay"
        else:
            label = "decay"
        if callable(overrides):
            label = overrides(name) or label
        elif overrides:
            for key, value in overrides.items():
                if name == key or (key.endswith(".") and name.startswith(key)):
                    label = value
        if label not in LABELS:
            raise ValueError(f"label of {name} must be one of {LABELS}, got {label!r}")
        out[name] = label
    return out


class HypernetAdamW:
    """optax.chain(clip_by_global_norm(max_grad_norm), multi_transform({train: adamw(lr, b1, b2, eps, weight_decay, mask),
    freeze: set_to_zero})) (train.py:638-656) for the parameters of `model`, as two multi-tensor HIP kernels per step:

    - the global gradient norm over EVERY parameter that has a gradient, frozen ones included (the reference clips before the
      freeze), then ``coef = 1 if norm < max_grad_norm else max_grad_norm / norm`` (optax's rule; max_grad_norm None: no clip);
    - one pass: ``g' = coef g; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2; p -= lr ((m/c1) / (sqrt(v/c2) + eps) + wd p)``,
      weight decay on "decay" parameters only (param_labels), "frozen" parameters untouched.

    A step whose gradient norm is not finite changes no parameter, no moment and not the step count, and is reported by
    ``last_step_stats()["skipped"]``.  With ``zero_grad=True`` it still clears every gradient, so that the non-finite values are not
    what the next backward accumulates into (every later step would be skipped too); without it the caller clears them.

    `model` is a ZettHypernet or a wrapper that holds one as ``.module`` (DistributedDataParallel): the wrapper is unwrapped.  step() does not wait for the host: norm, coefficient, skip flag and step count live in a
    device record.  It ends with ``model.refresh_weights()`` — the kernels write through raw pointers, which torch's version
    counters do not see — so a no_grad / eval forward after it runs on the new weights."""

    def __init__(self, model, lr: float, betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 0.01, max_grad_norm: Optional[float] = 0.1,
                 labels: Union[None, Mapping[str, str], Callable[[str], Optional[str]]] = None):
        if not hasattr(model, "refresh_weights") and hasattr(getattr(model, "module", None), "refresh_weights"):
            model = model.module                              # DistributedDataParallel and the like: the same Parameter objects
        if not hasattr(model, "refresh_weights"):
            raise TypeError("HypernetAdamW needs a model with refresh_weights() (a ZettHypernet, or a wrapper holding one as .module)")
        self.model = model
        self._set_hyper(lr, betas, eps, weight_decay, max_grad_norm)
        self.labels = param_labels(model, labels)
        self.state: Dict[str, Dict[str, torch.Tensor]] = {}
        self._record: Optional[torch.Tensor] = None          # [norm, coef, skip (i32), step (i32), 1 - b1^step, 1 - b2^step, 0, 0]
        self._partials: Optional[torch.Tensor] = None

    def _set_hyper(self, lr, betas, eps, weight_decay, max_grad_norm) -> None:
        betas = (float(betas[0]), float(betas[1]))
        max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or float(eps) < 0 or (max_grad_norm is not None and not max_grad_norm > 0):
            raise ValueError("betas must be in [0, 1), eps >= 0, max_grad_norm > 0 or None")
        self.lr, self.betas, self.eps, self.weight_decay, self.max_grad_norm = float(lr), betas, float(eps), float(weight_decay), max_grad_norm

    def _params(self):
        return [(n, p) for n, p in self.model.named_parameters() if p.grad is not None]

    def _device_record(self, device) -> torch.Tensor:
        if self._record is None or self._record.device != device:
            old = self._record
            self._record = torch.zeros(8, dtype=torch.float32, device=device)
            if old is not None:
                self._record.copy_(old)
        return self._record

    def _collect(self):
        """The tensor lists of this step as host arrays (they travel to the kernels as launch arguments), moments allocated."""
        todo = self._params()
        if not todo:
            return None
        device = todo[0][1].device
        n = len(todo)
        P, G, M, V = ((C.c_void_p * n)() for _ in range(4))
        numel, flags = (C.c_int64 * n)(), (C.c_uint8 * n)()
        items = 0
        for i, (name, p) in enumerate(todo):
            g = p.grad
            if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous() or not g.is_contiguous() or p.device != device or g.device != device:
                raise ValueError(f"{name}: parameters and gradients must be contiguous fp32 tensors on one device")
            label = self.labels.get(name, "decay")
            P[i], G[i], numel[i] = p.data_ptr(), g.data_ptr(), p.numel()
            items += -(-p.numel() // _lib.MT_CHUNK)
            if label == "frozen":
                flags[i] = _lib.ADAMW_FROZEN
                continue
            st = self.state.get(name)
            if st is None:
                st = self.state[name] = {k: torch.zeros_like(p, memory_format=torch.contiguous_format) for k in ("exp_avg", "exp_avg_sq")}
            elif st["exp_avg"].device != device:
                st = self.state[name] = {k: t.to(device) for k, t in st.items()}
            M[i], V[i] = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()
            flags[i] = _lib.ADAMW_DECAY if label == "decay" else 0
        if self._partials is None or self._partials.numel() < items or self._partials.device != device:
            self._partials = torch.empty(max(items, 1), dtype=torch.float32, device=device)
        return device, n, P, G, M, V, numel, flags, self._device_record(device)

    def _launch_norm(self, lists) -> None:
        device, n, _, G, _, _, numel, _, record = lists
        with torch.cuda.device(device):
            _lib.check(_lib.load().zett_op_grad_norm(G, numel, n, math.inf if self.max_grad_norm is None else float(self.max_grad_norm), self.betas[0], self.betas[1],
                                                     _ptr(self._partials), self._partials.numel(), _ptr(record), _stream(device)), "grad_norm")

    def _launch_adamw(self, lists, lr: Optional[float] = None, zero_grad: bool = False) -> None:
        device, n, P, G, M, V, numel, flags, record = lists
        with torch.cuda.device(device):
            _lib.check(_lib.load().zett_op_adamw(P, G, M, V, numel, flags, n, self.lr if lr is None else float(lr), self.betas[0], self.betas[1], self.eps,
                                                 self.weight_decay, int(bool(zero_grad)), _ptr(record), _stream(device)), "adamw")

    def step(self, lr: Optional[float] = None, zero_grad: bool = False) -> None:
        """One update from the parameters' ``.grad``.  lr: this step's learning rate (the caller's schedule); zero_grad: the
        gradients are zeroed in the same pass (they stay allocated: the next backward accumulates into zeros) — on a skipped
        step too."""
        lists = self._collect()
        if lists is None:
            return
        self._launch_norm(lists)
        self._launch_adamw(lists, lr, zero_grad)
        self.model.refresh_weights()

    def zero_grad(self, set_to_none: bool = True) -> None:
        self.model.zero_grad(set_to_none=set_to_none)

    def last_step_stats(self) -> Dict[str, float]:
        """Synchronises.  grad_norm: the global norm before clipping; clip_coef: what the gradients were multiplied by; skipped: 1 if
        the norm was not finite and the step changed nothing; step: updates applied so far."""
        if self._record is None:
            return {"grad_norm": 0.0, "clip_coef": 1.0, "skipped": 0, "step": 0}
        f = self._record.cpu()
        i = f.view(torch.int32)
        return {"grad_norm": float(f[0]), "clip_coef": float(f[1]), "skipped": int(i[2]), "step": int(i[3])}

    def state_dict(self) -> dict:
        return {"step": self.last_step_stats()["step"],
                "state": {n: {k: t.clone() for k, t in st.items()} for n, st in self.state.items()},
                "hyper": {"lr": self.lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay, "max_grad_norm": self.max_grad_norm},
                "labels": dict(self.labels)}

    def load_state_dict(self, sd: dict) -> None:
        """What state_dict() returned: "step" and "state" are required; "hyper" and "labels" (optional) replace the constructor's."""
        missing = [k for k in ("step", "state") if k not in sd]
        if missing:
            raise KeyError(f"optimizer state dict lacks {missing}")
        step = int(sd["step"])
        if step < 0:
            raise ValueError(f"step count {step} is negative")
        params = dict(self.model.named_parameters())
        unknown = [n for n in sd["state"] if n not in params]
        if unknown:
            raise KeyError(f"optimizer state for parameters the model does not have: {unknown}")
        state = {}
        for n, st in sd["state"].items():
            p = params[n]
            if tuple(st["exp_avg"].shape) != tuple(p.shape) or tuple(st["exp_avg_sq"].shape) != tuple(p.shape):
                raise ValueError(f"optimizer state of {n} does not match the parameter's shape {tuple(p.shape)}")
            state[n] = {k: st[k].detach().to(device=p.device, dtype=torch.float32).contiguous().clone() for k in ("exp_avg", "exp_avg_sq")}
        labels = param_labels(self.model, {n: l for n, l in sd["labels"].items() if n in self.labels}) if "labels" in sd else self.labels
        h = sd.get("hyper", {})
        self._set_hyper(h.get("lr", self.lr), h.get("betas", self.betas), h.get("eps", self.eps), h.get("weight_decay", self.weight_decay),
                        h.get("max_grad_norm", self.max_grad_norm))          # (validated like the constructor's; nothing was assigned before this)
        self.state, self.labels = state, labels
        device = next(iter(params.values())).device
        record = torch.zeros(8, dtype=torch.float32)
        record.view(torch.int32)[3] = step
        record[1] = 1.0
        self._record = record.to(device) if device.type == "cuda" else record
