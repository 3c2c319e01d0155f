"""The parameter update of the reference's trainer, ``optax.chain(clip_by_global_norm(max_grad_norm), multi_transform({train: adamw |
adafactor, freeze: set_to_zero}))`` (train.py:591-656), on the device: which parameters train and which decay (param_labels), one step
skeleton (HypernetOptimizer), its two updates HypernetAdamW (csrc/train_step.hip) and HypernetAdafactor (csrc/train_adafactor.hip; both
on csrc/train_optim.hip.h), and make_optimizer for the reference's TrainingArguments.  zett_amd/training.py re-exports all of it."""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, Mapping, Optional, Tuple, Union

import torch

from . import _lib
from ._glue import ptr, stream

# ---- which parameters train, and which decay -------------------------------------------------------------------------------
LABELS = ("decay", "no_decay", "frozen")
LabelOverrides = Union[None, Mapping[str, str], Callable[[str], Optional[str]]]


def param_labels(model, overrides: LabelOverrides = None) -> Dict[str, str]:
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


class HypernetOptimizer:
    """What HypernetAdamW and HypernetAdafactor share: everything of a step but the update rule.

    - The global gradient norm is taken over EVERY parameter that has a gradient, frozen ones included (the reference clips before the
      freeze), then ``coef = 1 if norm < max_grad_norm else max_grad_norm / norm`` (optax's rule; max_grad_norm None: no clip).  Weight
      decay acts on "decay" parameters only (param_labels), "frozen" parameters are untouched.
    - A step whose gradient norm is not finite changes no parameter, no state and not the step count, and is reported by
      ``last_step_stats()["skipped"]``.  With ``zero_grad=True`` it still clears every gradient, so that the non-finite values are not
      what the next backward accumulates into (every later step would be skipped too); without it the caller clears them.
    - `model` is a ZettHypernet or a wrapper that holds one as ``.module`` (DistributedDataParallel): the wrapper is unwrapped.  step() does
      not wait for the host: norm, coefficient, skip flag and step count live in a device record (``record``).  It ends with
      ``model.refresh_weights()`` — the kernels write through raw pointers, which torch's version counters do not see.
    - ValueError, before anything is launched: a parameter or gradient that is not a contiguous fp32 tensor on the one device, and a
      parameter that has a gradient and no label (one added to the model after the optimizer was built).

    A subclass names its hyper-parameters (HYPER: attributes, and the keys of ``state_dict()["hyper"]``) and validates them (_set_hyper),
    gives a parameter's state (STATE_KEYS, _state_shapes), may bound its dimensions (MAX_DIM), and makes its library call (_lists, _launch)."""

    HYPER: Tuple[str, ...] = ("lr", "weight_decay", "max_grad_norm")
    MAX_DIM: Optional[int] = None          # parameters of more dimensions are refused

    def __init__(self, model, labels: LabelOverrides = None, **hyper):
        if not hasattr(model, "refresh_weights") and hasattr(getattr(model, "module", None), "refresh_weights"):
            model = model.module                              # DistributedDataParallel and the like: the same Parameter objects
        if not hasattr(model, "refresh_weights"):
            raise TypeError(f"{type(self).__name__} needs a model with refresh_weights() (a ZettHypernet, or a wrapper holding one as .module)")
        self.model = model
        self._set_hyper(**hyper)
        self.labels = param_labels(model, labels)
        self.state: Dict[str, Dict[str, torch.Tensor]] = {}
        self._record: Optional[torch.Tensor] = None          # [norm, coef, skip (i32), step (i32), two words of the subclass, 0, 0]

    def _set_hyper(self, lr, weight_decay, max_grad_norm) -> None:
        """Validates, then assigns: a subclass checks its own values before it calls this, and assigns them after."""
        max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError("max_grad_norm must be > 0 or None")
        self.lr, self.weight_decay, self.max_grad_norm = float(lr), float(weight_decay), max_grad_norm

    def _params(self):
        return [(n, p) for n, p in self.model.named_parameters() if p.grad is not None]

    @property
    def record(self) -> Optional[torch.Tensor]:
        """The eight 32-bit words the last step() or load_state_dict left on the parameters' device, or None before either: [grad norm,
        clip coefficient, skipped (int32), step count (int32), ...].  Reading it does not wait for the host; the next step overwrites it."""
        return self._record

    def _device_record(self, device) -> torch.Tensor:
        if self._record is None or self._record.device != device:
            old = self._record
            self._record = torch.zeros(8, dtype=torch.float32, device=device)
            if old is not None:
                self._record.copy_(old)
        return self._record

    def collect(self):
        """The tensor lists of this step as host arrays (they travel to the kernels as launch arguments), states and scratch allocated;
        None when no parameter has a gradient.  Valid for a launch as long as no parameter, gradient or state tensor is replaced."""
        todo = self._params()
        if not todo:
            return None
        device = todo[0][1].device
        max_dim = self.MAX_DIM
        for name, p in todo:
            if max_dim is not None and p.dim() > max_dim:
                raise ValueError(f"{name}: {type(self).__name__} takes parameters of at most {max_dim} dimensions, got shape {tuple(p.shape)}")
            g = p.grad
            if p.dtype != torch.float32 or g.dtype != torch.float32 or not p.is_contiguous() or not g.is_contiguous() or p.device != device or g.device != device:
                raise ValueError(f"{name}: parameters and gradients must be contiguous fp32 tensors on one device")
            if name not in self.labels:
                raise ValueError(f"{name} has no label")
        n = len(todo)
        P, G, numel, flags = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_int64 * n)(), (C.c_uint8 * n)()
        S = {k: (C.c_void_p * n)() for k in self.STATE_KEYS}          # one pointer list per state tensor a parameter can keep; NULL where it keeps none
        for i, (name, p) in enumerate(todo):
            label = self.labels[name]
            P[i], G[i], numel[i] = p.data_ptr(), p.grad.data_ptr(), p.numel()
            if label == "frozen":
                flags[i] = _lib.ADAMW_FROZEN
                continue
            flags[i] = _lib.ADAMW_DECAY if label == "decay" else 0
            st = self.state.get(name)
            if st is None:
                st = self.state[name] = {k: torch.zeros(shape, dtype=torch.float32, device=device) for k, shape in self._state_shapes(p).items()}
            elif next(iter(st.values())).device != device:
                st = self.state[name] = {k: t.to(device) for k, t in st.items()}
            for k, t in st.items():
                S[k][i] = t.data_ptr()
        return self._lists(device, n, P, G, S, numel, flags, todo, self._device_record(device))

    def step(self, lr: Optional[float] = None, zero_grad: bool = False) -> None:
        """One update from the parameters' ``.grad``.  lr: this step's learning rate (the caller's schedule); zero_grad: the gradients
        are zeroed in the same pass (they stay allocated: the next backward accumulates into zeros) — on a skipped step too."""
        lists = self.collect()
        if lists is None:
            return
        self._launch(lists, lr, zero_grad)
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
                "hyper": {k: getattr(self, k) for k in self.HYPER},
                "labels": dict(self.labels)}

    def load_state_dict(self, sd: dict) -> None:
        """What state_dict() returned: "step" and "state" are required; "hyper" and "labels" (optional) replace the constructor's.
        Every parameter's state must hold the tensors its shape keeps (_state_shapes).  A refused dict changes nothing."""
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
            want = self._state_shapes(p)
            if set(st) != set(want) or any(tuple(st[k].shape) != want[k] for k in want):
                raise ValueError(f"optimizer state of {n} is {({k: tuple(t.shape) for k, t in st.items()})}, a parameter of shape {tuple(p.shape)} keeps {want}")
            state[n] = {k: st[k].detach().to(device=p.device, dtype=torch.float32).contiguous().clone() for k in want}
        labels = param_labels(self.model, {n: l for n, l in sd["labels"].items() if n in self.labels}) if "labels" in sd else self.labels
        h = sd.get("hyper", {})
        self._set_hyper(**{k: h.get(k, getattr(self, k)) for k in self.HYPER})          # (validated like the constructor's; nothing was assigned before this)
        self.state, self.labels = state, labels
        device = next(iter(params.values())).device
        record = torch.zeros(8, dtype=torch.float32)
        record.view(torch.int32)[3] = step
        record[1] = 1.0
        self._record = record.to(device) if device.type == "cuda" else record


class HypernetAdamW(HypernetOptimizer):
    """optax.chain(clip_by_global_norm(max_grad_norm), multi_transform({train: adamw(lr, b1, b2, eps, weight_decay, mask),
    freeze: set_to_zero})) (train.py:638-656) for the parameters of `model`, as two multi-tensor HIP kernels per step: the gradient norm
    (launch_norm), then one pass (launch_adamw): ``g' = coef g; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2; p -= lr ((m/c1) /
    (sqrt(v/c2) + eps) + wd p)``.  Labels, clip, the skipped step, ``zero_grad`` and the device record: HypernetOptimizer."""

    HYPER = ("lr", "betas", "eps", "weight_decay", "max_grad_norm")
    STATE_KEYS = ("exp_avg", "exp_avg_sq")

    def __init__(self, model, lr: float, betas=(0.9, 0.95), eps: float = 1e-8, weight_decay: float = 0.01, max_grad_norm: Optional[float] = 0.1,
                 labels: LabelOverrides = None):
        super().__init__(model, labels, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        self._partials: Optional[torch.Tensor] = None

    def _set_hyper(self, lr, betas, eps, weight_decay, max_grad_norm) -> None:
        betas = (float(betas[0]), float(betas[1]))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0) or float(eps) < 0:
            raise ValueError("betas must be in [0, 1), eps >= 0")
        super()._set_hyper(lr, weight_decay, max_grad_norm)
        self.betas, self.eps = betas, float(eps)

    def _state_shapes(self, p):
        return {"exp_avg": tuple(p.shape), "exp_avg_sq": tuple(p.shape)}

    def _lists(self, device, n, P, G, S, numel, flags, todo, record):
        items = sum(numel) // _lib.MT_CHUNK + n          # (at least the work items of the list: one partial each)
        if self._partials is None or self._partials.numel() < items or self._partials.device != device:
            self._partials = torch.empty(max(items, 1), dtype=torch.float32, device=device)
        return device, n, P, G, S["exp_avg"], S["exp_avg_sq"], numel, flags, record

    def launch_norm(self, lists) -> None:
        """The first half of step() on what collect() returned: the gradient norm and the record (every call advances its step count)."""
        device, n, _, G, _, _, numel, _, record = lists
        with torch.cuda.device(device):
            _lib.check(_lib.load().zett_op_grad_norm(G, numel, n, math.inf if self.max_grad_norm is None else self.max_grad_norm, self.betas[0], self.betas[1],
                                                     ptr(self._partials), self._partials.numel(), ptr(record), stream(device)), "grad_norm")

    def launch_adamw(self, lists, lr: Optional[float] = None, zero_grad: bool = False) -> None:
        """The second half: the update by the record launch_norm left.  It does not call ``refresh_weights()``; step() does."""
        device, n, P, G, M, V, numel, flags, record = lists
        with torch.cuda.device(device):
            _lib.check(_lib.load().zett_op_adamw(P, G, M, V, numel, flags, n, self.lr if lr is None else float(lr), self.betas[0], self.betas[1], self.eps,
                                                 self.weight_decay, int(bool(zero_grad)), ptr(record), stream(device)), "adamw")

    def _launch(self, lists, lr, zero_grad) -> None:
        self.launch_norm(lists)
        self.launch_adamw(lists, lr, zero_grad)


ADAFACTOR_MIN_DIM_TO_FACTOR = 128      # optax.adafactor's min_dim_size_to_factor


def adafactor_state_shapes(shape) -> Dict[str, Tuple[int, ...]]:
    """The statistics optax.scale_by_factored_rms keeps for a parameter of `shape` (1-D or 2-D): {"v_row", "v_col"} for a factored
    one (2-D, smaller dimension >= 128), {"v"} otherwise.  d0 is the larger and d1 the smaller dimension by ``numpy.argsort(shape)``
    (a square matrix: d1 = 0, d0 = 1); v_row is the mean over d0 and has shape[d1] entries, v_col the mean over d1 with shape[d0]."""
    shape = tuple(int(s) for s in shape)
    if len(shape) > 2:
        raise ValueError(f"Adafactor on the device takes 1-D and 2-D parameters, got shape {shape}")
    if len(shape) == 2 and min(shape) >= ADAFACTOR_MIN_DIM_TO_FACTOR:
        d1 = 0 if shape[0] <= shape[1] else 1
        return {"v_row": (shape[d1],), "v_col": (shape[1 - d1],)}
    return {"v": shape}


class HypernetAdafactor(HypernetOptimizer):
    """optax.chain(clip_by_global_norm(max_grad_norm), multi_transform({train: adafactor(lr, weight_decay_rate=weight_decay,
    weight_decay_mask), freeze: set_to_zero})) (train.py:631-636, 651-656) for the parameters of `model`, every other argument of
    optax.adafactor at its default (min_dim_size_to_factor 128, decay_rate 0.8, multiply_by_parameter_scale, clipping_threshold 1.0,
    no momentum, eps 1e-30), as one call of the library (zett_op_adafactor_step, csrc/train_adafactor.hip).  Per step, t updates applied so far:

    - norm and ``coef`` as HypernetOptimizer; ``g' = coef g``, ``q = g'^2 + 1e-30``, ``beta = 1 - (t + 1)^-0.8``;
    - a 2-D parameter whose smaller dimension is >= 128 keeps two vectors (adafactor_state_shapes): ``v_row = beta v_row + (1 - beta)
      mean(q, d0)``, ``v_col`` likewise over d1, ``u = g' (v_row / mean(v_row))^-1/2 v_col^-1/2``; every other parameter keeps a full
      ``v = beta v + (1 - beta) q`` and ``u = g' v^-1/2``;
    - ``u_hat = u / max(1, RMS(u))``, ``s = max(RMS(p), 1e-3)``, ``p -= lr s u_hat + (weight_decay p if "decay" else 0)``.

    The weight decay is NOT multiplied by lr: optax.adafactor chains add_decayed_weights after the learning-rate scaling (with
    optax.adamw it is the other way round, and HypernetAdamW's decay is lr wd p).  Everything else is HypernetOptimizer's and the
    interface is HypernetAdamW's, so the two can be swapped (make_optimizer).  Parameters of more than two dimensions are refused with
    ValueError before anything is launched."""

    STATE_KEYS = ("v_row", "v_col", "v")
    MAX_DIM = 2

    def __init__(self, model, lr: float, weight_decay: float = 0.01, max_grad_norm: Optional[float] = 0.1, labels: LabelOverrides = None):
        super().__init__(model, labels, lr=lr, weight_decay=weight_decay, max_grad_norm=max_grad_norm)
        self._workspace: Optional[torch.Tensor] = None

    def _state_shapes(self, p):
        return adafactor_state_shapes(p.shape)

    def _lists(self, device, n, P, G, S, numel, flags, todo, record):
        rows, cols = (C.c_int64 * n)(), (C.c_int64 * n)()
        for i, (_, p) in enumerate(todo):
            rows[i], cols[i] = p.shape if p.dim() == 2 else (1, numel[i])
        need = C.c_int64(0)
        _lib.check(_lib.load().zett_op_adafactor_workspace_floats(rows, cols, flags, n, C.byref(need)), "adafactor workspace")
        if self._workspace is None or self._workspace.numel() < need.value or self._workspace.device != device:
            self._workspace = torch.empty(need.value, dtype=torch.float32, device=device)
        return device, n, P, G, S["v_row"], S["v_col"], S["v"], rows, cols, flags, record

    def _launch(self, lists, lr, zero_grad) -> None:
        device, n, P, G, VR, VC, V, rows, cols, flags, record = lists
        with torch.cuda.device(device):
            _lib.check(_lib.load().zett_op_adafactor_step(P, G, VR, VC, V, rows, cols, flags, n, self.lr if lr is None else float(lr), self.weight_decay,
                                                          math.inf if self.max_grad_norm is None else self.max_grad_norm, int(bool(zero_grad)), ptr(self._workspace), self._workspace.numel(), ptr(record),
                                                          stream(device)), "adafactor")


def make_optimizer(model, training_args, labels: LabelOverrides = None):
    """The optimizer the reference builds from its TrainingArguments (train.py:631-656): HypernetAdafactor when ``use_adafactor`` is
    set, HypernetAdamW(adam_beta1, adam_beta2, adam_epsilon) otherwise, with ``learning_rate`` (a float, or the first entry of a list),
    ``weight_decay`` and ``max_grad_norm`` (None: no clip).  training_args: an object with these attributes or a mapping; a field it
    lacks takes the reference's default (train.py:91-101).  The learning-rate schedule stays the caller's: ``step(lr=...)``."""
    defaults = {"use_adafactor": False, "learning_rate": 3e-4, "max_grad_norm": None, "weight_decay": 0.0, "adam_beta1": 0.9, "adam_beta2": 0.999, "adam_epsilon": 1e-8}

    def field(name):
        if isinstance(training_args, Mapping):
            return training_args.get(name, defaults[name])
        return getattr(training_args, name, defaults[name])

    lr = field("learning_rate")
    if isinstance(lr, (list, tuple)):
        if not lr:
            raise ValueError("learning_rate is an empty list")
        lr = lr[0]
    if field("use_adafactor"):
        return HypernetAdafactor(model, float(lr), weight_decay=float(field("weight_decay")), max_grad_norm=field("max_grad_norm"), labels=labels)
    return HypernetAdamW(model, float(lr), betas=(float(field("adam_beta1")), float(field("adam_beta2"))), eps=float(field("adam_epsilon")),
                         weight_decay=float(field("weight_decay")), max_grad_norm=field("max_grad_norm"), labels=labels)
