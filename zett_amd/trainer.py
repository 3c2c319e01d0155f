"""The reference's training loop (train.py) around the device pieces of zett_amd/training.py and zett_amd/collate.py: the learning-rate
schedule, the identity / train / eval steps, accumulation, logging windows with per-language metrics, evaluation with the embedding
cache, checkpoints and resume with data replay.  One process, one GPU; the backbone is frozen.

No device math lives here and a step adds no wait for the host: per-micro-step scalars are written into a preallocated device window
with ``copy_`` of 0-dim tensors and read back once per logging window; the learning rate and the language index are host numbers to
begin with.  (The hypernetwork's own forward still reads its status word once per step, as before.)

    trainer = HypernetTrainer(hypernet, backbone, source_embeddings, training_args, hn_pad_token_id=hn_tokenizer.pad_token_id, langs=langs)
    loaders = [device_loader(dataset, collator, seed=training_args.seed)]
    trainer.fit(loaders, [1.0], identity_loader=device_loader(None, collator, seed=training_args.seed, for_identity_step=True,
                                                              length=training_args.identity_steps), eval_sets={"main": valid_loader})
"""
import dataclasses
import math
import os
import time
from collections.abc import Mapping
from typing import Callable, Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .collate import _mix64
from .optim import make_optimizer
from .train_config import TrainingArguments
from .training import identity_loss, lexical_loss, lm_head_loss, splice_special_rows, token_embeddings

# the reference's TrainingArguments defaults (train.py:82-121); output_dir has none
TRAINING_DEFAULTS = {f.name: (None if f.default is dataclasses.MISSING else f.default) for f in dataclasses.fields(TrainingArguments)}
REFUSED_FIELDS = ("apply_lexical_loss_to_init", "run_backbone_in_training_mode", "do_cost_analysis", "mix_languages")
STATE_FILE = "trainer_state.pt"
# the columns of the device window; a micro-step writes the ones it has
WINDOW_COLUMNS = ("identity_loss", "loss", "lexical_loss", "mean_lexical_overlap", "grad_norm", "skipped", "avg_byte_length", "unk_ratio", "pad_ratio")
_COLUMN = {name: i for i, name in enumerate(WINDOW_COLUMNS)}
_TRACKED = ("avg_byte_length", "unk_ratio", "pad_ratio")          # prepare_batch's metrics_tracker (train.py:175-191): per language, not per step


def _field(args, name):
    if isinstance(args, Mapping):
        return args.get(name, TRAINING_DEFAULTS[name])
    return getattr(args, name, TRAINING_DEFAULTS[name])


def _args_dict(args) -> dict:
    """training_args as a dict of plain values (what trainer_state.pt stores)"""
    if isinstance(args, Mapping):
        items = dict(args)
    else:
        items = dict(vars(args))
    plain = (bool, int, float, str, type(None))
    return {k: (list(v) if isinstance(v, (list, tuple)) else v) for k, v in items.items()
            if isinstance(v, plain) or (isinstance(v, (list, tuple)) and all(isinstance(x, plain) for x in v))}


# ---- the schedule -------------------------------------------------------------------------------------------------------------------------
def learning_rate_schedule(training_args) -> Callable[[int], float]:
    """The first schedule ``create_learning_rate_fn`` returns (zett/utils.py:83-141: optax ``linear_schedule``s and a
    ``cosine_decay_schedule`` under ``join_schedules``), from ``learning_rate`` (a float, or a list parallel to ``warmup_steps``),
    ``warmup_steps`` (an int or a list), ``random_warmup_steps`` R (default 0), ``random_learning_rate`` (default ``learning_rate``; of a
    list, its first entry), ``steps`` and ``learning_rate_alpha``.  With boundaries ``[R, W_1, ..., W_n]`` and ``W_0 = R``:

        s < R                 random_lr * s / R
        W_{i-1} <= s < W_i    lr_i * (s - W_{i-1}) / (W_i - W_{i-1})                       (every stage restarts from 0)
        s >= W_n              lr_n * ((1 - alpha) * 0.5 * (1 + cos(pi * c / (steps - W_n))) + alpha),  c = min(s - W_n, steps - W_n)

    A stage of zero length has an empty range.  ``steps - W_n <= 0``, boundaries that decrease and lists of different lengths raise
    ValueError.  Computed in Python floats (float64); the reference computes the same expressions in float32."""
    lr, warm = _field(training_args, "learning_rate"), _field(training_args, "warmup_steps")
    warm = [int(warm)] if isinstance(warm, (int, np.integer)) else [int(w) for w in warm]
    lrs = [float(x) for x in lr] if isinstance(lr, (list, tuple)) else [float(lr)] * len(warm)
    if not warm or len(lrs) != len(warm):
        raise ValueError(f"learning_rate {lrs} and warmup_steps {warm} must be lists of one length")
    r = int(_field(training_args, "random_warmup_steps") or 0)
    random_lr = _field(training_args, "random_learning_rate")
    random_lr = lrs[0] if not random_lr else float(random_lr[0] if isinstance(random_lr, (list, tuple)) else random_lr)
    bounds = [r] + warm
    if r < 0 or any(b < a for a, b in zip(bounds, bounds[1:])):
        raise ValueError(f"schedule boundaries {bounds} must not decrease")
    decay_steps = int(_field(training_args, "steps")) - warm[-1]
    if decay_steps <= 0:
        raise ValueError(f"steps = {_field(training_args, 'steps')} leaves no step after the last warm-up boundary {warm[-1]}")
    alpha = float(_field(training_args, "learning_rate_alpha"))

    def schedule(step: int) -> float:
        s = int(step)
        if s < r:
            return random_lr * s / r
        for lo, hi, peak in zip(bounds, bounds[1:], lrs):
            if s < hi:
                return peak * (s - lo) / (hi - lo)
        c = min(s - warm[-1], decay_steps)
        return lrs[-1] * ((1.0 - alpha) * 0.5 * (1.0 + math.cos(math.pi * c / decay_steps)) + alpha)

    return schedule


# ---- draws and loaders ----------------------------------------------------------------------------------------------------------------------
def loader_draw(seed: int, micro_step: int, probs: Sequence[float]) -> int:
    """Which train loader feeds `micro_step`: one ``choice(len(probs), p=probs)`` of a numpy Philox generator keyed by ``(seed,
    micro_step)`` — a pure function of its arguments, so a resumed run replays the draws without carrying generator state.  (The reference
    draws with a JAX key that it splits once per update: a deviation.)"""
    p = np.asarray(probs, dtype=np.float64)
    key = np.array([int(seed) & 0xFFFFFFFFFFFFFFFF, int(micro_step)], dtype=np.uint64)
    return int(np.random.Generator(np.random.Philox(key=key)).choice(len(p), p=p / p.sum()))


def item_seed(seed: int, index: int) -> int:
    """The collator seed of item `index` of a device_loader iteration: ``mix64(mix64(seed) + index)`` (the splitmix64 finaliser of
    zett_amd/collate.py), a pure function of the two."""
    return _mix64(_mix64(int(seed)) + int(index))


class device_loader:
    """A re-iterable over `dataset` through a ``DeviceCollator``: item i of an iteration is ``collator([item], seed=item_seed(seed, i),
    check=check)``; every iteration starts at i = 0 again, so a restarted loader repeats itself, as a ``DataLoader`` over the
    reference's deterministic datasets does.  With ``for_identity_step=True`` it yields `length` identity batches
    (``collator(None, True, seed=item_seed(seed, i))``; the trainer passes ``identity_steps``) and `dataset` is not read.  ``sampling``
    tells ``HypernetTrainer.evaluate`` not to cache the first batch's embeddings: the collator's ``do_tokenizer_sampling``, or an
    ``n_token_subsample``, under which every batch indexes a sub-vocabulary of its own (the reference caches there all the same).  Everything
    runs in the calling thread: no workers, threads or subprocesses."""

    def __init__(self, dataset, collator, *, seed: int, check: bool = False, for_identity_step: bool = False, length: Optional[int] = None):
        if for_identity_step and length is None:
            raise ValueError("an identity loader needs its length (identity_steps)")
        self.dataset, self.collator, self.seed, self.check = dataset, collator, int(seed), bool(check)
        self.for_identity_step, self.length = bool(for_identity_step), length
        a = getattr(collator, "data_args", None)
        self.sampling = bool(getattr(a, "do_tokenizer_sampling", False)) or getattr(a, "n_token_subsample", None) is not None

    def __iter__(self):
        if self.for_identity_step:
            for i in range(int(self.length)):
                yield self.collator(None, True, seed=item_seed(self.seed, i), check=self.check)
            return
        for i, item in enumerate(self.dataset):
            if self.length is not None and i >= self.length:
                return
            yield self.collator([item], seed=item_seed(self.seed, i), check=self.check)


# ---- aggregation (host) ---------------------------------------------------------------------------------------------------------------------
def _tracked(records, lang_indices, langs, names, out):
    for j, lang in enumerate(langs):
        for name in names:
            values = [r[name] for r, l in zip(records, lang_indices) if l == j and name in r]
            if not values:
                continue
            if name == "avg_byte_length":
                out[f"{lang}_avg_byte_length"] = float(np.mean(values))
                out[f"{lang}_std_byte_length"] = float(np.std(values))
            else:
                out[f"{lang}_{name}"] = float(np.mean(values))


def aggregate_window(records: Sequence[Mapping[str, float]], lang_indices: Sequence[int], langs: Sequence[str], elapsed: float) -> Dict[str, float]:
    """A logging window as train.py:1481-1530.  records: one dict of numbers per micro-step, holding the metrics that step carries;
    lang_indices: its language index.  Every metric but the tracked three: its mean over the steps that carry it; ``loss`` also per
    language (``{lang}_loss``), NaN for a language with no step in the window; ``time`` = elapsed; per language, from the steps that carry
    them, ``{lang}_avg_byte_length`` (mean) with ``{lang}_std_byte_length`` (population std, numpy's), ``{lang}_unk_ratio`` and
    ``{lang}_pad_ratio`` (means).  All keys prefixed ``train/``.  Means are taken in float64 (the reference's are float32)."""
    out: Dict[str, float] = {}
    names = []
    for r in records:
        names.extend(k for k in r if k not in names and k not in _TRACKED)
    for name in names:
        if name == "loss":
            for j, lang in enumerate(langs):
                values = [r[name] for r, l in zip(records, lang_indices) if l == j and name in r]
                out[f"{lang}_loss"] = float(np.mean(values)) if values else float("nan")
        out[name] = float(np.mean([r[name] for r in records if name in r]))
    out["time"] = float(elapsed)
    _tracked(records, lang_indices, langs, _TRACKED, out)
    return {"train/" + k: v for k, v in out.items()}


def aggregate_eval(records: Sequence[Mapping[str, float]], lang_indices: Sequence[int], langs: Sequence[str], set_name: str) -> Dict[str, float]:
    """One evaluation set as train.py:1362-1393: every metric averaged per language over that language's batches
    (``eval/{set}_{lang}_{metric}``; a language without batches has no key), ``{lang}_avg_byte_length`` / ``{lang}_std_byte_length`` and
    ``{lang}_unk_ratio`` from the batches' own metrics."""
    out: Dict[str, float] = {}
    names = []
    for r in records:
        names.extend(k for k in r if k not in names and k not in _TRACKED)
    for name in names:
        for j, lang in enumerate(langs):
            values = [r[name] for r, l in zip(records, lang_indices) if l == j and name in r]
            if values:
                out[f"{lang}_{name}"] = float(np.mean(values))
    _tracked(records, lang_indices, langs, ("avg_byte_length", "unk_ratio"), out)
    return {f"eval/{set_name}_{k}": v for k, v in out.items()}


class _Window:
    """Per-micro-step scalars on the device: a ``[rows, len(WINDOW_COLUMNS)]`` float64 tensor written with ``copy_`` of 0-dim tensors, and
    on the host which columns each row carries, its language index and its learning rate.  ``read()`` is the one transfer."""

    def __init__(self, rows: int, device):
        self.values = torch.zeros((max(int(rows), 1), len(WINDOW_COLUMNS)), dtype=torch.float64, device=device)
        self.written: List[Tuple[str, ...]] = []
        self.langs: List[int] = []
        self.rates: List[float] = []

    def add(self, metrics: Mapping[str, object], lang_index: int) -> None:
        row = len(self.written)
        if row == self.values.shape[0]:
            raise RuntimeError("the metric window is full")
        names = []
        for name, value in metrics.items():
            if name == "learning_rate":
                continue
            self.values[row, _COLUMN[name]].copy_(value)
            names.append(name)
        self.written.append(tuple(names))
        self.langs.append(int(lang_index))
        self.rates.append(float(metrics["learning_rate"]))

    def read(self):
        host = self.values[:max(len(self.written), 1)].cpu().numpy()
        records = [dict({name: float(host[i, _COLUMN[name]]) for name in names}, learning_rate=self.rates[i]) for i, names in enumerate(self.written)]
        langs = list(self.langs)
        self.written, self.langs, self.rates = [], [], []
        return records, langs


# ---- the trainer ----------------------------------------------------------------------------------------------------------------------------
class HypernetTrainer:
    """train.py's loop for a ZettHypernet in front of a frozen backbone.

    backbone: ``backbone(inputs_embeds, attention_mask) -> hidden [B, S, E]``, any torch callable; a ``torch.nn.Module`` is put in
    ``eval()`` with ``requires_grad_(False)`` and is never stepped.  head (optional): ``head(hidden) -> hidden``, the transform between the
    encoder and the output embeddings (RoBERTa's ``lm_head.dense -> gelu -> layer_norm``).  source_embeddings: ``[V, E]`` or ``[V, 2E]``
    on the hypernetwork's device, the matrix of train.py:330-346.  training_args: an object or a mapping with the reference's fields; a
    missing field takes the reference's default.  optimizer: default ``make_optimizer(hypernet, training_args)``.  lm_precision: the
    ``precision`` of ``lm_head_loss``; embed_dtype: the ``dtype`` of ``token_embeddings`` (the backbone's).  langs: the language codes
    that ``lang_index`` indexes (logging and evaluation); hn_tokenizer: saved beside the hypernetwork by ``fit``.

    The token lookup runs with ``check_ids=False`` (no wait for the host): an id outside the batch's vocabulary gives a zero row; the
    ``DeviceCollator`` produces none.

    Refused with NotImplementedError naming the field: ``backbone_training != "no"``, ``apply_lexical_loss_to_init``,
    ``run_backbone_in_training_mode``, ``do_cost_analysis``, ``mix_languages``.  ValueError: ``gradient_accumulation_steps < 1``,
    ``logging_steps < 1``, a ``loss`` other than "clm" / "mlm"."""

    def __init__(self, hypernet, backbone, source_embeddings, training_args, *, hn_pad_token_id, head=None, optimizer=None, lm_precision="bf16", embed_dtype=None,
                 langs: Optional[Sequence[str]] = None, hn_tokenizer=None):
        a = training_args
        if _field(a, "backbone_training") != "no":
            raise NotImplementedError(f"backbone_training={_field(a, 'backbone_training')!r}: the backbone is frozen here")
        for name in REFUSED_FIELDS:
            if _field(a, name):
                raise NotImplementedError(name)
        self.k = int(_field(a, "gradient_accumulation_steps"))
        if self.k < 1:
            raise ValueError("gradient_accumulation_steps must be at least 1")
        if int(_field(a, "logging_steps")) < 1:
            raise ValueError("logging_steps must be at least 1")
        self.loss = _field(a, "loss")
        if self.loss not in ("clm", "mlm"):
            raise ValueError(f"loss must be \"clm\" or \"mlm\", got {self.loss!r}")
        self.args = a
        self.hypernet, self.backbone, self.head, self.source_embeddings = hypernet, backbone, head, source_embeddings
        for module in (backbone, head):
            if isinstance(module, torch.nn.Module):
                module.eval().requires_grad_(False)
        self.hn_pad_token_id = hn_pad_token_id
        self.lm_precision, self.embed_dtype = lm_precision, embed_dtype
        self.optimizer = make_optimizer(hypernet, a) if optimizer is None else optimizer
        self.schedule = learning_rate_schedule(a)
        self.langs = None if langs is None else list(langs)
        self.hn_tokenizer = hn_tokenizer
        self.micro_step = 0
        self.use_lexical = bool(getattr(getattr(hypernet, "config", None), "hn_embed_using_source_embeddings", True))

    # ---- steps ----
    def _predict(self, batch):
        return self.hypernet(batch["target_surface_forms"], source_embeddings=self.source_embeddings, lang_index=batch["lang_index"])

    def _backward_and_update(self, loss, metrics) -> None:
        """(loss / k).backward(); on every k-th micro-step the update, whose norm and skip flag are cloned out of the optimizer's device
        record (last_step_stats() would wait for the host)"""
        update = self.micro_step // self.k
        lr = self.schedule(update)
        metrics["learning_rate"] = lr
        (loss / self.k).backward()
        if (self.micro_step + 1) % self.k == 0:
            self.optimizer.step(lr=lr, zero_grad=True)
            record = self.optimizer.record
            if record is not None:
                metrics["grad_norm"] = record[0].clone()
                metrics["skipped"] = record.view(torch.int32)[2].clone()
        self.micro_step += 1

    def identity_micro_step(self, batch) -> Dict[str, object]:
        """identity_train_step (train.py:914-975).  Metrics: identity_loss (0-dim device tensor), learning_rate (float); after an update
        also grad_norm and skipped."""
        self.hypernet.train()
        pred_in, pred_out, _ = self._predict(batch)
        loss = identity_loss(pred_in, pred_out, self.source_embeddings, batch["ids_to_embed"])
        metrics = {"identity_loss": loss.detach()}
        self._backward_and_update(loss, metrics)
        return metrics

    def _lm(self, batch, pred_in, pred_out, bias):
        x = token_embeddings(pred_in, batch["input_ids"], dtype=self.embed_dtype, check_ids=False)
        hidden = self.backbone(x, batch["attention_mask"])
        if self.head is not None:
            hidden = self.head(hidden)
        return lm_head_loss(hidden, pred_out if pred_out is not None else pred_in, batch["labels"], batch["attention_mask"], mode=self.loss,
                            bias=bias if _field(self.args, "learnable_bias") else None,
                            priors=batch["target_priors"] if _field(self.args, "add_target_priors_to_bias") else None, vocab_mask=batch["mask"],
                            precision=self.lm_precision)

    def train_micro_step(self, batch) -> Dict[str, object]:
        """train_step (train.py:977-1162).  Metrics: loss, lexical_loss, mean_lexical_overlap (0-dim device tensors), learning_rate
        (float); after an update also grad_norm and skipped."""
        self.hypernet.train()
        pred_in, pred_out, bias = self._predict(batch)
        pred_in, pred_out = splice_special_rows(pred_in, pred_out, self.source_embeddings, batch["special_indices"], batch["special_indices_in_reference"], inplace=True)
        lm, _ = self._lm(batch, pred_in, pred_out, bias)
        if self.use_lexical:
            lex, overlap = lexical_loss(pred_in, pred_out, self.source_embeddings, batch["target_surface_forms"], self.hn_pad_token_id,
                                        kind=_field(self.args, "lexical_loss_kind"))
            loss = lm + float(_field(self.args, "lexical_loss_weight")) * lex
        else:
            lex = overlap = torch.zeros((), dtype=torch.float32, device=lm.device)
            loss = lm
        metrics = {"loss": loss.detach(), "lexical_loss": lex.detach(), "mean_lexical_overlap": overlap.detach()}
        self._backward_and_update(loss, metrics)
        return metrics

    def eval_step(self, batch, cache=None):
        """eval_step (train.py:1164-1263) under ``torch.no_grad()`` with the hypernetwork in ``eval()`` (the inference path).  cache: the
        ``(pred_in, pred_out, bias)`` an earlier call returned for the same vocabulary; None predicts and splices the batch's.  Returns
        ``({"loss", "bpb"} for clm | {"loss", "acc"} for mlm, cache)``, 0-dim device tensors.  The hypernetwork's mode is restored."""
        was_training = self.hypernet.training
        self.hypernet.eval()
        try:
            with torch.no_grad():
                if cache is None:
                    pred_in, pred_out, bias = self._predict(batch)
                    pred_in, pred_out = splice_special_rows(pred_in, pred_out, self.source_embeddings, batch["special_indices"], batch["special_indices_in_reference"],
                                                            inplace=True)
                    cache = (pred_in, pred_out, bias)
                loss, stats = self._lm(batch, *cache)
                metrics = {"loss": loss}
                if self.loss == "clm":
                    b, s = batch["labels"].shape
                    metrics["bpb"] = (stats["row_loss"].view(b, s).sum(-1) / batch["byte_lengths"].sum(-1)).mean()
                else:
                    metrics["acc"] = stats["n_correct"] / stats["n_counted"]
        finally:
            self.hypernet.train(was_training)
        return metrics, cache

    # ---- loops ----
    def _langs(self, langs):
        langs = self.langs if langs is None else list(langs)
        if langs is None:
            raise ValueError("the language codes are needed: pass langs= here or to the constructor")
        return langs

    @staticmethod
    def _batch_columns(batch, with_pad_ratio: bool):
        out = dict(batch.get("metrics") or {})
        if with_pad_ratio and out and "attention_mask" in batch:
            out["pad_ratio"] = (batch["attention_mask"] == 0).to(torch.float64).mean()
        return out

    def evaluate(self, eval_sets: Mapping[str, Iterable], langs: Optional[Sequence[str]] = None) -> Dict[str, float]:
        """eval_loop (train.py:1307-1395).  eval_sets: ``{name: batches}`` or ``{name: (batches, sampling)}``.  The embeddings of a set's
        first batch are cached for its remaining batches unless the set is flagged as sampling — the ``sampling`` of the pair, or the
        ``sampling`` attribute of `batches` (a device_loader sets it), False when neither is there.  As in the reference the cache is the
        first batch's whatever its language: with ``hn_embed_lang_id`` a later language of the set is scored on the first one's
        embeddings.  The set's scalars are read back once, after its last batch."""
        langs = self._langs(langs)
        out: Dict[str, float] = {}
        for name, batches in eval_sets.items():
            if isinstance(batches, tuple):
                batches, sampling = batches
            else:
                sampling = bool(getattr(batches, "sampling", False))
            rows, lang_indices, cache = [], [], None
            for batch in batches:
                metrics, new_cache = self.eval_step(batch, cache)
                if not sampling:
                    cache = new_cache
                metrics.update(self._batch_columns(batch, False))
                rows.append(metrics)
                lang_indices.append(int(batch["lang_index"]))          # (a host tensor)
            if not rows:
                continue
            names = sorted({k for r in rows for k in r})
            device = self.source_embeddings.device
            flat = torch.stack([r[k].to(device=device, dtype=torch.float64) if k in r else torch.zeros((), dtype=torch.float64, device=device) for r in rows for k in names])
            host = flat.cpu().numpy().reshape(len(rows), len(names))
            records = [{k: float(host[i, j]) for j, k in enumerate(names) if k in r} for i, r in enumerate(rows)]
            out.update(aggregate_eval(records, lang_indices, langs, name))
        return out

    def fit(self, train_loaders: Sequence[Iterable], train_probs: Sequence[float], *, identity_loader: Optional[Iterable] = None,
            eval_sets: Optional[Mapping[str, Iterable]] = None, log: Callable = print, langs: Optional[Sequence[str]] = None,
            stop_after: Optional[int] = None) -> None:
        """The loop of train.py:1397-1561 up to ``steps`` updates.  An update below ``identity_steps`` takes its micro-steps from
        `identity_loader` and ``identity_micro_step``; after that each micro-step draws one of `train_loaders` (``loader_draw(seed,
        micro_step, train_probs)``).  An exhausted loader is restarted with ``iter()``.  Micro-steps below ``self.micro_step`` (set by
        ``resume``) are replayed: the draw and ``next()`` happen, the step is skipped, so collators, sampler queues and seeds stand where
        an uninterrupted run had them.  Every ``logging_steps`` updates ``log(aggregate_window(...), step)``; ``save_steps``,
        ``eval_steps``, ``eval_at_step_zero`` as the reference (``log(evaluate(...), step)``; without an ``output_dir`` nothing is saved).  stop_after: return after that many updates of
        the schedule's ``steps`` (an interrupted run; the schedule still spans ``steps``)."""
        a = self.args
        langs = self._langs(langs)
        steps, identity_steps, logging_steps = int(_field(a, "steps")), int(_field(a, "identity_steps")), int(_field(a, "logging_steps"))
        save_steps, eval_steps, seed = int(_field(a, "save_steps")), int(_field(a, "eval_steps")), int(_field(a, "seed"))
        if identity_steps > 0 and identity_loader is None:
            raise ValueError("identity_steps > 0 needs an identity_loader")
        if len(train_loaders) != len(train_probs) or not train_loaders:
            raise ValueError("one probability per train loader")
        start = time.time()
        iters = [iter(loader) for loader in train_loaders]
        identity_iter = iter(identity_loader) if identity_steps > 0 else None
        window = _Window(logging_steps * self.k, self.source_embeddings.device)
        resumed_at = self.micro_step
        if _field(a, "eval_at_step_zero") and eval_sets:
            log(self.evaluate(eval_sets, langs), 0)
        for step in range(steps if stop_after is None else min(steps, int(stop_after))):
            for j in range(self.k):
                m = step * self.k + j
                index = loader_draw(seed, m, train_probs)
                identity = step < identity_steps
                try:
                    batch = next(identity_iter if identity else iters[index])
                except StopIteration:
                    if identity:
                        identity_iter = iter(identity_loader)
                        batch = next(identity_iter)
                    else:
                        iters[index] = iter(train_loaders[index])
                        batch = next(iters[index])
                if m < resumed_at:
                    continue
                metrics = self.identity_micro_step(batch) if identity else self.train_micro_step(batch)
                metrics.update(self._batch_columns(batch, True))
                window.add(metrics, int(batch["lang_index"]))
            if (step + 1) * self.k <= resumed_at:
                continue
            if (step + 1) % logging_steps == 0:
                records, lang_indices = window.read()
                log(aggregate_window(records, lang_indices, langs, time.time() - start), step + 1)
            if (step + 1) % save_steps == 0 and _field(a, "output_dir"):
                self.save(_field(a, "output_dir"))
                if self.hn_tokenizer is not None:
                    self.hn_tokenizer.save_pretrained(_field(a, "output_dir"))
            if (step + 1) % eval_steps == 0 and eval_sets:
                log(self.evaluate(eval_sets, langs), step + 1)

    # ---- checkpoints ----
    def save(self, output_dir: str) -> None:
        """``hypernet.save_pretrained(output_dir)`` and, with ``save_state``, ``trainer_state.pt``: the optimizer's state_dict, the
        micro-step count and training_args as a dict."""
        os.makedirs(output_dir, exist_ok=True)
        self.hypernet.save_pretrained(output_dir)
        if _field(self.args, "save_state"):
            sd = self.optimizer.state_dict()
            sd["state"] = {n: {k: t.cpu() for k, t in st.items()} for n, st in sd["state"].items()}
            sd["hyper"] = {k: (list(v) if isinstance(v, tuple) else v) for k, v in sd["hyper"].items()}
            torch.save({"optimizer": sd, "micro_step": int(self.micro_step), "training_args": _args_dict(self.args)}, os.path.join(output_dir, STATE_FILE))

    def resume(self, checkpoint_dir: str) -> None:
        """Loads what ``save`` wrote: the hypernetwork's parameters (``from_pretrained``'s layout) into this hypernetwork, the optimizer's
        state and the micro-step count, which ``fit`` then replays.  With ``resume_from_checkpoint_reset_steps`` parameters and moments
        are kept and the count — and with it the schedule — restarts at 0.  (optax's own count would go on there while the reported
        rate restarts; the reported one is followed.)"""
        self.hypernet.load_state_dict(type(self.hypernet).from_pretrained(checkpoint_dir).state_dict())
        state = torch.load(os.path.join(checkpoint_dir, STATE_FILE), weights_only=True)
        self.optimizer.load_state_dict(state["optimizer"])
        self.micro_step = 0 if _field(self.args, "resume_from_checkpoint_reset_steps") else int(state["micro_step"])
