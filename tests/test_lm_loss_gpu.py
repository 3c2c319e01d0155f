"""zett_amd.training.lm_head_loss on the GPU: the language-model loss over predicted output embeddings (csrc/train_loss.hip between the
library's GEMMs).  The yardstick is float64 torch on the CPU on the as-written formula

    logits = hidden @ W.T + where(vocab_mask, 0, -100000) + bias + priors
    loss = sum(w * (logsumexp(logits) - logits[label])) / sum(w)          (a label outside [0, V): an all-zero one-hot, w * logsumexp)

and torch autograd on it — never the kernels themselves.  Forward quantities are held against float64 on the SAME operands (rounded to the
operand type in the 16-bit modes: only fp32 accumulation separates the two) to 1e-5 relative; gradients against float64 on the UNROUNDED
operands to the limits of tests/test_autograd_gpu.py."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from zett_amd import synth
from zett_amd.training import lm_head_loss

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SHAPES = ((150, 203, 64), (333, 1000, 128), (70, 4100, 192))          # (T, V, E): V = 203 pads the columns, V = 4100 spans tile columns
CHUNK = 64                                                             # several chunks and a ragged last one
FWD_LIMIT = 1e-5                                                       # the loss limit of tests/test_training_gpu.py
GRAD_LIMIT = {"f32": 2e-4, "f16": 1e-2, "bf16": 6e-2}                  # tests/test_autograd_gpu.py
LO = {"f32": None, "bf16": torch.bfloat16, "f16": torch.float16}
MASK_FILL = -100000.0
GAP = 1e-4


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


@functools.lru_cache(maxsize=None)
def _inputs(t, v, e, addend, weights, scale=1.0):
    g = torch.Generator().manual_seed(1234)
    hidden = torch.randn(t, e, generator=g) * scale
    w_out = 2.0 * torch.randn(v, e, generator=g) / e ** 0.5
    labels = torch.randint(0, v, (t,), generator=g)
    bias = priors = vmask = weight = None
    if addend:
        bias = 0.3 * torch.randn(v, generator=g)
        priors = -3.0 * torch.rand(v, generator=g)
        vmask = torch.rand(v, generator=g) >= 0.2                      # about 20 % of the columns are masked
        labels = torch.where(vmask[labels], labels, (labels + 1) % v)  # labels avoid masked columns ...
        labels = torch.where(vmask[labels], labels, (labels + 1) % v)
        labels = torch.where(vmask[labels], labels, torch.nonzero(vmask)[0, 0].expand_as(labels))
        labels[3] = int(torch.nonzero(~vmask)[0, 0])                   # ... except one row, whose label IS a masked column
    if weights == "binary":
        weight = (torch.rand(t, generator=g) >= 0.3).float()           # about 30 % zeros, whose labels are -100
        labels = torch.where(weight > 0, labels, torch.full_like(labels, -100))
        weight[3] = 1.0
        if addend:
            labels[3] = int(torch.nonzero(~vmask)[0, 0])
    elif weights == "real":
        weight = 2.0 * torch.rand(t, generator=g)
    return hidden, w_out, labels, bias, priors, vmask, weight


def _formula64(hidden, w_out, labels, bias, priors, vmask, weight):
    """The as-written formula in float64; hidden / w_out / bias may require grad.  -> loss, row_loss, lse, logits"""
    v = w_out.shape[0]
    logits = hidden @ w_out.T
    if vmask is not None:
        logits = logits + torch.where(vmask, 0.0, MASK_FILL).double()
    if bias is not None:
        logits = logits + bias
    if priors is not None:
        logits = logits + priors.double()
    lse = torch.logsumexp(logits, -1)
    hit = (labels >= 0) & (labels < v)
    picked = torch.where(hit, logits.gather(1, labels.clamp(0, v - 1)[:, None])[:, 0], torch.zeros_like(lse))
    w = torch.ones_like(lse) if weight is None else weight.double()
    row = w * (lse - picked)
    return row.sum() / w.sum(), row, lse, logits


@functools.lru_cache(maxsize=None)
def _reference(t, v, e, addend, weights, scale=1.0):
    """float64 on the unrounded operands, with autograd: computed once per case and shared"""
    hidden, w_out, labels, bias, priors, vmask, weight = _inputs(t, v, e, addend, weights, scale)
    h64, w64 = hidden.double().requires_grad_(True), w_out.double().requires_grad_(True)
    b64 = None if bias is None else bias.double().requires_grad_(True)
    loss, _, _, _ = _formula64(h64, w64, labels, b64, priors, vmask, weight)
    loss.backward()
    return {"d_hidden": h64.grad, "d_w": w64.grad, "d_bias": None if b64 is None else b64.grad}


@functools.lru_cache(maxsize=None)
def _forward_reference(t, v, e, addend, weights, precision, scale=1.0, hidden_dtype=torch.float32):
    """float64 on the operands the kernels see: rounded to the operand type in the 16-bit modes"""
    hidden, w_out, labels, bias, priors, vmask, weight = _inputs(t, v, e, addend, weights, scale)
    hidden = hidden.to(hidden_dtype).float()
    if LO[precision] is not None:
        hidden, w_out = hidden.to(LO[precision]), w_out.to(LO[precision])
    with torch.no_grad():
        loss, row, lse, logits = _formula64(hidden.double(), w_out.double(), labels, None if bias is None else bias.double(), priors, vmask, weight)
    top = logits.topk(2, dim=-1)
    return {"loss": loss, "row_loss": row, "lse": lse, "argmax": top.indices[:, 0], "gap": top.values[:, 0] - top.values[:, 1]}


def _dev(x):
    return None if x is None else x.to(DEV)


def _run(t, v, e, addend, weights, precision, scale=1.0, grad=True, hidden_dtype=torch.float32, **kw):
    hidden, w_out, labels, bias, priors, vmask, weight = _inputs(t, v, e, addend, weights, scale)
    h = hidden.to(hidden_dtype).to(DEV).requires_grad_(grad)
    w = w_out.to(DEV).requires_grad_(grad)
    b = None if bias is None else bias.to(DEV).requires_grad_(grad)
    kw.setdefault("chunk_rows", CHUNK)
    loss, stats = lm_head_loss(h, w, _dev(labels), weight=_dev(weight), bias=b, priors=_dev(priors), vocab_mask=_dev(vmask), precision=precision, **kw)
    out = {"loss": loss.detach(), **stats}
    if grad:
        loss.backward()
        out.update(d_hidden=h.grad, d_w=w.grad, d_bias=None if b is None else b.grad)
    return out


def _check_forward(got, ref, what, apart=None):
    """apart: a row whose loss is ~1e5 (its label is a masked column) — the l2 error over the OTHER rows is held to the limit as well"""
    assert abs(float(got["loss"]) - float(ref["loss"])) <= FWD_LIMIT * abs(float(ref["loss"])), (what, float(got["loss"]), float(ref["loss"]))
    for key in ("row_loss", "lse"):
        err = _rel(got[key], ref[key])
        print(what, key, err)
        assert err <= FWD_LIMIT, (what, key, err)
    if apart is not None:
        rest = torch.arange(len(ref["row_loss"])) != apart
        err = _rel(got["row_loss"].cpu()[rest], ref["row_loss"][rest])
        print(what, "row_loss without row", apart, err)
        assert err <= FWD_LIMIT, (what, err)
    clear = ref["gap"] >= GAP
    assert float((~clear).double().mean()) <= 0.02, what
    assert torch.equal(got["argmax"].cpu().long()[clear], ref["argmax"][clear]), what


def _check_grads(got, ref, limit, what):
    for key in ("d_hidden", "d_w", "d_bias"):
        if ref[key] is None:
            continue
        assert bool(torch.isfinite(got[key]).all()), (what, key)
        err = _rel(got[key], ref[key])
        print(what, key, err)
        assert err <= limit, (what, key, err)


# ---- 1. values and gradients ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [None, "binary", "real"])
@pytest.mark.parametrize("addend", [False, True], ids=["plain", "addend"])
@pytest.mark.parametrize("precision", ["f32", "bf16", "f16"])
def test_values_and_gradients_match_float64(precision, addend, weights):
    for t, v, e in SHAPES:
        what = (precision, addend, weights, t, v, e)
        got = _run(t, v, e, addend, weights, precision)
        _check_forward(got, _forward_reference(t, v, e, addend, weights, precision), what, apart=3 if addend else None)
        _check_grads(got, _reference(t, v, e, addend, weights), GRAD_LIMIT[precision], what)
        _, _, labels, _, _, vmask, weight = _inputs(t, v, e, addend, weights)
        w = torch.ones(t) if weight is None else weight
        assert int(got["n_counted"]) == int((w > 0).sum()) and float(got["weight_sum"]) == pytest.approx(float(w.double().sum()), rel=1e-6)
        assert int(got["n_correct"]) == int(((got["argmax"].cpu().long() == labels) & (w > 0)).sum())
        if addend:
            # a masked column no label points at receives exactly no gradient; the one row whose label is masked follows the formula
            untouched = ~vmask
            untouched[labels[(labels >= 0) & (w > 0)]] = False
            assert int(untouched.sum()) > 0 and not got["d_w"].cpu()[untouched].any(), what
            assert bool(torch.isfinite(got["row_loss"]).all()) and float(got["row_loss"][3]) > 0.9 * -MASK_FILL * float(w[3]) > 0, what


@pytest.mark.parametrize("mode", ["clm", "mlm"])
def test_clm_and_mlm_follow_the_reference_slicing(mode):
    """loss_fn of train.py:874-912 written as it stands (shifted views of the logits), on a [B, S] layout."""
    t, v, e = SHAPES[0]
    b, s = 5, 30
    hidden, w_out, labels, *_ = _inputs(t, v, e, False, None)
    g = torch.Generator().manual_seed(1234)
    attention = (torch.arange(s)[None, :] < torch.randint(s // 2, s + 1, (b, 1), generator=g)).long()
    labels = labels.view(b, s).clone()
    if mode == "mlm":
        labels[torch.rand(b, s, generator=g) < 0.6] = -100
    h64, w64 = hidden.double().requires_grad_(True), w_out.double().requires_grad_(True)
    logits = (h64 @ w64.T).view(b, s, v)
    if mode == "clm":
        ce = F.cross_entropy(logits[..., :-1, :].reshape(-1, v), labels[..., 1:].reshape(-1), reduction="none").view(b, s - 1)
        want = (ce * attention[..., :-1]).sum() / attention[..., :-1].sum()
    else:
        label_mask = ((labels != -100) & (attention == 1)).double()
        ce = F.cross_entropy(logits.view(-1, v), labels.clamp(min=0).view(-1), reduction="none").view(b, s)          # (rows of -100 have weight 0)
        want = (ce * label_mask).sum() / label_mask.sum()
    want.backward()
    h = hidden.view(b, s, e).to(DEV).requires_grad_(True)
    w = w_out.to(DEV).requires_grad_(True)
    loss, stats = lm_head_loss(h, w, labels.to(DEV), attention.to(DEV), mode=mode, precision="f32", chunk_rows=CHUNK)
    loss.backward()
    assert abs(float(loss.detach()) - float(want.detach())) <= FWD_LIMIT * abs(float(want.detach())), (float(loss.detach()), float(want.detach()))
    assert h.grad.shape == (b, s, e) and _rel(h.grad.view(t, e), h64.grad) <= GRAD_LIMIT["f32"] and _rel(w.grad, w64.grad) <= GRAD_LIMIT["f32"]
    if mode == "clm":
        assert not stats["row_loss"].view(b, s)[:, -1].any() and not h.grad[:, -1].any()          # the last position scores nothing


# ---- 2. invariance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16", "f16"])
def test_results_do_not_depend_on_the_chunk_size_or_the_run(precision):
    for t, v, e in SHAPES:
        what = (precision, t, v, e)
        a = _run(t, v, e, True, "real", precision, chunk_rows=CHUNK)
        again = _run(t, v, e, True, "real", precision, chunk_rows=CHUNK)
        one = _run(t, v, e, True, "real", precision, chunk_rows=t)
        for key in ("loss", "row_loss", "lse", "argmax", "n_correct", "n_counted", "weight_sum", "d_hidden", "d_w", "d_bias"):
            assert torch.equal(a[key], again[key]), (what, key)          # the same call twice: every bit
        for key in ("loss", "row_loss", "lse", "argmax", "d_hidden"):
            assert torch.equal(a[key], one[key]), (what, key)            # rows are independent of the chunking
        for key in ("d_w", "d_bias"):                                    # sums over T: only their order follows the chunking
            print(what, key, "chunks of", CHUNK, "against one chunk", _rel(a[key], one[key]))
            assert _rel(a[key], one[key]) <= GRAD_LIMIT["f32"], (what, key, _rel(a[key], one[key]))


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_both_paths_of_the_rows_pass_give_the_same_bits(precision):
    for t, v, e in SHAPES:
        once = _run(t, v, e, True, "binary", precision, rows_path="once")
        twice = _run(t, v, e, True, "binary", precision, rows_path="twice")
        for key in ("loss", "row_loss", "lse", "argmax", "d_hidden", "d_w", "d_bias"):
            assert torch.equal(once[key], twice[key]), (precision, t, v, e, key)
    with torch.no_grad():
        a = _run(*SHAPES[2], False, None, precision, grad=False, rows_path="once")
        b = _run(*SHAPES[2], False, None, precision, grad=False, rows_path="twice")
    assert torch.equal(a["row_loss"], b["row_loss"]) and torch.equal(a["argmax"], b["argmax"])


@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("v", [12000, 32768, 32772, 262144])
def test_vocabulary_sizes_around_the_read_once_limit(v, precision):
    """The row lengths at which the rows pass changes its code: four and eight vectors per lane (12 000, 32 768 columns: the longest row
    that is read once), the first length that is read twice (32 772), and the largest vocabulary the library is used with (262 144);
    few rows, two chunks."""
    t, e = 5, 64
    what = (precision, t, v, e)
    got = _run(t, v, e, False, "real", precision, chunk_rows=3)
    _check_forward(got, _forward_reference(t, v, e, False, "real", precision), what)
    _check_grads(got, _reference(t, v, e, False, "real"), GRAD_LIMIT[precision], what)
    if v <= 32768:
        twice = _run(t, v, e, False, "real", precision, chunk_rows=3, rows_path="twice")
        for key in ("row_loss", "lse", "argmax", "d_hidden", "d_w"):
            assert torch.equal(got[key], twice[key]), (what, key)


# ---- 3. edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16", "f16"])
def test_large_logits_stay_finite(precision):
    """hidden x 30: |logits| in the hundreds"""
    t, v, e = SHAPES[1]
    got = _run(t, v, e, True, "real", precision, scale=30.0)
    ref = _forward_reference(t, v, e, True, "real", precision, 30.0)
    assert float(ref["lse"].abs().max()) > 100.0
    for key, x in got.items():
        assert bool(torch.isfinite(x.float()).all()), (precision, key)
    assert _rel(got["lse"], ref["lse"]) <= FWD_LIMIT, _rel(got["lse"], ref["lse"])


def test_labels_outside_the_vocabulary_are_an_all_zero_one_hot():
    t, v, e = SHAPES[0]
    hidden, w_out, labels, *_ = _inputs(t, v, e, False, None)
    labels = labels.clone()
    labels[0], labels[1], labels[2], labels[7] = v, -100, v + 12345, -1
    weight = 0.5 + torch.rand(t, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        want, row, lse, _ = _formula64(hidden.double(), w_out.double(), labels, None, None, None, weight)
    loss, stats = lm_head_loss(hidden.to(DEV), w_out.to(DEV), labels.to(DEV), weight=weight.to(DEV), precision="f32", chunk_rows=CHUNK)
    odd = torch.tensor([0, 1, 2, 7])
    assert torch.equal(stats["row_loss"].cpu()[odd], (weight.to(DEV) * stats["lse"]).cpu()[odd])          # w * lse, and no read at the label
    assert _rel(stats["row_loss"], row) <= FWD_LIMIT and abs(float(loss) - float(want)) <= FWD_LIMIT * float(want)


@pytest.mark.parametrize("precision", ["f32", "bf16"])
def test_a_zero_weight_sum_gives_zero_and_no_nan(precision):
    """Deviation from the reference (0 / 0 = NaN there): loss 0 and every gradient 0."""
    t, v, e = SHAPES[0]
    hidden, w_out, labels, bias, priors, vmask, _ = _inputs(t, v, e, True, None)
    h, w, b = hidden.to(DEV).requires_grad_(True), w_out.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)
    loss, stats = lm_head_loss(h, w, labels.to(DEV), weight=torch.zeros(t, device=DEV), bias=b, priors=priors.to(DEV), vocab_mask=vmask.to(DEV),
                               precision=precision, chunk_rows=CHUNK)
    loss.backward()
    assert float(loss) == 0.0 and int(stats["n_counted"]) == 0 and float(stats["weight_sum"]) == 0.0 and not stats["row_loss"].any()
    for x in (h.grad, w.grad, b.grad):
        assert bool(torch.isfinite(x).all()) and not x.any()


@pytest.mark.parametrize("hidden_dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["h_f32", "h_bf16", "h_f16"])
@pytest.mark.parametrize("precision", ["f32", "bf16", "f16"])
def test_every_hidden_dtype_with_every_precision(precision, hidden_dtype):
    """The forward is held against float64 on what the kernels see (hidden rounded to its own dtype, then to the operand type).  The
    gradients are held against float64 on the unrounded operands: hidden's own rounding and the rounding of d hidden to hidden's dtype
    add one more relative error of that format, so the limit is the sum of the precision's limit and the hidden dtype's."""
    t, v, e = SHAPES[1]
    got = _run(t, v, e, True, "real", precision, hidden_dtype=hidden_dtype)
    _check_forward(got, _forward_reference(t, v, e, True, "real", precision, 1.0, hidden_dtype), (precision, hidden_dtype))
    assert got["d_hidden"].dtype == hidden_dtype and got["d_w"].dtype == torch.float32
    extra = {torch.float32: 0.0, torch.bfloat16: GRAD_LIMIT["bf16"], torch.float16: GRAD_LIMIT["f16"]}[hidden_dtype]
    _check_grads(got, _reference(t, v, e, True, "real"), GRAD_LIMIT[precision] + extra, (precision, hidden_dtype))


# ---- 4. autograd --------------------------------------------------------------------------------------------------------------------
def test_upstream_scalar_accumulation_and_no_grad():
    t, v, e = SHAPES[0]
    hidden, w_out, labels, bias, priors, vmask, weight = _inputs(t, v, e, True, "real")
    args = dict(weight=weight.to(DEV), priors=priors.to(DEV), vocab_mask=vmask.to(DEV), precision="f32", chunk_rows=CHUNK)

    def leaves():
        return hidden.to(DEV).requires_grad_(True), w_out.to(DEV).requires_grad_(True), bias.to(DEV).requires_grad_(True)

    h1, w1, b1 = leaves()
    loss1, _ = lm_head_loss(h1, w1, labels.to(DEV), bias=b1, **args)
    loss1.backward()
    h3, w3, b3 = leaves()
    loss3, _ = lm_head_loss(h3, w3, labels.to(DEV), bias=b3, **args)
    (3.0 * loss3).backward()
    for one, three in ((h1, h3), (w1, w3), (b1, b3)):
        assert _rel(three.grad, 3.0 * one.grad) <= 1e-6
    # a second backward accumulates into the existing .grad
    first = [x.grad.clone() for x in (h1, w1, b1)]
    loss_again, _ = lm_head_loss(h1, w1, labels.to(DEV), bias=b1, **args)
    loss_again.backward()
    for x, g in zip((h1, w1, b1), first):
        assert _rel(x.grad, 2.0 * g) <= 1e-6
    # eval_step: the same bits, no graph, nothing saved
    with torch.no_grad():
        quiet, stats = lm_head_loss(h1, w1, labels.to(DEV), bias=b1, **args)
    assert torch.equal(quiet, loss1.detach()) and quiet.grad_fn is None and not quiet.requires_grad
    plain, _ = lm_head_loss(h1.detach(), w1.detach(), labels.to(DEV), bias=b1.detach(), **args)
    assert torch.equal(plain, quiet) and plain.grad_fn is None
    assert float(stats["n_correct"]) <= float(stats["n_counted"]) == t


def _tiny(seed, rows=64):          # (the case of tests/test_training_gpu.py)
    from zett_amd.config import ZettHypernetConfig
    from zett_amd.hypernet import ZettHypernet
    cfg, *_ = synth.workload("tiny")
    w = synth.make_weights(cfg, seed=seed)
    src = synth.make_source_embeddings(cfg, seed)
    ids = synth.make_surface_forms(cfg, rows, seed=seed, n_special=1)
    ids[::3, 1:] = cfg["pad_token_id"]                                  # single-token rows for the lexical loss
    models = []
    for _ in range(2):
        model = ZettHypernet(ZettHypernetConfig(**cfg))
        model.load_state_dict({k: torch.from_numpy(x) for k, x in w.items()})
        models.append(model.to(DEV).requires_grad_(True).train())
    return cfg, models, torch.from_numpy(src).to(DEV), torch.from_numpy(ids).to(DEV)


def test_training_a_tiny_hypernet_with_the_lm_loss():
    """lm_head_loss + 0.5 lexical_loss -> backward -> HypernetAdamW.step on the tiny hypernetwork; the first step's parameter gradients
    equal those obtained with torch's fp32 F.cross_entropy in place of lm_head_loss."""
    from zett_amd.training import HypernetAdamW, lexical_loss
    rows, t = 64, 96
    cfg, (ours, theirs), src, ids = _tiny(seed=83, rows=rows)
    pad, e = cfg["pad_token_id"], cfg["n_embd"]
    g = torch.Generator().manual_seed(1234)
    hidden = torch.randn(t, e, generator=g).to(DEV)
    labels = torch.randint(0, rows, (t,), generator=g).to(DEV)
    lang = torch.tensor(2)

    def total(model, use_torch):
        pred_in, pred_out, _bias = model(ids, source_embeddings=src, lang_index=lang)
        lm = F.cross_entropy(hidden @ pred_out.T, labels) if use_torch else lm_head_loss(hidden, pred_out, labels, precision="f32", chunk_rows=CHUNK)[0]
        return lm + 0.5 * lexical_loss(pred_in, pred_out, src, ids, pad)[0]

    total(theirs, True).backward()
    opt = HypernetAdamW(ours, lr=1e-3)
    losses = []
    for step in range(5):
        loss = total(ours, False)
        loss.backward()
        if step == 0:
            # A gradient that is zero in exact arithmetic — the key biases: softmax does not see a shift along the keys — is fp32
            # round-off on BOTH sides (the yardstick here is fp32 too); such a parameter is held to "negligible next to the largest
            # gradient" on both sides instead of to a relative error between two noises.
            want, worst = dict(theirs.named_parameters()), {}
            floor = 1e-6 * max(float(q.grad.double().norm()) for q in want.values() if q.grad is not None)
            for name, p in ours.named_parameters():
                if p.grad is None and want[name].grad is None:
                    continue
                ref = want[name].grad.double()
                if float(ref.norm()) < floor:
                    assert float(p.grad.double().norm()) < floor, (name, float(p.grad.double().norm()), floor)
                else:
                    worst[name] = _rel(p.grad, ref)
            bad = {k: x for k, x in worst.items() if x > GRAD_LIMIT["f32"]}
            assert not bad and len(worst) >= 40, bad
        opt.step(zero_grad=True)
        losses.append(loss.detach())
    losses = [float(x) for x in torch.stack(losses).cpu()]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert opt.last_step_stats()["step"] == 5


# ---- 5. the kernels shared with the primitives of zett_amd/autograd.py -------------------------------------------------------------
def _call_op(fn, *args):
    """a zett_op_* entry point on the NULL stream (the trailing stream argument), checked and waited for"""
    from zett_amd import _lib
    stream = None
    _lib.check(getattr(_lib.load(), fn)(*args, stream), fn)
    torch.cuda.synchronize()


def test_colsum_f32_and_ce_colsum_share_one_kernel():
    """zett_op_colsum_f32 and zett_op_ce_colsum(ZETT_F32) run the same kernel: the same bits, and — small integers, every fp32 sum
    exact — numpy's column sums.  65 columns reach into a second 64-column workgroup; 5 rows leave the four waves uneven shares."""
    from zett_amd import _lib
    rows, v, ld = 5, 65, 72
    x = np.random.default_rng(7).integers(-8, 9, size=(rows, ld)).astype(np.float32)
    start = np.arange(v, dtype=np.float32) - 30.0
    dx = torch.from_numpy(x).to(DEV)
    for accumulate in (0, 1):
        want = x[:, :v].sum(0) + (start if accumulate else 0.0)
        plain, ce = torch.from_numpy(start).to(DEV), torch.from_numpy(start).to(DEV)
        _call_op("zett_op_colsum_f32", dx.data_ptr(), ld, rows, v, plain.data_ptr(), accumulate)
        _call_op("zett_op_ce_colsum", dx.data_ptr(), _lib.DTYPE_F32, ld, rows, v, ce.data_ptr(), accumulate)
        assert np.array_equal(plain.cpu().numpy().view(np.uint32), ce.cpu().numpy().view(np.uint32)), accumulate
        assert np.array_equal(plain.cpu().numpy(), want.astype(np.float32)), accumulate


@pytest.mark.parametrize("cols", (5, 8))
@pytest.mark.parametrize("precision", ("f16", "bf16"))
def test_convert_lo_and_ce_cast_share_one_kernel(precision, cols):
    """zett_op_convert_lo and zett_op_ce_cast from fp32 give the same bits: cols = 5 of 8 is the general path of both (one kernel, a
    zero-filled pad), cols = 8 of 8 convert's float4 path against that kernel."""
    from zett_amd import _lib
    rows, cp = 3, 8
    prec, code = {"f16": (_lib.PREC_F16, _lib.DTYPE_F16), "bf16": (_lib.PREC_BF16, _lib.DTYPE_BF16)}[precision]
    x = (torch.randn(rows, cols, generator=torch.Generator().manual_seed(11)) * 3.0).to(DEV)
    a = torch.full((rows, cp), 7.0, device=DEV).to(LO[precision])          # (stale contents: the pad must be written)
    b = a.clone()
    _call_op("zett_op_convert_lo", prec, x.data_ptr(), cols, a.data_ptr(), cp, rows, cols, cp)
    _call_op("zett_op_ce_cast", x.data_ptr(), _lib.DTYPE_F32, cols, b.data_ptr(), code, cp, rows, cols, cp)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    assert torch.equal(a[:, :cols], x.to(LO[precision]))                    # round to nearest even, as torch's cast
    assert torch.equal(a.view(torch.int16)[:, cols:], torch.zeros(rows, cp - cols, dtype=torch.int16, device=DEV))
