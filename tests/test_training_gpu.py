"""zett_amd/training.py on the GPU: the identity / lexical losses and the clipped multi-tensor AdamW step (csrc/train_step.hip).
The yardstick everywhere is float64 torch on the CPU (or, in one test, torch.optim.AdamW on the GPU), written here — never the
kernels themselves."""
import itertools
import math

import numpy as np
import pytest
import torch

from tests import torch_port, util
from zett_amd import synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HUBER_DELTA, HUBER_CORRECTION, EPSILON = 1e-3, 30, 1e-8          # train.py:1107-1108, zett/utils.py:25
MEAN, LEXICAL = 0, 1
SRC_ROWS = 50


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / max(float(b.double().norm()), 1e-300))


# ---- 1. losses ------------------------------------------------------------------------------------------------------------------
def _distance64(pred, tgt, kind):
    e = pred - tgt
    if kind == "mse":
        return (e ** 2).sum(-1)
    if kind == "rmse":
        return torch.linalg.norm(e, dim=-1)                    # (torch's subgradient at e = 0 is 0: what the kernel documents)
    a = e.abs()
    q = a.clamp(max=HUBER_DELTA)
    return (0.5 * q ** 2 + HUBER_DELTA * (a - q)).sum(-1) / HUBER_DELTA / HUBER_CORRECTION


def _loss64(pred, src, col0, ids, mask, kind, mode):
    """float64 restatement of train.py:941-946 (mode MEAN) and train.py:1086-1125 (mode LEXICAL); pred requires grad."""
    e = pred.shape[1]
    tgt = src.double()[ids.long().clamp(0, src.shape[0] - 1), col0:col0 + e]
    d = _distance64(pred, tgt, kind)
    m = torch.ones(len(pred), dtype=torch.float64) if mask is None else mask.double()
    d = d * m
    if mode == MEAN:
        return d.mean()
    return d.sum() / (m.sum() + EPSILON) / torch.linalg.norm(tgt, dim=1).mean()


def _loss_case(n, e, dtype, col0, kind, seed):
    g = torch.Generator().manual_seed(seed)
    src = (torch.randn(SRC_ROWS, 2 * e, generator=g) * 0.05).to(dtype)
    ids = torch.randint(0, SRC_ROWS, (n,), generator=g)
    ids[-1] = SRC_ROWS + 7                                       # beyond the matrix: clamped to its last row
    if n > 2:
        ids[1] = -3                                              # below it: clamped to its first row
    tgt = src.float()[ids.clamp(0, SRC_ROWS - 1), col0:col0 + e]
    pred = tgt + torch.randn(n, e, generator=g) * 0.03
    pred[:, ::3] = tgt[:, ::3] + torch.randn(n, e, generator=g)[:, ::3] * 3e-4          # some errors inside huber's quadratic zone
    pred[0] = tgt[0]                                             # a row that equals its target (rmse: gradient 0, not NaN)
    mask = (torch.rand(n, generator=g) < 0.6).float()
    mask[0] = 1.0
    return src, ids, pred, mask


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
@pytest.mark.parametrize("kind", ["mse", "rmse", "huber"])
def test_losses_and_gradients_match_float64(kind, dtype):
    from zett_amd import training
    seed = 0
    for n, e, half, masked in itertools.product((1, 63, 300), (8, 64, 100, 768), (0, 1), (False, True)):
        seed += 1
        col0 = half * e
        src, ids, pred, mask = _loss_case(n, e, dtype, col0, kind, seed)
        if (seed // 2) % 2:                                       # int32 ids read with a stride (column 0 of a matrix) in half of the cases
            mat = torch.full((n, 3), -5, dtype=torch.int32)
            mat[:, 0] = ids.int()
            ids_d, stride = mat.to(DEV), 3
        else:
            ids_d, stride = ids.to(DEV), 1
        for m, mode in ((mask, LEXICAL), (None, LEXICAL)) if masked else ((None, MEAN),):
            what = (kind, str(dtype), n, e, col0, masked, mode)
            p64 = pred.double().requires_grad_(True)
            want = _loss64(p64, src, col0, ids, m, kind, mode)
            up = 0.37
            (want * up).backward()
            want = want.detach()
            pred_d, src_d, m_d = pred.to(DEV), src.to(DEV), None if m is None else m.to(DEV)
            record, row_dist, _ = training.embed_distance_forward(pred_d, src_d, col0, ids_d, stride, m_d, kind, mode)
            got = float(record[0])
            assert abs(got - float(want)) <= 1e-5 * abs(float(want)), (what, got, float(want))
            if m is not None:
                assert float(record[2]) == pytest.approx(float(m.mean()), rel=1e-6)
            upstream = torch.tensor(up, device=DEV)
            grad = training.embed_distance_backward(pred_d, src_d, col0, ids_d, stride, m_d, kind, row_dist, record, upstream)
            assert bool(torch.isfinite(grad).all()), what
            assert not grad[0].any(), what                         # pred == target: zero under every kind
            if float(p64.grad.norm()) == 0.0:
                assert not grad.any(), what
            else:
                assert _rel(grad, p64.grad) <= 1e-5, (what, _rel(grad, p64.grad))
            # the same bits on a second run; accumulate adds exactly what a plain call writes
            record2, row_dist2, _ = training.embed_distance_forward(pred_d, src_d, col0, ids_d, stride, m_d, kind, mode)
            grad2 = training.embed_distance_backward(pred_d, src_d, col0, ids_d, stride, m_d, kind, row_dist2, record2, upstream)
            assert torch.equal(record, record2) and torch.equal(row_dist, row_dist2) and torch.equal(grad, grad2), what
            before = torch.randn(n, e, device=DEV, generator=torch.Generator(device=DEV).manual_seed(seed)) * 0.01
            acc = training.embed_distance_backward(pred_d, src_d, col0, ids_d, stride, m_d, kind, row_dist, record, upstream, out=before.clone(), accumulate=True)
            assert torch.equal(acc, before + grad), what


@pytest.mark.parametrize("kind", ["mse", "rmse", "huber"])
def test_an_all_zero_mask_gives_exactly_zero(kind):
    from zett_amd import training
    src, ids, pred, _ = _loss_case(63, 100, torch.float32, 100, kind, seed=7)
    mask = torch.zeros(63, device=DEV)
    record, row_dist, _ = training.embed_distance_forward(pred.to(DEV), src.to(DEV), 100, ids.to(DEV), 1, mask, kind, LEXICAL)
    assert float(record[0]) == 0.0 and float(record[2]) == 0.0
    grad = training.embed_distance_backward(pred.to(DEV), src.to(DEV), 100, ids.to(DEV), 1, mask, kind, row_dist, record, torch.ones((), device=DEV))
    assert bool(torch.isfinite(grad).all()) and not grad.any()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_unaligned_rows_take_the_scalar_path(dtype):
    """Widths that are no multiple of 4 and a prediction matrix that starts one element into its storage."""
    from zett_amd import training
    for n, e, col0 in ((5, 10, 10), (63, 7, 0), (9, 64, 64)):
        src, ids, pred, mask = _loss_case(n, e, dtype, col0, "mse", seed=n)
        store = torch.zeros(n * e + 1, device=DEV)
        pred_d = store[1:].view(n, e)
        pred_d.copy_(pred)
        p64 = pred.double().requires_grad_(True)
        want = _loss64(p64, src, col0, ids, mask, "mse", LEXICAL)
        want.backward()
        want = want.detach()
        record, row_dist, _ = training.embed_distance_forward(pred_d, src.to(DEV), col0, ids.to(DEV), 1, mask.to(DEV), "mse", LEXICAL)
        assert abs(float(record[0]) - float(want)) <= 1e-5 * abs(float(want))
        out = torch.zeros(n * e + 1, device=DEV)[1:].view(n, e)
        training.embed_distance_backward(pred_d, src.to(DEV), col0, ids.to(DEV), 1, mask.to(DEV), "mse", row_dist, record, torch.ones((), device=DEV), out=out)
        assert _rel(out, p64.grad) <= 1e-5


def test_public_losses_respect_an_upstream_scalar_and_match_float64():
    from zett_amd import training
    n, e, pad = 63, 64, 1
    g = torch.Generator().manual_seed(11)
    src = torch.randn(SRC_ROWS, 2 * e, generator=g) * 0.05
    tsf = torch.randint(2, SRC_ROWS, (n, 5), generator=g)
    tsf[::2, 1:] = pad                                           # every other row is a single token
    tsf[4, 0] = SRC_ROWS + 3                                     # ... one of them a fallback id: the last source row (JAX's clamp)
    pin, pout = (torch.randn(n, e, generator=g) * 0.05 for _ in range(2))
    mask = (tsf[:, 1:] == pad).all(1)
    for kind in ("mse", "rmse", "huber"):
        a64, b64 = pin.double().requires_grad_(True), pout.double().requires_grad_(True)
        lex = (_loss64(a64, src, 0, tsf[:, 0], mask, kind, LEXICAL) + _loss64(b64, src, e, tsf[:, 0], mask, kind, LEXICAL)) / 2
        ident = (_loss64(a64, src, 0, tsf[:, 0], None, "mse", MEAN) + _loss64(b64, src, e, tsf[:, 0], None, "mse", MEAN)) / 2
        (0.5 * lex + 3.0 * ident).backward()
        a, b = pin.to(DEV).requires_grad_(True), pout.to(DEV).requires_grad_(True)
        got_lex, overlap = training.lexical_loss(a, b, src.to(DEV), tsf.to(DEV), pad, kind=kind)
        got_ident = training.identity_loss(a, b, src.to(DEV), tsf[:, 0].to(DEV).clamp(max=SRC_ROWS - 1))
        assert got_lex.dim() == 0 and got_lex.is_cuda and not overlap.requires_grad
        (0.5 * got_lex + 3.0 * got_ident).backward()
        assert float(got_lex.detach()) == pytest.approx(float(lex.detach()), rel=1e-5) and float(got_ident.detach()) == pytest.approx(float(ident.detach()), rel=1e-5)
        assert float(overlap) == pytest.approx(float(mask.double().mean()), rel=1e-6)
        assert _rel(a.grad, a64.grad) <= 1e-5 and _rel(b.grad, b64.grad) <= 1e-5
    # tied embeddings: the input half alone
    a64 = pin.double().requires_grad_(True)
    a = pin.to(DEV).requires_grad_(True)
    tied = training.identity_loss(a, None, src.to(DEV), tsf[:, 1].to(DEV))
    assert float(tied.detach()) == pytest.approx(float(_loss64(a64, src, 0, tsf[:, 1], None, "mse", MEAN).detach()), rel=1e-5)


# ---- 2.-4. the optimizer ----------------------------------------------------------------------------------------------------------
class _Bag(torch.nn.Module):
    """Named parameters and a refresh_weights() counter: what HypernetAdamW needs of a model."""

    def __init__(self, tensors):
        super().__init__()
        for name, t in tensors.items():
            self.register_parameter(name, torch.nn.Parameter(t))
        self.refreshed = 0

    def refresh_weights(self):
        self.refreshed += 1


def _adamw64(P, G, M, V, labels, t, lr, b1, b2, eps, wd, max_norm):
    """optax.chain(clip_by_global_norm, multi_transform({train: adamw(mask), freeze: set_to_zero})) in float64, in place."""
    norm = math.sqrt(sum(float((g ** 2).sum()) for g in G.values()))          # every gradient, frozen tensors included
    coef = 1.0 if norm < max_norm else max_norm / norm
    for k in P:
        if labels[k] == "frozen":
            continue
        g = G[k] * coef
        M[k] = b1 * M[k] + (1 - b1) * g
        V[k] = b2 * V[k] + (1 - b2) * g * g
        P[k] -= lr * ((M[k] / (1 - b1 ** t)) / ((V[k] / (1 - b2 ** t)).sqrt() + eps) + (wd if labels[k] == "decay" else 0.0) * P[k])
    return norm, coef


SHAPES = {"one": (1,), "three": (3,), "b64": (64,), "odd129": (129,), "wide": (257, 128), "tall": (300, 64), "offset": (64,), "norm_like": (129,),
          "frozen": (300, 64), "chunks": (2 * 65536 + 5,)}
BAG_LABELS = {"one": "no_decay", "three": "decay", "b64": "no_decay", "odd129": "decay", "wide": "decay", "tall": "no_decay", "offset": "decay",
              "norm_like": "no_decay", "frozen": "frozen", "chunks": "decay"}


def _bag(seed):
    g = torch.Generator().manual_seed(seed)
    init = {k: torch.randn(s, generator=g) * 0.02 for k, s in SHAPES.items()}
    init["norm_like"] = torch.ones(SHAPES["norm_like"])          # LayerNorm-like: values at 1.0, where an fp32 step rounds coarsest
    dev = {k: v.to(DEV) for k, v in init.items()}
    store = torch.zeros(65, device=DEV)
    store[1:].copy_(init["offset"])
    dev["offset"] = store[1:]                                    # a view one element into its storage: 4-byte aligned only
    return init, _Bag(dev)


def _set_grads(bag, grads):
    for k, p in bag.named_parameters():
        if k == "offset":                                       # the gradient, too, one element into its storage
            p.grad = torch.zeros(65, device=DEV)[1:].copy_(grads[k])
        else:
            p.grad = grads[k].to(DEV).clone()


@pytest.mark.parametrize("scale", [1.0, 1e-3, 1e-6])
def test_adamw_steps_match_float64(scale):
    from zett_amd.training import HypernetAdamW
    lr, b1, b2, eps, wd, max_norm = 1e-2, 0.9, 0.95, 1e-8, 0.01, 0.1
    init, bag = _bag(seed=3)
    assert bag.offset.data_ptr() % 16 == 4
    opt = HypernetAdamW(bag, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, max_grad_norm=max_norm, labels=BAG_LABELS)
    P = {k: v.double().clone() for k, v in init.items()}
    M = {k: torch.zeros_like(v) for k, v in P.items()}
    V = {k: torch.zeros_like(v) for k, v in P.items()}
    g = torch.Generator().manual_seed(17)
    for t in (1, 2, 3):
        G32 = {k: torch.randn(s, generator=g) * scale for k, s in SHAPES.items()}
        params = dict(bag.named_parameters())
        _set_grads(bag, G32)
        norm, coef = _adamw64(P, {k: v.double() for k, v in G32.items()}, M, V, BAG_LABELS, t, lr, b1, b2, eps, wd, max_norm)
        opt.step(zero_grad=(t == 2))
        stats = opt.last_step_stats()
        assert stats["grad_norm"] == pytest.approx(norm, rel=1e-6) and stats["clip_coef"] == pytest.approx(coef, rel=1e-6)
        assert stats["skipped"] == 0 and stats["step"] == t and bag.refreshed == t
        assert (coef < 1.0) == (scale >= 1e-3)                  # scale 1 clips (and 1e-3 still does), scale 1e-6 does not
        if t == 2:
            assert all(not p.grad.any() for p in params.values())       # zeroed in the same pass, frozen ones too
        else:
            assert all(torch.equal(p.grad.cpu(), G32[k]) for k, p in params.items())
    params = dict(bag.named_parameters())
    assert torch.equal(params["frozen"].cpu(), init["frozen"]) and "frozen" not in opt.state
    worst = {}
    for k in SHAPES:
        if BAG_LABELS[k] == "frozen":
            continue
        moved = float((P[k] - init[k].double()).norm())
        worst[k] = max(float((params[k].detach().double().cpu() - P[k]).norm()) / moved,
                       _rel(opt.state[k]["exp_avg"], M[k]), _rel(opt.state[k]["exp_avg_sq"], V[k]))
    assert max(worst.values()) <= 5e-5, worst


def _tiny_pair(seed):
    from zett_amd.config import ZettHypernetConfig
    from zett_amd.hypernet import ZettHypernet
    cfg, *_ = synth.workload("tiny")
    w = synth.make_weights(cfg, seed=seed)
    models = []
    for _ in range(2):
        m = ZettHypernet(ZettHypernetConfig(**cfg))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
        models.append(m.to(DEV).requires_grad_(True).train())
    return cfg, models


def test_adamw_matches_torch_adamw_on_the_whole_model():
    """The tiny model, identical .grad tensors: optax-style clip in torch + torch.optim.AdamW (decay / no_decay groups, frozen
    parameters left out) against one HypernetAdamW.step."""
    from zett_amd.training import HypernetAdamW, param_labels
    lr, betas, eps, wd, max_norm = 1e-2, (0.9, 0.95), 1e-8, 0.01, 0.1
    cfg, (ours, theirs) = _tiny_pair(seed=5)
    labels = param_labels(ours)
    init = {k: p.detach().clone() for k, p in ours.named_parameters()}
    tp = dict(theirs.named_parameters())
    ref = torch.optim.AdamW([{"params": [tp[k] for k, l in labels.items() if l == "decay"], "weight_decay": wd},
                             {"params": [tp[k] for k, l in labels.items() if l == "no_decay"], "weight_decay": 0.0}], lr=lr, betas=betas, eps=eps)
    opt = HypernetAdamW(ours, lr=lr, betas=betas, eps=eps, weight_decay=wd, max_grad_norm=max_norm)
    gen = torch.Generator(device=DEV).manual_seed(23)
    for t, scale in enumerate((1.0, 1e-3, 1e-5)):
        grads = {k: torch.randn(p.shape, device=DEV, generator=gen) * scale for k, p in init.items()}
        norm = torch.sqrt(sum((g.double() ** 2).sum() for g in grads.values()))
        coef = 1.0 if float(norm) < max_norm else max_norm / float(norm)
        for k, p in ours.named_parameters():
            p.grad = grads[k].clone()
            tp[k].grad = grads[k] * coef
        opt.step()
        ref.step()
        assert opt.last_step_stats()["grad_norm"] == pytest.approx(float(norm), rel=1e-6)
    worst = {}
    for k, p in ours.named_parameters():
        if labels[k] == "frozen":
            assert torch.equal(p, init[k]), k
            continue
        moved = float((tp[k].detach().double() - init[k].double()).norm())
        worst[k] = float((p.detach().double() - tp[k].detach().double()).norm()) / moved
    assert len(worst) == 83 and max(worst.values()) <= 5e-5, {k: v for k, v in worst.items() if v > 5e-5}


def test_a_non_finite_gradient_skips_the_step():
    from zett_amd.training import HypernetAdamW
    init, bag = _bag(seed=9)
    opt = HypernetAdamW(bag, lr=1e-2, labels=BAG_LABELS)
    g = torch.Generator().manual_seed(1)
    _set_grads(bag, {k: torch.randn(s, generator=g) * 1e-3 for k, s in SHAPES.items()})
    opt.step()
    assert opt.last_step_stats()["skipped"] == 0 and opt.last_step_stats()["step"] == 1
    snap = {k: p.detach().clone() for k, p in bag.named_parameters()}
    moments = {k: {n: t.clone() for n, t in st.items()} for k, st in opt.state.items()}
    dict(bag.named_parameters())["wide"].grad[100, 7] = float("inf")
    opt.step(zero_grad=True)
    stats = opt.last_step_stats()
    assert stats["skipped"] == 1 and stats["step"] == 1 and not math.isfinite(stats["grad_norm"])
    for k, p in bag.named_parameters():
        assert torch.equal(p.detach(), snap[k]), k
    for k, st in opt.state.items():
        assert torch.equal(st["exp_avg"], moments[k]["exp_avg"]) and torch.equal(st["exp_avg_sq"], moments[k]["exp_avg_sq"]), k
    # ... but the gradients the caller asked to clear ARE cleared, the non-finite one and the frozen tensor's included: what the next
    # backward accumulates into (torch adds to an allocated .grad in place) is zeros, and the step after it is taken, from step 1
    kept = {k: p.grad for k, p in bag.named_parameters()}
    assert all(not g.any() for g in kept.values())
    for p in bag.parameters():
        p.grad += torch.full_like(p, 1e-3)
    assert all(p.grad is kept[k] for k, p in bag.named_parameters())
    opt.step()
    stats = opt.last_step_stats()
    assert stats["skipped"] == 0 and stats["step"] == 2 and math.isfinite(stats["grad_norm"])
    assert not torch.equal(dict(bag.named_parameters())["wide"].detach(), snap["wide"])
    assert torch.equal(dict(bag.named_parameters())["frozen"].detach(), snap["frozen"])
    # without zero_grad a skipped step writes nothing at all
    dict(bag.named_parameters())["odd129"].grad[5] = float("nan")
    grads = {k: p.grad.clone() for k, p in bag.named_parameters()}
    snap = {k: p.detach().clone() for k, p in bag.named_parameters()}
    opt.step()
    assert opt.last_step_stats()["skipped"] == 1 and opt.last_step_stats()["step"] == 2
    for k, p in bag.named_parameters():
        assert torch.equal(p.detach(), snap[k]) and torch.equal(p.grad.nan_to_num(7.0), grads[k].nan_to_num(7.0)), k


def test_optimizer_state_round_trip():
    from zett_amd.training import HypernetAdamW
    _, bag = _bag(seed=13)
    _, twin = _bag(seed=13)
    a, b = HypernetAdamW(bag, lr=1e-2, labels=BAG_LABELS), HypernetAdamW(twin, lr=5.0, labels=BAG_LABELS)
    gen = torch.Generator(device=DEV).manual_seed(2)
    grads = [{k: torch.randn(s, device=DEV, generator=gen) * 1e-3 for k, s in SHAPES.items()} for _ in range(2)]
    _set_grads(bag, grads[0])
    a.step()
    sd = a.state_dict()
    assert sd["step"] == 1
    with torch.no_grad():
        for (k, p), q in zip(bag.named_parameters(), twin.parameters()):
            q.copy_(p)
    b.load_state_dict(sd)
    for opt, model in ((a, bag), (b, twin)):
        _set_grads(model, grads[1])
        opt.step()
    assert b.last_step_stats() == a.last_step_stats() and a.last_step_stats()["step"] == 2
    for p, q in zip(bag.parameters(), twin.parameters()):
        assert torch.equal(p, q)


# ---- 5. identity warm-up end to end ------------------------------------------------------------------------------------------------
def _case(flags, seed, rows=24):          # (the case of tests/test_autograd_gpu.py)
    cfg, *_ = synth.workload("tiny")
    cfg = dict(cfg, **flags)
    w = synth.make_weights(cfg, seed=seed)
    src = synth.make_source_embeddings(cfg, seed)
    ids = synth.make_surface_forms(cfg, rows, seed=seed, n_special=1)
    ids[2, 1] = cfg["original_vocab_size"] + 2                       # a fallback id
    return cfg, w, src, ids


def _model(cfg, w):
    from zett_amd.config import ZettHypernetConfig
    from zett_amd.hypernet import ZettHypernet
    model = ZettHypernet(ZettHypernetConfig(**cfg))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return model.to(DEV).requires_grad_(True).train()


def test_identity_warm_up_end_to_end():
    """identity_train_step (train.py:914-975): forward, identity_loss, backward, HypernetAdamW.step — 20 times."""
    from zett_amd.training import HypernetAdamW, identity_loss
    cfg, w, src_np, ids_np = _case({}, seed=61, rows=64)
    e = cfg["n_embd"]
    ids_to_embed_np = np.random.default_rng(3).integers(0, cfg["original_vocab_size"], 64)
    W64 = {k: torch.from_numpy(v).double() for k, v in w.items()}
    pin, pout, _ = torch_port.forward(W64, cfg, torch.from_numpy(ids_np).long(), torch.from_numpy(src_np), 1)
    tgt = torch.from_numpy(src_np).double()[torch.from_numpy(ids_to_embed_np)]
    want = float((((pin - tgt[:, :e]) ** 2).sum(-1).mean() + ((pout - tgt[:, e:]) ** 2).sum(-1).mean()) / 2)
    model = _model(cfg, w)
    model.precision = "f32"
    src, ids, ids_to_embed, lang = torch.from_numpy(src_np).to(DEV), torch.from_numpy(ids_np).to(DEV), torch.from_numpy(ids_to_embed_np).to(DEV), torch.tensor(1)
    with torch.no_grad():
        before = model(ids, source_embeddings=src, lang_index=lang)
    opt = HypernetAdamW(model, lr=3e-4)
    losses = []
    torch.cuda.synchronize()
    for _ in range(20):
        pred_in, pred_out, _bias = model(ids, source_embeddings=src, lang_index=lang)      # (validates its ids on the host: one read per step)
        torch.cuda.set_sync_debug_mode("error")                  # the loss, the backward and the step never wait for the host
        try:
            loss = identity_loss(pred_in, pred_out, src, ids_to_embed)
            loss.backward()
            opt.step(zero_grad=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        losses.append(loss.detach())
    losses = [float(l) for l in torch.stack(losses).cpu()]        # the one read of the losses
    util.assert_f32_close(np.float32(losses[0]), np.float64(want), "identity loss at step 0")
    assert losses[1] < losses[0] and losses[-1] < 0.9 * losses[0] and all(np.isfinite(losses)), losses
    stats = opt.last_step_stats()
    assert stats["step"] == 20 and stats["skipped"] == 0 and stats["clip_coef"] < 1.0
    with torch.no_grad():
        after = model(ids, source_embeddings=src, lang_index=lang)
    assert not after[0].requires_grad and not torch.equal(before[0], after[0])          # the engine was refreshed: new weights
    frozen = dict(model.named_parameters())
    for name in ("scaler.w", "scaler.b", "in_scaler.w", "in_scaler.b"):
        assert torch.equal(frozen[name].detach().cpu(), torch.from_numpy(w[name])), name


# ---- 6. the lexical loss next to another loss ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mse", "huber"])
def test_lexical_loss_composes_with_another_loss(kind):
    from zett_amd.training import lexical_loss
    cfg, w, src_np, ids_np = _case({}, seed=71, rows=64)
    pad, e, v0 = cfg["pad_token_id"], cfg["n_embd"], cfg["original_vocab_size"]
    ids_np[::3, 1:] = pad                                        # single-token rows
    ids_np[6, 0] = v0 + 1                                        # ... one of them a fallback id: its target is the last source row
    ids64, src64 = torch.from_numpy(ids_np).long(), torch.from_numpy(src_np)
    W64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in w.items()}
    pin, pout, _ = torch_port.forward(W64, cfg, ids64, src64, 2)
    mask = (ids64[:, 1:] == pad).all(1)
    lex = (_loss64(pin, src64, 0, ids64[:, 0], mask, kind, LEXICAL) + _loss64(pout, src64, e, ids64[:, 0], mask, kind, LEXICAL)) / 2
    total64 = (pin ** 2).mean() + 0.5 * lex
    total64.backward()
    model = _model(cfg, w)
    src, ids = src64.to(DEV), torch.from_numpy(ids_np).to(DEV)
    pred_in, pred_out, _bias = model(ids, source_embeddings=src, lang_index=torch.tensor(2))
    got_lex, overlap = lexical_loss(pred_in, pred_out, src, ids, pad, kind=kind)
    total = (pred_in ** 2).mean() + 0.5 * got_lex
    total.backward()
    assert float(overlap) == pytest.approx(float(mask.double().mean()), rel=1e-6) and float(overlap) >= 1 / 3
    assert float(total.detach()) == pytest.approx(float(total64.detach()), rel=1e-4)
    params = dict(model.named_parameters())
    worst = {}
    for name, p64 in W64.items():
        if name not in params or (params[name].grad is None and p64.grad is None):
            continue
        g_ref = torch.zeros_like(p64) if p64.grad is None else p64.grad
        assert params[name].grad is not None, name
        denom = float(g_ref.norm())
        err = float((params[name].grad.double().cpu() - g_ref).norm())
        if denom < 1e-12:
            assert err < 1e-6, (name, err)
        else:
            worst[name] = err / denom
    bad = {k: v for k, v in worst.items() if v > 2e-4}
    assert not bad and len(worst) >= 40, bad
