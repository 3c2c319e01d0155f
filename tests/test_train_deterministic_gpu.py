"""The order-stable mode of the hypernetwork's backward on the GPU (ZettHypernet.train_deterministic, zett_amd/autograd.py
deterministic=True): its sums are pinned BIT FOR BIT to their definition (tests/embed_lookup_ref.py::embed_bwd_ref — ascending
positions, fp32 partials of 64, partials in ascending order), not held to a bound: Ops.index_sum_rows and the fallback gradient as
primitives, the two sums inside a whole step from the captured gradient they add up, every parameter gradient against float64 autograd,
repeatability of a step including the AdamW update, and the default mode left as it was."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import torch_port
from tests import train_ops_check as tc
from tests.embed_lookup_ref import embed_bwd_ref
from tests.train_deterministic_cases import (FB_64, FB_65, FB_E_IN, FB_NONE, FB_ROWS, FB_T, FB_V0, SUM_CASES, bits, fallback_dx, fallback_ids,
                                             sum_case)
from zett_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ops(precision="f32"):
    from zett_amd.autograd import Ops
    return Ops(torch.device(DEV), precision)


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ---- the primitives ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SUM_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_index_sum_rows_is_the_defined_sum_bit_for_bit(case):
    t, n_dst, cols, _ = case
    idx, src, want = sum_case(t, n_dst, cols)
    ops = _ops()
    I, S = idx.to(DEV), src.to(DEV)
    runs = [ops.index_sum_rows(I, S, n_dst) for _ in range(3)]
    got = runs[0]
    assert got.shape == (n_dst, cols) and got.dtype == torch.float32
    diff = bits(got) != want.view(np.int32)
    assert not diff.any(), (case, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert _same_bits(runs[1], got) and _same_bits(runs[2], got)          # three runs of the same input
    assert _same_bits(ops.index_sum_rows(I.long(), S, n_dst), got)          # int64 indices: the same plan
    # a shifted index array: the rows of idx + 1000 over [1000, 1000 + n_dst) are the rows of idx over [0, n_dst)
    assert _same_bits(ops.index_sum_rows(I + 1000, S, n_dst, id_base=1000), got)


@pytest.mark.parametrize("e_in", FB_E_IN)
@pytest.mark.parametrize("src_kind", ("f32", "f16", "bf16"))
def test_fallback_gradient_is_the_defined_sum_and_prod_keep_are_unchanged(src_kind, e_in):
    """ids around v0 (v0 - 1 and v0 both present), one fallback id with exactly 64 uses, one with 65, one with none: dfallback bit for
    bit the defined sum of dx over ids - v0; prod and keep bit for bit what zett_op_gather_bwd_f32 is held to."""
    from zett_amd import _lib
    lib = _lib.load()
    dtype, code = {"f32": (torch.float32, _lib.DTYPE_F32), "f16": (torch.float16, _lib.DTYPE_F16), "bf16": (torch.bfloat16, _lib.DTYPE_BF16)}[src_kind]
    ids, dx = fallback_ids(), fallback_dx(e_in)
    src = torch.randn(FB_V0, e_in, generator=torch.Generator().manual_seed(e_in + 5)).to(dtype)
    ops = _ops()
    IDS, SRC, DX = ids.to(DEV), src.to(DEV), dx.to(DEV)
    prod, keep = (torch.full((FB_T, e_in), float("nan"), device=DEV) for _ in range(2))
    ptr = lambda x: C.c_void_p(x.data_ptr())          # noqa: E731
    rc = lib.zett_op_gather_bwd_rows_f32(ptr(IDS), FB_T, ptr(SRC), code, e_in, FB_V0, ptr(DX), ptr(prod), ptr(keep), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.zett_last_error().decode()
    ref = tc.gather_bwd_ref(ids, src, FB_V0, FB_ROWS, dx, torch.zeros(FB_ROWS, e_in))
    name = f"gather_bwd_rows {src_kind} e_in={e_in}"
    tc.exact(prod.cpu(), ref["prod"], name + " prod")
    tc.exact(keep.cpu(), ref["keep"], name + " keep")
    dfb, dsw, dsb = ops.gather_bwd(IDS, SRC, FB_V0, DX, FB_ROWS, deterministic=True)
    want = embed_bwd_ref(ids.long().numpy() - FB_V0, dx.numpy(), FB_ROWS)
    assert dfb.shape == (FB_ROWS, e_in)
    diff = bits(dfb) != want.view(np.int32)
    assert not diff.any(), (name, int(diff.sum()), np.argwhere(diff)[:4].tolist())
    assert not bits(dfb[FB_NONE - FB_V0]).any() and bits(dfb[FB_64 - FB_V0]).any() and bits(dfb[FB_65 - FB_V0]).any()
    _, dsw_a, dsb_a = ops.gather_bwd(IDS, SRC, FB_V0, DX, FB_ROWS)          # the default entry point: the same prod / keep, so the same column sums
    assert _same_bits(dsw, dsw_a) and _same_bits(dsb, dsb_a)
    # no fallback id at all: zeros
    dfb0, _, _ = ops.gather_bwd(IDS.clamp(max=FB_V0 - 1), SRC, FB_V0, DX, FB_ROWS, deterministic=True)
    assert dfb0.shape == (FB_ROWS, e_in) and not bits(dfb0).any()


# ---- the whole hypernetwork ----------------------------------------------------------------------------------------------------
ROWS = 300
FLAGS = {"default": {}, "no-lang": dict(hn_embed_lang_id=False), "no-rescale": dict(hn_rescale_embeddings=False)}
PACKED_ONLY = ("input_projection.", "fallback_embeddings.", "in_scaler.", "model.embeddings.position_embeddings.", "model.embeddings.token_type_embeddings.",
               "lang_embeddings.")          # what lies behind the packed schedule's two index sums
DENSE_ONLY = ("fallback_embeddings.",)


@functools.lru_cache(maxsize=None)
def _case(flag_key):
    """300 rows of L = 7: every position takes up to 300 addends, fallback id v0 + 2 has 100 uses, v0 + 3 has 65.
    -> cfg, weights, source, ids (numpy), lang"""
    cfg, *_ = synth.workload("tiny")
    cfg = dict(cfg, **FLAGS[flag_key])
    w = synth.make_weights(cfg, seed=61)
    src = synth.make_source_embeddings(cfg, 61)
    ids = synth.make_surface_forms(cfg, ROWS, seed=61, n_special=1)
    v0 = cfg["original_vocab_size"]
    ids[50:150, 1] = v0 + 2
    ids[150:215, 0] = v0 + 3
    return cfg, w, src, ids, (2 if cfg.get("hn_embed_lang_id") else None)


def _cotangents(ref):
    gen = torch.Generator().manual_seed(5)
    return [None if r is None else torch.randn(r.shape, generator=gen, dtype=torch.float64) for r in ref]


@functools.lru_cache(maxsize=None)
def _reference_grads(flag_key):
    """float64 torch autograd of tests/torch_port.py: computed once per flag set, shared by both schedules"""
    cfg, w, src, ids, lang = _case(flag_key)
    W64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in w.items()}
    ref = torch_port.forward(W64, cfg, torch.from_numpy(ids).long(), torch.from_numpy(src), lang)
    sum((r * c).sum() for r, c in zip(ref, _cotangents(ref)) if r is not None).backward()
    return {k: (None if p.grad is None else p.grad.detach()) for k, p in W64.items()}, tuple(None if r is None else tuple(r.shape) for r in ref)


def _model(flag_key, packed, deterministic, precision="f32"):
    from zett_amd.config import ZettHypernetConfig
    from zett_amd.hypernet import ZettHypernet
    cfg, w, *_ = _case(flag_key)
    model = ZettHypernet(ZettHypernetConfig(**cfg))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    model = model.to(DEV).requires_grad_(True).train()
    model.train_packed, model.train_precision = packed, precision
    if deterministic:
        model.train_deterministic = True
    return model


def _step(model, flag_key):
    """one forward + backward with the shared cotangents -> {name: gradient}"""
    cfg, w, src, ids, lang = _case(flag_key)
    model.zero_grad(set_to_none=True)
    out = model(torch.from_numpy(ids).to(DEV), source_embeddings=torch.from_numpy(src).to(DEV), lang_index=None if lang is None else torch.tensor(lang))
    cot = _cotangents([None if o is None else o.detach().cpu() for o in out])
    sum((o.double() * c.to(DEV)).sum() for o, c in zip(out, cot) if o is not None).backward()
    torch.cuda.synchronize()
    return {n: p.grad for n, p in model.named_parameters() if p.grad is not None}


def _against_float64(grads, flag_key, lim):
    ref, _ = _reference_grads(flag_key)
    worst = {}
    for name, g_ref in ref.items():
        if name not in grads:
            continue
        g_ref = torch.zeros_like(grads[name], dtype=torch.float64, device="cpu") if g_ref is None else g_ref
        denom, err = float(g_ref.norm()), float((grads[name].double().cpu() - g_ref).norm())
        if denom < 1e-12:
            assert err < 1e-6, (name, err)
        else:
            worst[name] = err / denom
    bad = {k: v for k, v in worst.items() if v > lim}
    assert not bad and len(worst) >= 35, (bad, len(worst))


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "dense"])
@pytest.mark.parametrize("flag_key", sorted(FLAGS))
def test_every_gradient_in_deterministic_mode_matches_float64_autograd(flag_key, packed):
    """the limits of tests/test_autograd_gpu.py: rel-L2 2e-4 per parameter in f32"""
    _against_float64(_step(_model(flag_key, packed, True), flag_key), flag_key, 2e-4)


def test_every_gradient_in_deterministic_mode_bf16():
    """bf16 operands in every contraction: the 16-bit limit of tests/test_autograd_gpu.py (6e-2)"""
    _against_float64(_step(_model("default", True, True, "bf16"), "default"), "default", 6e-2)


class _Capture:
    """wraps methods of Ops for the length of a test: records (arguments, result) of every call"""

    def __init__(self, monkeypatch, *names):
        from zett_amd.autograd import Ops
        self.calls = {n: [] for n in names}
        for n in names:
            monkeypatch.setattr(Ops, n, self._wrap(n, getattr(Ops, n)))

    def _wrap(self, name, orig):
        def f(ops, *a, **k):
            out = orig(ops, *a, **k)
            self.calls[name].append((a, k, out))
            return out
        return f


def test_the_packed_sums_inside_the_step_are_the_defined_ones(monkeypatch):
    """demb — what the embeddings' LayerNorm backward returns — summed per position and per distinct id: the position embeddings'
    gradient and the language embedding's row are bit for bit embed_bwd_ref of the captured demb."""
    from zett_amd import autograd
    cfg, w, src, ids, lang = _case("default")
    model = _model("default", True, True)
    cap = _Capture(monkeypatch, "layernorm_bwd", "index_sum_rows")
    grads = _step(model, "default")
    gamma = model.get_parameter("model.embeddings.LayerNorm.weight").data_ptr()
    demb = [out[0] for a, _, out in cap.calls["layernorm_bwd"] if a[3].data_ptr() == gamma]
    assert len(demb) == 1
    demb = demb[0]
    L, lam = ids.shape[1], 1
    plan = autograd.plan_packed(torch.from_numpy(ids).to(DEV), cfg["pad_token_id"], lam)
    tok_pos = plan["tok_pos"].cpu().numpy()
    assert demb.shape == (tok_pos.size, cfg["hn_hidden_size"]) and np.bincount(tok_pos, minlength=L + 1)[0] == ROWS          # > 64 addends per position
    want = embed_bwd_ref(tok_pos, demb.cpu().numpy(), L + lam)
    dpos = grads["model.embeddings.position_embeddings.weight"]
    assert np.array_equal(bits(dpos[:L]), want[:L].view(np.int32))
    assert not bits(dpos[L:]).any()
    # the sums were taken from exactly that tensor, and the second one (per distinct id + the language row) is the defined sum too
    (a0, _, _), (a1, _, out1) = cap.calls["index_sum_rows"]
    assert a0[1].data_ptr() == demb.data_ptr() and a1[1].data_ptr() == demb.data_ptr() and np.array_equal(a0[0].cpu().numpy(), tok_pos)
    slot, n_dst = a1[0].cpu().numpy(), a1[2]
    assert np.array_equal(bits(out1), embed_bwd_ref(slot, demb.cpu().numpy(), n_dst).view(np.int32))
    assert np.array_equal(bits(grads["lang_embeddings.weight"][lang]), bits(out1[n_dst - 1]))


def test_the_dense_fallback_sum_inside_the_step_is_the_defined_one(monkeypatch):
    """dx0 — the gradient of the gathered source rows — summed per fallback id over all n * L positions: bit for bit embed_bwd_ref"""
    cfg, w, src, ids, lang = _case("default")
    model = _model("default", False, True)
    cap = _Capture(monkeypatch, "gather_bwd")
    grads = _step(model, "default")
    (a, k, _), = cap.calls["gather_bwd"]
    assert k.get("deterministic") is True
    flat, dx0, v0, n_fb = a[0].cpu().numpy(), a[3].cpu().numpy(), a[2], a[4]
    assert np.array_equal(flat, ids.reshape(-1)) and v0 == cfg["original_vocab_size"]
    assert np.bincount(flat[flat >= v0] - v0, minlength=n_fb)[2] >= 100 and np.bincount(flat[flat >= v0] - v0, minlength=n_fb)[3] >= 65
    want = embed_bwd_ref(flat.astype(np.int64) - v0, dx0, n_fb)
    assert np.array_equal(bits(grads["fallback_embeddings.weight"]), want.view(np.int32))


@pytest.mark.parametrize("packed", [True, False], ids=["packed", "dense"])
def test_a_step_repeats_bit_for_bit(packed):
    """Three forward + backward runs from identical parameters and inputs, then one HypernetAdamW step each: the same bits in every
    gradient and every parameter.  A guard: at this size atomics often agree by luck — the definitional tests above are the proof."""
    from zett_amd import training
    runs = []
    for _ in range(3):
        model = _model("default", packed, True)
        grads = {n: g.clone() for n, g in _step(model, "default").items()}
        training.HypernetAdamW(model, lr=1e-3).step()
        torch.cuda.synchronize()
        runs.append((grads, {n: p.detach().clone() for n, p in model.named_parameters()}))
    for grads, params in runs[1:]:
        assert grads.keys() == runs[0][0].keys() and len(grads) >= 40
        assert not [n for n in grads if not _same_bits(grads[n], runs[0][0][n])]
        assert not [n for n in params if not _same_bits(params[n], runs[0][1][n])]
    moved = [n for n, p in runs[0][1].items() if n in runs[0][0] and not torch.equal(p.cpu(), torch.from_numpy(_case("default")[1][n]))]
    assert len(moved) >= 30          # (the step did move the parameters)


def _index_sum_within_bound(got, want, idx, src, n_dst, base=0):
    """|got - want| <= train_ops_check.sum_bound(n, sum |addends|) per element, n the destination's count.  Why the any-order bound
    holds between two ORDERS of the same sum: each is within (n - 1) 2^-24 sum |addends| of the exact sum, so they are within
    (n - 1) 2^-23 = (n - 1) U of each other, below (n + 2) U."""
    idx = idx.long().cpu() - base
    inside = (idx >= 0) & (idx < n_dst)
    mag = torch.zeros(n_dst, src.shape[1], dtype=torch.float64).index_add_(0, idx[inside], src.cpu().double().abs()[inside])
    n = torch.bincount(idx[inside], minlength=n_dst).double()[:, None]
    err = (got.cpu().double() - want.cpu().double()).abs()
    assert bool((err <= tc.sum_bound(n, mag)).all()), float((err / tc.sum_bound(n, mag).clamp_min(1e-300)).max())


def test_the_default_mode_is_unchanged(monkeypatch):
    """train_deterministic unset: the three affected sums (per position, per distinct id, per fallback row) still come from the float
    atomics and are within the any-order bound of the deterministic ones, from the same addends; every gradient that does not lie
    behind one of them is the same bits in both modes."""
    for packed, behind in ((True, PACKED_ONLY), (False, DENSE_ONLY)):
        cap = _Capture(monkeypatch, "scatter_add_rows", "index_sum_rows", "gather_bwd")
        g_def = {n: g.clone() for n, g in _step(_model("default", packed, False), "default").items()}
        default_calls = {k: list(v) for k, v in cap.calls.items()}
        for v in cap.calls.values():
            v.clear()
        g_det = _step(_model("default", packed, True), "default")
        monkeypatch.undo()
        assert not default_calls["index_sum_rows"] and all(not k.get("deterministic") for _, k, _ in default_calls["gather_bwd"])
        if packed:
            # default: the position-0 scatter, then the two sums; deterministic: the same scatter and two index sums
            assert len(default_calls["scatter_add_rows"]) == 3 and len(cap.calls["scatter_add_rows"]) == 1 and len(cap.calls["index_sum_rows"]) == 2
            for (a_def, _, out_def), (a_det, _, out_det) in zip(default_calls["scatter_add_rows"][1:], cap.calls["index_sum_rows"]):
                dst, idx, src = a_def
                assert _same_bits(src, a_det[1]) and torch.equal(idx, a_det[0])          # the same addends in both modes
                _index_sum_within_bound(dst, out_det, idx, src, dst.shape[0])
        else:
            assert not default_calls["scatter_add_rows"] and not cap.calls["scatter_add_rows"] and len(cap.calls["index_sum_rows"]) == 1
            (a_def, _, out_def), = default_calls["gather_bwd"]
            (a_det, _, out_det), = cap.calls["gather_bwd"]
            assert _same_bits(a_def[3], a_det[3])
            _index_sum_within_bound(out_def[0], out_det[0], a_def[0], a_def[3], a_def[4], base=a_def[2])
        assert g_def.keys() == g_det.keys()
        free = [n for n in g_def if not n.startswith(behind)]
        assert len(free) >= 30 and not [n for n in free if not _same_bits(g_def[n], g_det[n])]
