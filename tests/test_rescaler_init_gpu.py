"""ZettHypernet.init_rescaler and training.init_hypernet_state on the smallest synthetic hypernetworks — two output heads, one tied
matrix, hn_single_head — with fp32 and bf16 source embeddings that carry a per-column offset (so that the means matter), in f32
arithmetic (the forward then adds no 16-bit rounding to the comparison).

The three (w, b) pairs are held, element by element, to the float64 restatement of Hypernet.init_rescaler
(tests/rescaler_check.py init_rescaler_ref).  For scaler / out_scaler the restatement is fed the ENGINE'S OWN predictions under the
fitted in_scaler and identity scalers — the bits the fit saw, the rule tests/rowops_check.py uses for two-stage checks; in_scaler is
compared against the float64 moments of the source matrix itself.  One fit per configuration is computed once and shared."""
import numpy as np
import pytest
import torch

from tests import rescaler_check as rk

DEV = "cuda:0"
gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
ANCHORS = 96
CONFIGS = {
    "two_heads": dict(),                                                  # the tiny workload: separate output embeddings, a language id
    "tied": dict(separate_out_embeddings=False, hn_embed_lang_id=False),
    "single_head": dict(hn_single_head=True),
}
CASES = [(name, kind) for name in CONFIGS for kind in ("f32", "bf16")]
SCALERS = ("in_scaler", "scaler", "out_scaler")


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = rk.record_path()
    if path:
        rk.write_record(path)


def _model(name):
    from zett_amd import synth
    from zett_amd.config import ZettHypernetConfig
    from zett_amd.hypernet import ZettHypernet
    cfg, _rows, _dtype, hist = synth.workload("tiny")
    cfg.update(CONFIGS[name])
    model = ZettHypernet(ZettHypernetConfig(**cfg))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synth.make_weights(cfg, seed=21).items()})
    model.precision = "f32"
    return cfg, hist, model.to(DEV)


def _scalers(model):
    p = dict(model.named_parameters())
    return {n: (p[n + ".w"].detach().cpu().clone(), p[n + ".b"].detach().cpu().clone()) for n in SCALERS if n + ".w" in p}


_FITS = {}


def fitted(name, kind):
    """One init_rescaler per (configuration, source type): the model, its starting parameters, the inputs, the fitted pairs and the
    engine's identity-scaler predictions under the fitted in_scaler.  Computed once, shared, never modified."""
    key = (name, kind)
    if key in _FITS:
        return _FITS[key]
    from zett_amd import synth
    cfg, hist, model = _model(name)
    e = model.dims.n_embd
    src = synth.make_source_embeddings(cfg, seed=21).astype(np.float64)
    offset = np.random.Generator(np.random.Philox(key=77)).uniform(-0.05, 0.05, size=src.shape[1])
    src = torch.from_numpy(src + offset[None, :]).to(rk.DT[kind]).to(DEV)
    ids = torch.from_numpy(synth.make_surface_forms(cfg, ANCHORS, seed=21, hist=hist)).to(DEV)
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    was_training = model.training
    model.init_rescaler(ids, src)
    assert model.training == was_training and model.precision == "f32"
    got = _scalers(model)
    after = [None if t is None else t.cpu() for t in model(ids, source_embeddings=src, lang_index=0)[:2]]
    # the predictions the fit saw: the fitted in_scaler, identity scalers
    params = dict(model.named_parameters())
    with torch.no_grad():
        for n in ("scaler", "out_scaler"):
            if n + ".w" in params:
                params[n + ".w"].fill_(1.0)
                params[n + ".b"].zero_()
    pred = [None if t is None else t.cpu() for t in model(ids, source_embeddings=src, lang_index=0)[:2]]
    model.load_state_dict(start)
    _FITS[key] = dict(cfg=cfg, model=model, e=e, src=src, ids=ids, start=start, got=got, pred=pred, after=after)
    return _FITS[key]


def _targets(f):
    s = f["src"].cpu()
    return s[:, :f["e"]], (s[:, f["e"]:] if f["model"].dims.separate_out else None)


@gpu
@pytest.mark.parametrize("name,kind", CASES)
def test_fitted_pairs_match_the_float64_restatement(name, kind):
    from zett_amd.hypernet import EMBED_INIT_RANGE
    f = fitted(name, kind)
    t_in, t_out = _targets(f)
    ref = rk.init_rescaler_ref(f["src"].cpu(), f["pred"][0], f["pred"][1], t_in, t_out, EMBED_INIT_RANGE)
    bnd = rk.init_rescaler_bound(f["src"].cpu(), f["pred"][0], f["pred"][1], t_in, t_out, EMBED_INIT_RANGE)
    assert set(ref) == set(f["got"]) == ({"in_scaler", "scaler", "out_scaler"} if t_out is not None else {"in_scaler", "scaler"})
    for scaler, (w, b) in f["got"].items():
        assert w.shape == b.shape == ref[scaler][0].shape and w.dtype == b.dtype == F32
        rk.check(w, ref[scaler][0], bnd[scaler][0][None], f"{name} {kind} {scaler}.w", key=("init_rescaler", f"{scaler} w"))
        rk.check(b, ref[scaler][1], bnd[scaler][1][None], f"{name} {kind} {scaler}.b", key=("init_rescaler", f"{scaler} b"))
        assert bool((b != 1.0).all()), f"{scaler}.b still holds the torch port's placeholder 1"
    # what the fit is for: the rescaled source has std EMBED_INIT_RANGE and mean 0, the rescaled predictions the targets' moments
    w, b = (t.double() for t in f["got"]["in_scaler"])
    y = f["src"].cpu().double() * w + b
    assert float(y.mean(0).abs().max()) < 1e-6 and float((y.std(0, unbiased=False) - EMBED_INIT_RANGE).abs().max()) < 1e-6


@gpu
@pytest.mark.parametrize("name,kind", CASES)
def test_forward_after_the_call_applies_the_fitted_pairs(name, kind):
    f = fitted(name, kind)
    for which, scaler in ((0, "scaler"), (1, "out_scaler")):
        if f["pred"][which] is None:
            assert f["after"][which] is None
            continue
        w, b = (t.double() for t in f["got"][scaler])
        p = f["pred"][which].double()
        rk.check(f["after"][which], w * p + b, rk.fma_bound(w * p, b.expand_as(p)), f"{name} {kind} forward after the fit, {scaler}",
                 key=("init_rescaler", f"forward {scaler}"))


@gpu
@pytest.mark.parametrize("name,kind", CASES)
def test_second_call_and_explicit_targets_give_the_same_bits(name, kind):
    f = fitted(name, kind)
    model, src, e = f["model"], f["src"], f["e"]

    def same(what):
        got = _scalers(model)
        for scaler, (w, b) in f["got"].items():
            assert torch.equal(got[scaler][0].view(torch.int32), w.view(torch.int32)), (what, scaler, "w")
            assert torch.equal(got[scaler][1].view(torch.int32), b.view(torch.int32)), (what, scaler, "b")
        model.load_state_dict(f["start"])

    model.load_state_dict(f["start"])
    model.init_rescaler(f["ids"], src)
    same("a second call from the same starting parameters")
    # the default targets are column ranges of the source matrix's state; explicit slices are passes of their own over the same values
    model.init_rescaler(f["ids"], src, src[:, :e], src[:, e:] if model.dims.separate_out else None)
    same("explicit target slices")
    model.train()
    model.init_rescaler(f["ids"], src)
    assert model.training                                             # the mode is restored
    model.eval()
    same("called in train mode")


@gpu
def test_init_hypernet_state_overlays_and_reinitialises():
    from zett_amd import training
    f = fitted("two_heads", "f32")
    model, src, ids = f["model"], f["src"], f["ids"]
    pre = {"scaler.w": torch.full((1, f["e"]), 3.0), "model.embeddings.LayerNorm.bias": torch.full_like(f["start"]["model.embeddings.LayerNorm.bias"], 0.25).cpu()}
    model.load_state_dict(f["start"])
    assert training.init_hypernet_state(model, src, ids, pretrained_state=pre) == []
    p = dict(model.named_parameters())
    assert bool((p["scaler.w"] == 3.0).all())                                      # the dict's value wins over the fitted one
    assert torch.equal(p["scaler.b"].detach().cpu().view(torch.int32), f["got"]["scaler"][1].view(torch.int32))
    assert bool((p["model.embeddings.LayerNorm.bias"] == 0.25).all())
    model.load_state_dict(f["start"])
    assert training.init_hypernet_state(model, src, ids, pretrained_state=pre, reinit_projectors=True) == ["scaler.w"]
    p = dict(model.named_parameters())
    assert torch.equal(p["scaler.w"].detach().cpu().view(torch.int32), f["got"]["scaler"][0].view(torch.int32))      # the fitted one stays
    assert bool((p["model.embeddings.LayerNorm.bias"] == 0.25).all())
    # the engines noticed the writes: a forward now runs on the overlaid parameters
    a = model(ids, source_embeddings=src, lang_index=0)[0].cpu()
    model.load_state_dict(f["start"])
    assert not torch.equal(a, model(ids, source_embeddings=src, lang_index=0)[0].cpu())
    model.load_state_dict(f["start"])
