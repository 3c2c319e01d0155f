"""What zett_load_weight / zett_finalize promise about the model's weights, whatever the library does inside: which names are
required (dims.weight_shapes, minus the word-embedding table nobody reads), which shapes are accepted, what a name outside the
config's set does, in which states the two calls answer what, and that neither the order of the uploads nor an upload that is
repeated before finalize reaches the outputs.

Shapes: the `tiny` synthetic config (H = 128: no LayerNorm fold) and a two-layer H = 512 config in f16 (the fold operands of the
encoder and of both heads exist, layer 1's fused QKV is folded with layer 0's output LayerNorm): the smallest at which a weight can
be bound to the wrong place.  One forward of 300 rows per digest."""
import ctypes as C
import functools
import hashlib

import pytest
import torch

from zett_amd import _lib, synth
from zett_amd._glue import ptr
from zett_amd.dims import HypernetDims, weight_shapes

pytestmark = pytest.mark.gpu

SEED = 31
ROWS = 300
WORD_TABLE = "model.embeddings.word_embeddings.weight"
TINY = synth.workload("tiny")[0]
H512 = dict(TINY, n_embd=128, hn_hidden_size=512, hn_num_attention_heads=8, hn_intermediate_size=1024, hn_n_layers=2)
CONFIGS = {"tiny_f32": (TINY, "f32"), "tiny_f16": (TINY, "f16"), "h512_f16": (H512, "f16")}


def _handle(cfg, precision="f16"):
    """A fresh handle, nothing loaded."""
    from zett_amd.hypernet import HipEngine
    return HipEngine(HypernetDims.from_config(cfg), 1e-5, torch.device("cuda:0"), precision)


@functools.lru_cache(maxsize=None)
def _weights(key):
    cfg = CONFIGS[key][0] if key in CONFIGS else dict(TINY, **dict(key))
    return {k: torch.from_numpy(v).cuda() for k, v in synth.make_weights(cfg, SEED).items()}


def _load(eng, name, t):
    """zett_load_weight of one tensor -> (status, error text)."""
    t = t.contiguous()
    shape = (C.c_int64 * t.dim())(*t.shape)
    rc = eng.lib.zett_load_weight(eng.handle, name.encode(), ptr(t), _lib.DTYPE_F32, shape, t.dim())
    return rc, eng.lib.zett_last_error().decode()


def _finalize(eng):
    rc = eng.lib.zett_finalize(eng.handle)
    return rc, eng.lib.zett_last_error().decode()


def _load_all(eng, weights, skip=()):
    for name, t in weights.items():
        if name not in skip:
            assert _load(eng, name, t)[0] == 0, name


def _digests(eng, cfg):
    src = torch.from_numpy(synth.make_source_embeddings(cfg, SEED)).cuda()
    ids = torch.from_numpy(synth.make_surface_forms(cfg, ROWS, seed=SEED, n_special=2)).cuda()
    outs = eng.forward(ids, src, 3 if cfg.get("hn_embed_lang_id") else -1)
    torch.cuda.synchronize()
    return [None if t is None else hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest() for t in outs]


@functools.lru_cache(maxsize=None)
def _reference(key):
    """The digests of the config loaded once, in the order of weight_shapes.  Computed once per config and shared."""
    cfg, precision = CONFIGS[key]
    eng = _handle(cfg, precision)
    _load_all(eng, _weights(key))
    assert _finalize(eng)[0] == 0
    got = tuple(_digests(eng, cfg))
    eng.close()
    assert all(d is not None for d in got)
    return got


def test_every_declared_weight_is_required_and_named():
    weights = _weights("tiny_f16")
    required = [n for n in weight_shapes(TINY) if n != WORD_TABLE]
    assert set(required) | {WORD_TABLE} == set(weights)
    for missing in required:
        eng = _handle(TINY)
        _load_all(eng, weights, skip=(missing,))
        rc, text = _finalize(eng)
        eng.close()
        assert rc == _lib.E_STATE, missing
        assert text == f"missing weight: {missing}"


def test_a_wrong_shape_is_refused_with_both_shapes():
    eng = _handle(TINY)
    weights = _weights("tiny_f16")
    name = "model.encoder.layer.0.intermediate.dense.weight"          # [I, H] = [256, 128]
    rc, text = _load(eng, name, weights[name].t().contiguous())
    assert rc == _lib.E_INVALID
    assert text == f"{name}: shape [128,256,] does not match the config's [256,128,]"
    name = "model.embeddings.LayerNorm.bias"
    rc, text = _load(eng, name, torch.zeros(129, device="cuda"))
    assert rc == _lib.E_INVALID
    assert text == f"{name}: shape [129,] does not match the config's [128,]"
    rc, text = _load(eng, "in_scaler.w", torch.zeros(128, device="cuda"))      # the Rescaler's vectors are [1, n]
    assert rc == _lib.E_INVALID
    assert text == "in_scaler.w: shape [128,] does not match the config's [1,128,]"
    eng.close()


def test_a_name_outside_the_declaration_is_accepted_and_ignored():
    one_out = (("separate_out_embeddings", False),)
    cfg = dict(TINY, **dict(one_out))
    assert "out_scaler.w" not in weight_shapes(cfg)
    eng = _handle(cfg)
    assert _load(eng, WORD_TABLE, torch.zeros(7, 3, device="cuda"))[0] == 0          # (any shape: the name is not looked at)
    assert _load(eng, "out_scaler.w", torch.ones(1, 64, device="cuda"))[0] == 0
    assert _load(eng, "no.such.weight", torch.ones(1, device="cuda"))[0] == 0
    _load_all(eng, _weights(one_out))
    assert _finalize(eng)[0] == 0
    assert all(d is not None for d in _digests(eng, cfg)[::2])
    eng.close()


@pytest.mark.parametrize("switch,gone", [
    ("hn_embed_lang_id", {"lang_embeddings.weight"}),
    ("hn_rescale_embeddings", {"in_scaler.w", "in_scaler.b", "scaler.w", "scaler.b", "out_scaler.w", "out_scaler.b"}),
    ("hn_predict_bias", {"bias_projection.weight", "bias_projection.bias"}),
    ("separate_out_embeddings", {"out_scaler.w", "out_scaler.b", "output_projection_out.1.weight", "output_projection_out.1.bias"}
     | {f"output_projection_out.0.{n}" for n in ("dense1.weight", "dense1.bias", "dense2.weight", "dense2.bias", "ln.weight", "ln.bias")}),
])
def test_a_switched_off_part_needs_no_weights(switch, gone):
    key = ((switch, False),)
    cfg = dict(TINY, **dict(key))
    assert set(weight_shapes(TINY)) - set(weight_shapes(cfg)) == gone
    eng = _handle(cfg)
    _load_all(eng, _weights(key))
    rc, text = _finalize(eng)
    assert rc == 0, text
    _digests(eng, cfg)
    eng.close()


def test_states_of_load_and_finalize():
    eng = _handle(TINY)
    weights = _weights("tiny_f16")
    _load_all(eng, weights)
    assert _finalize(eng)[0] == 0
    name = "model.embeddings.LayerNorm.bias"
    rc, text = _load(eng, name, weights[name])
    assert rc == _lib.E_STATE
    assert text == "weights are frozen after zett_finalize"
    assert _finalize(eng)[0] == 0
    eng.close()


@pytest.mark.parametrize("key", sorted(CONFIGS))
def test_the_load_order_does_not_reach_the_outputs(key):
    cfg, precision = CONFIGS[key]
    eng = _handle(cfg, precision)
    weights = _weights(key)
    for name in sorted(weights, reverse=True):
        assert _load(eng, name, weights[name])[0] == 0
    assert _finalize(eng)[0] == 0
    assert tuple(_digests(eng, cfg)) == _reference(key)
    eng.close()


@pytest.mark.parametrize("key", sorted(CONFIGS))
def test_the_last_upload_of_a_weight_wins(key):
    """An operand (part of the fused QKV, and of layer 1's folded one) and a vector (a LayerNorm weight that is folded into the next
    GEMM's operand at H = 512), each uploaded with other values first: a second upload frees and reallocates the tensor."""
    cfg, precision = CONFIGS[key]
    eng = _handle(cfg, precision)
    weights = _weights(key)
    twice = ("model.encoder.layer.1.attention.self.key.weight", "model.encoder.layer.0.output.LayerNorm.weight",
             "model.encoder.layer.1.intermediate.dense.weight", "output_projection.1.bias")
    for name in twice:
        assert _load(eng, name, weights[name] * 0.5 + 0.25)[0] == 0
    _load_all(eng, weights)
    assert _finalize(eng)[0] == 0
    assert tuple(_digests(eng, cfg)) == _reference(key)
    eng.close()
