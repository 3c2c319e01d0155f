"""zett_amd/training.py without a GPU: the freeze / decay rule of the reference's optimizer (train.py:591-622) on the
checkpoint's PyTorch names, and the C ABI surface of the training-step kernels."""
import os
import re

import pytest

from zett_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("zett_op_single_token_mask", "zett_op_embed_dist_rows", "zett_op_embed_dist_finalize", "zett_op_embed_dist_grad", "zett_op_grad_norm",
               "zett_op_adamw")


def _tiny_model():
    from zett_amd.config import ZettHypernetConfig
    from zett_amd.hypernet import ZettHypernet
    cfg, *_ = synth.workload("tiny")
    return ZettHypernet(ZettHypernetConfig(**cfg))


def test_param_labels_follow_the_reference_rule():
    from zett_amd.training import param_labels
    model = _tiny_model()
    names = [n for n, _ in model.named_parameters()]
    labels = param_labels(model)
    assert len(names) == 87 and set(labels) == set(names)
    assert set(labels.values()) <= {"decay", "no_decay", "frozen"}
    # get_labels (train.py:607-622): the parents "scaler" and "in_scaler", nothing else
    assert {n for n, l in labels.items() if l == "frozen"} == {"scaler.w", "scaler.b", "in_scaler.w", "in_scaler.b"}
    # decay_mask_fn (train.py:591-605): no decay on biases and LayerNorm parameters
    for n in names:
        if n.endswith(".bias") or ".LayerNorm." in n or ".ln." in n:
            assert labels[n] == "no_decay", n
    assert sum(l == "no_decay" for l in labels.values()) >= 40
    # the reference's freeze set does not name out_scaler, and its leaves are "w" / "b" (not "bias"): trained and decayed
    assert labels["out_scaler.w"] == "decay" and labels["out_scaler.b"] == "decay"
    # every dense kernel and embedding table decays
    for n in ("model.encoder.layer.0.attention.self.query.weight", "lang_embeddings.weight", "fallback_embeddings.weight", "output_projection.1.weight",
              "bias_projection.weight", "model.embeddings.position_embeddings.weight"):
        assert labels[n] == "decay", n


def test_param_labels_can_be_overridden():
    from zett_amd.training import HypernetAdamW, param_labels
    model = _tiny_model()
    base = param_labels(model)
    by_map = param_labels(model, {"out_scaler.": "frozen", "lang_embeddings.weight": "no_decay"})
    assert by_map["out_scaler.w"] == by_map["out_scaler.b"] == "frozen" and by_map["lang_embeddings.weight"] == "no_decay"
    assert {n: l for n, l in by_map.items() if not n.startswith("out_scaler.") and n != "lang_embeddings.weight"} == \
           {n: l for n, l in base.items() if not n.startswith("out_scaler.") and n != "lang_embeddings.weight"}
    by_fn = param_labels(model, lambda n: "frozen" if n.startswith("model.embeddings.") else None)
    assert by_fn["model.embeddings.LayerNorm.weight"] == "frozen" and by_fn["scaler.w"] == "frozen" and by_fn["bias_projection.bias"] == "no_decay"
    with pytest.raises(ValueError):
        param_labels(model, {"scaler.w": "train"})
    opt = HypernetAdamW(model, lr=1e-3, labels={"out_scaler.": "frozen"})
    assert opt.labels["out_scaler.w"] == "frozen" and opt.betas == (0.9, 0.95) and opt.max_grad_norm == 0.1
    assert opt.last_step_stats() == {"grad_norm": 0.0, "clip_coef": 1.0, "skipped": 0, "step": 0}


def test_a_wrapper_is_unwrapped_and_a_model_without_refresh_weights_is_refused():
    import torch
    from zett_amd.training import HypernetAdamW
    model = _tiny_model()

    class Wrapper(torch.nn.Module):          # what DistributedDataParallel looks like from here: parameters named "module. ..."
        def __init__(self, module):
            super().__init__()
            self.module = module

    opt = HypernetAdamW(Wrapper(model), lr=1e-3)
    assert opt.model is model and "scaler.w" in opt.labels and not any(n.startswith("module.") for n in opt.labels)
    with pytest.raises(TypeError, match="refresh_weights"):
        HypernetAdamW(torch.nn.Linear(4, 4), lr=1e-3)


def test_load_state_dict_validates_what_the_constructor_validates():
    from zett_amd.training import HypernetAdamW
    opt = HypernetAdamW(_tiny_model(), lr=1e-3)
    good = opt.state_dict()
    assert good["step"] == 0 and good["state"] == {}
    opt.load_state_dict(dict(good, step=7, hyper=dict(good["hyper"], lr=0.5, max_grad_norm=None)))
    assert opt.lr == 0.5 and opt.max_grad_norm is None and opt.last_step_stats()["step"] == 7
    opt.load_state_dict({"step": 3, "state": {}})                        # "hyper" and "labels" are optional
    assert opt.lr == 0.5 and opt.last_step_stats()["step"] == 3
    with pytest.raises(KeyError, match="step"):
        opt.load_state_dict({"state": {}})
    for bad in (dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0), dict(betas=(0.9, 1.0)), dict(eps=-1e-8)):
        with pytest.raises(ValueError):
            opt.load_state_dict(dict(good, hyper=dict(good["hyper"], **bad)))
    with pytest.raises(KeyError, match="nonexistent"):
        opt.load_state_dict(dict(good, state={"nonexistent.weight": {}}))
    with pytest.raises(ValueError):
        opt.load_state_dict(dict(good, labels=dict(good["labels"], **{"scaler.w": "train"})))
    assert opt.lr == 0.5 and opt.last_step_stats()["step"] == 3         # a refused state dict changes nothing


def test_adafactor_load_state_dict_validates_what_the_constructor_validates():
    """the cases of the test above that apply to HypernetAdafactor (it has no betas or eps), and its own: the statistics a shape keeps"""
    import torch
    from zett_amd.training import HypernetAdafactor, adafactor_state_shapes
    model = _tiny_model()
    opt = HypernetAdafactor(model, lr=1e-3)
    assert not hasattr(opt, "betas") and not hasattr(opt, "eps")
    good = opt.state_dict()
    assert good["step"] == 0 and good["state"] == {} and good["hyper"] == {"lr": 1e-3, "weight_decay": 0.01, "max_grad_norm": 0.1}
    big = next(n for n, p in model.named_parameters() if p.dim() == 2 and min(p.shape) >= 128)
    shapes = adafactor_state_shapes(dict(model.named_parameters())[big].shape)
    assert set(shapes) == {"v_row", "v_col"}
    state = {big: {k: torch.full(s, 0.25) for k, s in shapes.items()}, "bias_projection.bias": {"v": torch.ones(model.bias_projection.bias.shape)}}
    opt.load_state_dict(dict(good, step=7, state=state, hyper=dict(good["hyper"], lr=0.5, max_grad_norm=None)))
    assert opt.lr == 0.5 and opt.max_grad_norm is None and opt.last_step_stats()["step"] == 7 and set(opt.state) == set(state)
    assert float(opt.state[big]["v_row"][0]) == 0.25 and opt.state[big]["v_row"] is not state[big]["v_row"]
    opt.load_state_dict({"step": 3, "state": state})                    # "hyper" and "labels" are optional
    assert opt.lr == 0.5 and opt.last_step_stats()["step"] == 3
    with pytest.raises(KeyError, match="step"):
        opt.load_state_dict({"state": {}})
    with pytest.raises(ValueError, match="negative"):
        opt.load_state_dict(dict(good, step=-1))
    for bad in (dict(max_grad_norm=0.0), dict(max_grad_norm=-1.0)):
        with pytest.raises(ValueError):
            opt.load_state_dict(dict(good, hyper=dict(good["hyper"], **bad)))
    with pytest.raises(KeyError, match="nonexistent"):
        opt.load_state_dict(dict(good, state={"nonexistent.weight": {}}))
    wrong_shape = {big: dict(state[big], v_row=torch.zeros(shapes["v_row"][0] + 1))}
    full_v = {big: {"v": torch.zeros(dict(model.named_parameters())[big].shape)}}          # a factored shape keeps no full-size v
    extra_key = {big: dict(state[big], v=torch.zeros(1))}
    for bad in (wrong_shape, full_v, extra_key, {big: {"v_row": state[big]["v_row"]}}):
        with pytest.raises(ValueError, match=big):
            opt.load_state_dict(dict(good, state=bad))
    with pytest.raises(ValueError):
        opt.load_state_dict(dict(good, labels=dict(good["labels"], **{"scaler.w": "train"})))
    assert opt.lr == 0.5 and opt.last_step_stats()["step"] == 3 and set(opt.state) == set(state)          # a refused state dict changes nothing
    assert float(opt.state[big]["v_row"][0]) == 0.25 and opt.labels == good["labels"]


def test_adamw_load_state_dict_takes_exactly_the_two_moments():
    """what the shared load_state_dict changed for HypernetAdamW: an entry's keys must be exactly exp_avg and exp_avg_sq of the
    parameter's shape.  A missing moment is a ValueError naming the parameter (it was a bare KeyError), an extra key is refused (it
    was dropped without a word); betas / eps and max_grad_norm are validated one after the other, each with its own message."""
    import torch
    from zett_amd.training import HypernetAdamW
    model = _tiny_model()
    opt = HypernetAdamW(model, lr=1e-3)
    good = opt.state_dict()
    name, p = next(iter(model.named_parameters()))
    moments = {"exp_avg": torch.full(p.shape, 0.5), "exp_avg_sq": torch.full(p.shape, 0.25)}
    opt.load_state_dict(dict(good, step=2, state={name: moments}))
    assert set(opt.state[name]) == {"exp_avg", "exp_avg_sq"} and float(opt.state[name]["exp_avg"].flatten()[0]) == 0.5
    assert opt.state[name]["exp_avg"] is not moments["exp_avg"]
    for bad in ({"exp_avg": moments["exp_avg"]}, dict(moments, step=torch.zeros(())), dict(moments, exp_avg_sq=torch.zeros(p.numel() + 1))):
        with pytest.raises(ValueError, match=name):
            opt.load_state_dict(dict(good, step=9, state={name: bad}))
    with pytest.raises(ValueError, match="betas"):
        opt.load_state_dict(dict(good, step=9, hyper=dict(good["hyper"], betas=(1.0, 0.5))))
    with pytest.raises(ValueError, match="max_grad_norm"):
        opt.load_state_dict(dict(good, step=9, hyper=dict(good["hyper"], max_grad_norm=0.0)))
    assert opt.last_step_stats()["step"] == 2 and float(opt.state[name]["exp_avg_sq"].flatten()[0]) == 0.25          # refused: nothing changed


@pytest.mark.parametrize("which", ["HypernetAdamW", "HypernetAdafactor"])
def test_a_parameter_without_a_label_is_refused(which):
    """a parameter added to the model after the optimizer was built has no label: ValueError before anything is launched or allocated,
    from both classes (AdamW used to decay it silently)"""
    import torch
    from zett_amd import training
    model = _tiny_model()
    opt = getattr(training, which)(model, lr=1e-3)
    model.late = torch.nn.Parameter(torch.zeros(4))
    assert "late" not in opt.labels and "late" in dict(model.named_parameters())
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    with pytest.raises(ValueError, match="late has no label"):
        opt.step()
    assert opt.state == {} and opt.record is None and opt.last_step_stats()["step"] == 0


def test_header_and_binding_agree_on_the_training_step_symbols():
    from zett_amd import _lib
    header = open(os.path.join(REPO, "include", "zett_hip.h")).read()
    declared = set(re.findall(r"\b(zett_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.ABI_SYMBOLS, name
    assert int(re.search(r"#define ZETT_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 8
    assert int(re.search(r"#define ZETT_MT_CHUNK (\d+)", header).group(1)) == _lib.MT_CHUNK
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert getattr(lib, name).restype is not None
    assert lib.zett_abi_version() == 8


def test_the_training_step_kernels_stay_outside_the_measured_forward():
    """csrc/train_step.hip is training-only: profiles/pmc_traffic.json stays tied to the forward's sources."""
    from zett_amd import build
    assert "train_step.hip" in build.SOURCES and "train_step.hip" in build.TRAINING_ONLY
    assert "train_dist.hip" in build.SOURCES and "train_dist.hip" in build.TRAINING_ONLY
    assert "train_optim.hip.h" in build.HEADERS and "train_optim.hip.h" in build.TRAINING_ONLY
