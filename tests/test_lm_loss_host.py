"""zett_amd.training.lm_head_loss without a GPU: the C ABI surface of csrc/train_loss.hip, the checks that run before any launch, and
the label / weight arrays of the reference's loss_fn (train.py:874-912)."""
import os
import re

import pytest
import torch

from zett_amd.training import lm_default_chunk_rows, lm_head_loss, lm_label_arrays

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("zett_op_ce_addend", "zett_op_ce_rows", "zett_op_ce_finalize", "zett_op_ce_colsum", "zett_op_ce_scale", "zett_op_ce_cast")


def test_header_binding_and_library_agree_on_the_loss_symbols():
    from zett_amd import _lib
    header = open(os.path.join(REPO, "include", "zett_hip.h")).read()
    declared = set(re.findall(r"\b(zett_[a-z0-9_]+)\s*\(", header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.ABI_SYMBOLS, name
    assert int(re.search(r"#define ZETT_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 8          # additive: the version stays
    assert int(re.search(r"#define ZETT_CE_ONCE_MAX_COLS (\d+)", header).group(1)) == _lib.CE_ONCE_MAX_COLS
    paths = re.search(r"enum zett_ce_path \{ ZETT_CE_AUTO = (\d+), ZETT_CE_ONCE = (\d+), ZETT_CE_TWICE = (\d+) \}", header)
    assert tuple(int(x) for x in paths.groups()) == (_lib.CE_AUTO, _lib.CE_ONCE, _lib.CE_TWICE)
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        fn = getattr(lib, name)
        assert fn.restype is not None and fn.argtypes, name
        proto = re.search(r"int %s\(([^;]*)\);" % name, header).group(1)
        assert len(fn.argtypes) == proto.count(",") + 1, name                                    # as many arguments as the header declares
    assert lib.zett_abi_version() == 8


def test_the_entry_points_validate_before_any_launch():
    """Null pointers and impossible shapes are refused with ZETT_E_INVALID: no kernel is launched (there is no GPU here)."""
    import ctypes as C
    from zett_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    null = C.c_void_p(0)
    assert lib.zett_op_ce_rows(null, 8, p, null, 1, 8, 8, null, 0, 8, p, p, p, 0, null) == _lib.E_INVALID
    assert lib.zett_op_ce_rows(p, 8, p, null, 1, 0, 8, null, 0, 8, p, p, p, 0, null) == _lib.E_INVALID           # no columns
    assert lib.zett_op_ce_rows(p, 8, p, null, 1, 7, 6, null, 0, 8, p, p, p, 0, null) == _lib.E_INVALID           # v_padded < v
    assert lib.zett_op_ce_rows(p, 8, p, null, 1, 6, 6, null, 0, 8, p, p, p, 0, null) == _lib.E_INVALID           # v_padded % 4
    assert lib.zett_op_ce_rows(p, 4, p, null, 1, 8, 8, null, 0, 8, p, p, p, 0, null) == _lib.E_INVALID           # ld_z < v_padded
    assert lib.zett_op_ce_rows(p, 8, p, null, 1, 8, 8, p, 7, 8, p, p, p, 0, null) == _lib.E_INVALID              # unknown dtype of G
    assert lib.zett_op_ce_rows(p, 8, p, null, 1, 8, 8, p, _lib.DTYPE_BF16, 8, p, p, p, 0, null) == _lib.E_INVALID    # a 16-bit G over the logits
    assert lib.zett_op_ce_rows(p, 8, p, null, 1, 8, 8, null, 0, 8, p, p, p, 3, null) == _lib.E_INVALID           # unknown path
    big = _lib.CE_ONCE_MAX_COLS + 4
    assert lib.zett_op_ce_rows(p, big, p, null, 1, big, big, null, 0, big, p, p, p, _lib.CE_ONCE, null) == _lib.E_INVALID
    assert b"read-once" in lib.zett_last_error()
    assert lib.zett_op_ce_finalize(p, null, p, p, 0, p, null) == _lib.E_INVALID
    assert lib.zett_op_ce_addend(null, null, null, 9, 8, p, null) == _lib.E_INVALID
    assert lib.zett_op_ce_colsum(p, 5, 8, 1, 8, p, 0, null) == _lib.E_INVALID
    assert lib.zett_op_ce_scale(p, 4, p, p, p, 9, null) == _lib.E_INVALID
    assert lib.zett_op_ce_cast(p, 0, 4, p, 2, 4, 1, 8, 8, null) == _lib.E_INVALID                                  # ld < cols


def test_shape_and_dtype_errors_raise_before_any_launch():
    hidden, w, labels = torch.zeros(2, 5, 16), torch.zeros(30, 16), torch.zeros(2, 5, dtype=torch.long)
    bad = [
        dict(hidden=torch.zeros(16)),                                                   # no leading dimension
        dict(hidden=hidden.double()),
        dict(pred_out=torch.zeros(30, 8)),                                              # E differs
        dict(pred_out=w.half()),
        dict(pred_out=torch.zeros(0, 16)),
        dict(labels=torch.zeros(10, dtype=torch.long)),                                 # not hidden's leading shape
        dict(labels=torch.zeros(2, 5)),                                                 # not integers
        dict(bias=torch.zeros(29)),
        dict(priors=torch.zeros(30, 1)),
        dict(vocab_mask=torch.zeros(30)),                                               # not bool
        dict(precision="fp8"),
        dict(chunk_rows=0),
        dict(rows_path="thrice"),
        dict(mode="causal"),
        dict(mode="clm", weight=torch.ones(2, 5)),                                      # clm derives its weights
        dict(attention_mask=torch.ones(2, 5)),                                          # an attention mask needs a mode
        dict(mode="mlm", attention_mask=torch.ones(2, 4)),
        dict(weight=torch.ones(10)),
    ]
    for change in bad:
        args = dict(hidden=hidden, pred_out=w, labels=labels, precision="f32")
        args.update(change)
        h, p, l = args.pop("hidden"), args.pop("pred_out"), args.pop("labels")
        with pytest.raises(ValueError):
            lm_head_loss(h, p, l, args.pop("attention_mask", None), **args)
    with pytest.raises(ValueError, match="no CPU path"):                                # well-formed, but not on a GPU: still no launch
        lm_head_loss(hidden, w, labels, precision="f32")


def test_clm_arrays_equal_the_reference_slicing():
    """train.py:883-885: logits[..., :-1, :], labels[..., 1:], attention_mask[..., :-1]"""
    g = torch.Generator().manual_seed(1234)
    b, s, v = 3, 7, 11
    labels = torch.randint(0, v, (b, s), generator=g)
    attention = torch.tensor([[1, 1, 1, 1, 1, 1, 1], [1, 1, 1, 1, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0]])
    lab, w = lm_label_arrays(labels, attention, "clm")
    assert lab.dtype == torch.int32 and w.dtype == torch.float32 and lab.shape == w.shape == (b * s,)
    lab, w = lab.view(b, s), w.view(b, s)
    assert torch.equal(lab[:, :-1].long(), labels[..., 1:]) and torch.equal(w[:, :-1], attention[..., :-1].float())
    assert not w[:, -1].any()                                                           # the last position scores nothing
    # the loss over these arrays is the loss over the reference's shifted views
    logits = torch.randn(b, s, v, generator=g, dtype=torch.float64)
    ce = torch.nn.functional.cross_entropy
    want = (ce(logits[..., :-1, :].reshape(-1, v), labels[..., 1:].reshape(-1), reduction="none").view(b, s - 1) * attention[..., :-1]).sum() / attention[..., :-1].sum()
    rows = ce(logits.view(-1, v), lab.view(-1).long().clamp(min=0), reduction="none") * w.view(-1)
    assert float(rows.sum() / w.sum()) == pytest.approx(float(want), rel=1e-12)
    lab1, w1 = lm_label_arrays(labels, None, "clm")                                     # no attention mask: every position but the last
    assert torch.equal(lab1, lab.reshape(-1)) and torch.equal(w1.view(b, s)[:, :-1], torch.ones(b, s - 1)) and not w1.view(b, s)[:, -1].any()


def test_mlm_and_plain_arrays():
    labels = torch.tensor([[4, -100, 2, 9], [-100, -100, 1, 3]])
    attention = torch.tensor([[1, 1, 1, 0], [1, 1, 1, 1]])
    lab, w = lm_label_arrays(labels, attention, "mlm")
    assert torch.equal(lab.view(2, 4).long(), labels)
    assert torch.equal(w.view(2, 4), ((labels != -100) & (attention == 1)).float())     # train.py:902
    lab, w = lm_label_arrays(labels, None, None)
    assert w is None and torch.equal(lab.long(), labels.reshape(-1))
    lab, w = lm_label_arrays(labels, None, None, torch.full((2, 4), 0.25, dtype=torch.float64))
    assert w.dtype == torch.float32 and torch.equal(w, torch.full((8,), 0.25))


def test_default_chunk_keeps_the_logits_at_one_gibibyte():
    assert lm_default_chunk_rows(32768, "bf16") == 8192 and lm_default_chunk_rows(262144, "bf16") == 1024
    for v in (203, 32001, 50370, 262144):
        for precision, step in (("f32", 32), ("bf16", 64)):
            rows = lm_default_chunk_rows(v, precision)
            vp = -(-v // step) * step
            assert rows % 64 == 0 and rows * vp * 4 <= 1 << 30 < (rows + 64) * vp * 4


def test_the_loss_kernels_stay_outside_the_measured_forward_and_use_no_scratch():
    from zett_amd import build
    assert "train_loss.hip" in build.SOURCES and "train_loss.hip" in build.TRAINING_ONLY
    remarks = build.fresh_remarks("train_loss.hip")
    if remarks is None:                                  # (a library built elsewhere: the compiler's remarks did not travel with it)
        return
    kernels = re.findall(r"Function Name: (\S+)", remarks)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", remarks)]
    assert len(kernels) == len(scratch) >= 30 and any("ce_rows_kernel" in k for k in kernels)
    assert not any(scratch), [k for k, s in zip(kernels, scratch) if s]
