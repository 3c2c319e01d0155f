"""Lever 6 without a GPU (tests/id_qkv_check.py): the identity behind it on the oracle's tiny case without a language position, the
kernel's fp32 emulation inside its own bounds on the case table of tests/test_id_qkv_direct_gpu.py, and the ABI declaration."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import hypernet_ref
from tests import id_qkv_check as ic
from tests import test_id_qkv_direct_gpu as direct
from tests import util
from zett_amd import synth


@pytest.mark.parametrize("kind", ("f16", "bf16"))
def test_identity_meets_the_tolerance_on_the_tiny_case(kind):
    """layer 0's q / k / v from the id-level product, rounded where the device rounds, against the oracle's forward: the tolerance of
    the precision (tests/util.py), not a wider one"""
    cfg, rows, _, hist = synth.workload("tiny")
    cfg = dict(cfg, hn_embed_lang_id=False)
    assert int(cfg.get("hn_n_layers", 3)) >= 2
    w = synth.make_weights(cfg, seed=11)
    src = synth.make_source_embeddings(cfg, seed=11)
    ids = synth.make_surface_forms(cfg, rows, seed=11, hist=hist, n_special=2)
    want = hypernet_ref.forward(w, cfg, ids, src)
    got = ic.forward_id_qkv(w, cfg, ids, src, kind)
    keep = ~util.all_pad_rows(cfg, ids)
    for g, r, what in zip(got, want, ("pred_in", "pred_out", "bias")):
        util.CLOSE[kind](g[keep], r[keep], f"id_qkv identity {kind} {what}")


@pytest.mark.parametrize("case", direct.CASES, ids=direct.case_id)
def test_emulation_is_inside_the_bounds(case):
    """the fp32 emulation of the kernel against float64 with the bounds the GPU test applies; the f16 overflow row overflows"""
    v = direct.make_values(case)
    lo = direct.LO[case["prec"]]
    x = ic.pair_qkv_ref(v["u"], v["slot"], v["pos"], v["stats"], v["c_pos"], v["c_w"], v["b_q"])
    got = ic.pair_qkv_emulate(v["u"], v["slot"], v["pos"], v["stats"], v["c_pos"], v["c_w"], v["b_q"], lo)
    over = ic.check_pair_qkv(f"emulation {case}", got, x, lo)
    assert over == (case["prec"] == "f16" and case["n"] >= 7)


def test_case_table():
    """both column-block layouts, every row count, positions on both sides of the kernel's LDS cache, slots out of order"""
    assert {c["h"] for c in direct.CASES} == {128, 704} and {c["n"] for c in direct.CASES} == {1, 7, 300}
    assert {c["prec"] for c in direct.CASES} == {"f16", "bf16"} and {c["buffer"] for c in direct.CASES} == {False, True}
    v = direct.make_values(dict(h=704, n=300, prec="f16", buffer=True))
    assert set(v["pos"].tolist()) == set(range(9)) and set(v["slot"].tolist()) == set(range(direct.SLOTS))
    assert (np.diff(v["slot"].numpy()) < 0).any()


def test_abi_declares_the_entry_points():
    from zett_amd import _lib
    header = open(os.path.join(os.path.dirname(util.HERE), "include", "zett_hip.h")).read()
    for name in ("zett_op_fwd_pair_qkv", "zett_id_qkv"):
        assert re.search(r"\bint " + name + r"\(", header) and name in _lib.ABI_SYMBOLS
    assert torch.float16 in direct.LO.values()
