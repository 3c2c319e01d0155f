"""The checker of the Adafactor step (tests/adafactor_check.py) passes a right kernel, its case tables reach every branch of
zett_amd/csrc/train_adafactor.hip they claim to, the definition (tests/adafactor_ref.py) is pinned to an independent implementation
where the two coincide, and the host side of zett_amd.training.HypernetAdafactor refuses what it must (no GPU).

A right kernel is the fp32 emulation: the definition's formulas in fp32, every sum in the order the kernels document.  With all
constants at 1 it stays at or below 0.25 of every bound that is a long sum (the first step's v_row / v_col from zero statistics, which
ARE the row and column means of q) and at or below 0.5 of every bound that is a handful of roundings (p, v, and the statistics once
beta v is in them): U is the round-off twice over, so operations that all round the same way reach exactly half of such a bound.
"""
import ctypes as C
import os
import re

import pytest
import torch

from tests import adafactor_check as ac
from tests import adafactor_ref as ref
from tests import loss_step_check as lc

F32, F64 = torch.float32, torch.float64
U = ac.U
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT_SUM, LIMIT_FEW = 0.25, 0.5


def _ratio(got, want, bnd):
    err = (got.double() - want.double()).abs()
    assert bool(torch.isfinite(err).all())
    r = torch.where(err == 0, torch.zeros_like(err), err / bnd.double().clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


# ---- the emulation against the bounds ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(ac.single_cases())))
def test_emulation_stays_inside_the_bounds(i):
    e = ac.single_cases()[i]
    p, g, st = ac.values(e, i, 0), ac.values(e, i, 1), ac.values(e, i, 2)
    for t, coef in ((0, 1.0), (5, 0.3125)):
        beta, omb = ref.decay(t)
        st0 = {k: torch.zeros_like(v) for k, v in st.items()} if t == 0 else st
        a = ac.tensor_step(p, g, st0, e["flags"], coef, beta, omb, ac.HYPER["lr"], ac.HYPER["wd"], e["off"], F64)
        b = ac.tensor_step(p, g, st0, e["flags"], coef, beta, omb, ac.HYPER["lr"], ac.HYPER["wd"], e["off"], F32)
        # the float64 run IS the definition
        pn, sn, info = ref.update_tensor(p, g, st0, float(torch.tensor(coef, dtype=F32)), beta, omb, ac.HYPER["lr"], lc.f32(ac.HYPER["wd"]) if e["flags"] & ac.DECAY else 0.0)
        assert torch.allclose(pn, a["p"], rtol=1e-10, atol=0.0) and all(torch.allclose(sn[k], a["state"][k], rtol=1e-12, atol=0.0) for k in sn)
        assert _ratio(b["p"], a["p"], a["b_p"]) * ac.C_AF_P <= LIMIT_FEW
        for k in a["state"]:
            long_sum = t == 0 and k != "v"
            assert _ratio(b["state"][k], a["state"][k], a["b_state"][k]) * ac.C_AF_V <= (LIMIT_SUM if long_sum else LIMIT_FEW), (k, t)
        if t == 0 and "v" in a["state"]:          # nothing is added at t = 0: v = q to the bit
            assert torch.equal(b["state"]["v"], g * g + torch.tensor(1e-30, dtype=F32))


def test_norm_partials_and_record():
    entries = ac.mixed_list()
    grads = [ac.values(e, i, 1) for i, e in enumerate(entries)]
    parts = ac.norm_partials(grads, entries)
    assert parts.numel() == sum(ac.items_of(e["shape"], e["flags"]) for e in entries)
    for t0, max_norm in ((0, 1e6), (3, 2.0)):
        want = ac.record_ref(grads, max_norm, t0)
        norm = torch.sqrt(parts.double().sum()).to(F32)
        assert _ratio(norm, want["norm"][0], want["norm"][1]) * ac.C_AF_SCALAR <= LIMIT_SUM
        assert want["skip"] == 0 and want["t"] == t0 + 1
        beta, omb = ref.decay(t0)
        assert abs(beta - float(want["beta"][0])) <= float(want["beta"][1]) and abs(omb - float(want["omb"][0])) <= float(want["omb"][1])
    assert ref.decay(0) == (0.0, 1.0)
    bad = [g.clone() for g in grads]
    bad[3].view(-1)[0] = float("inf")
    assert ac.record_ref(bad, 1.0, 4)["skip"] == 1 and ac.record_ref(bad, 1.0, 4)["t"] == 4


# ---- the case tables reach every branch ---------------------------------------------------------------------------------------------
def test_case_tables_reach_every_branch():
    cases = ac.single_cases()
    shapes = [c["shape"] for c in cases]
    for s in ((127, 300), (128, 300), (300, 128), (128, 128), (129, 257), (1, 4096), (26, 256), (1,), (63,), (64,), (65,), (4097,), (ac.MT_CHUNK + 5,)):
        assert s in shapes, s
    fact = [c for c in cases if ac.is_factored(c["shape"], c["flags"])]
    flat = [c for c in cases if not ac.is_factored(c["shape"], c["flags"])]
    # the factoring rule: the threshold on either dimension, from both sides, and which statistic is normalised (rows <= cols, rows > cols, square)
    assert not ac.is_factored((127, 300), 0) and not ac.is_factored((300, 127), 0) and ac.is_factored((128, 300), 0) and ac.is_factored((300, 128), 0)
    assert not ac.is_factored((128, 300), ac.FROZEN) and not ac.is_factored((4096,), 0)
    assert any(c["shape"][0] < c["shape"][1] for c in fact) and any(c["shape"][0] > c["shape"][1] for c in fact) and any(c["shape"][0] == c["shape"][1] for c in fact)
    assert ref.factored_dims((128, 128)) == (0, 1) and ref.factored_dims((300, 128)) == (1, 0) and ref.factored_dims((128, 300)) == (0, 1) and ref.factored_dims((127, 300)) is None
    # +-1 around a tile height (in tiles: 2 and 3 rows of tiles), a tile width, the statistics segment and the vector width
    rows, cols = {c["shape"][0] for c in fact}, {c["shape"][1] for c in fact}
    for k in (2 * ac.TILE_ROWS, 3 * ac.TILE_ROWS):
        assert {k - 1, k, k + 1} & rows == {k - 1, k, k + 1} or k == 2 * ac.TILE_ROWS and {k, k + 1} <= rows, (k, sorted(rows))       # (127 rows is below the factoring threshold: not a tile case)
    assert {ac.TILE_COLS - 1, ac.TILE_COLS, ac.TILE_COLS + 1} <= cols
    for side in (rows, cols):
        assert {ac.SEG - 1, ac.SEG, ac.SEG + 1} <= side, sorted(side)
    assert {259, 260, 261} <= cols and any(c % ac.VEC == 0 for c in cols) and any(c % ac.VEC for c in cols)
    assert any(ac.items_of(c["shape"], 0) > 1 for c in fact) and any(ac.items_of(c["shape"], 0) > 1 for c in flat)
    assert ac.is_factored(ac.STRIDE_SHAPE, 0) and ac.items_of(ac.STRIDE_SHAPE, 0) == ac.MT_GRID + 1          # one item past the grid's cap
    # the flat path: below, at and past a vector, a vector pass of the workgroup (1024), a chunk
    n = {c["shape"][0] for c in flat if len(c["shape"]) == 1}
    assert {3, 4, 5, 1023, 1024, 1025, ac.MT_CHUNK + 5} <= n
    # the 16-byte accesses switched off by each pointer alone, on a factored tensor whose width allows them and on a flat one
    for kind in (fact, flat):
        offs = {c["off"] for c in kind}
        assert {(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)} <= offs
    assert any(ac.tile_vec(c["shape"], c["off"][0], c["off"][1]) for c in fact) and any(not ac.tile_vec(c["shape"], 0, 0) for c in fact)
    assert any(not ac.tile_vec(c["shape"], c["off"][0], c["off"][1]) and c["shape"][1] % 4 == 0 for c in fact)
    # the list: all three labels, frozen tensors of factored shape, NULL parameters, empty tensors, three launch groups
    entries = ac.mixed_list()
    assert {e["flags"] for e in entries} == {0, ac.DECAY, ac.FROZEN}
    assert any(e["flags"] & ac.FROZEN and min(ac.shape2(e["shape"])) >= 128 for e in entries) and any(e["null"] for e in entries)
    assert all(e["flags"] & ac.FROZEN for e in entries if e["null"])
    assert sum(1 for e in entries if ac.items_of(e["shape"], e["flags"]) == 0) == 2
    groups = ac.launches(entries)
    assert len(groups) == 3 and len(groups[0]) == ac.GROUP and all(0 < len(g) <= ac.GROUP for g in groups)
    assert {s for s in ac.SHAPES} <= {e["shape"] for e in entries}


# ---- the pin: the definition against transformers.optimization.Adafactor where the two coincide -----------------------------------------
PIN_SHAPES = ((128, 300), (300, 128), (128, 128), (257, 129), (1,), (63,), (4097,))


def test_definition_matches_transformers_adafactor():
    """Five steps, no global clip, no weight decay, lr 1e-2.  transformers factors EVERY 2-D tensor and normalises the row statistic;
    optax factors from 128 up and normalises the statistic of the smaller dimension — the two means are the same number in exact
    arithmetic — so the comparison is made on 1-D tensors and on matrices with both dimensions >= 128.

    The bound is for the fp32 side (torch, sums in an order this test does not know: (n + 2) U sum |terms|), per step and element:
        a mean of q over n terms                  (n + 4) U                         r_row: n = cols, r_col: n = rows
        v after k steps                           the mean's error + 3 U per step   (beta v + (1 - beta) mean: positive terms)
        u = g r_factor c_factor                   (r_row + r_col + (L + 2) U + 6 k U) / 2 + 8 U      (L entries in the normalised mean)
        flat: u = g / sqrt(v)                     (5 U + 3 k U) / 2 + 3 U
        RMS(u), RMS(p) over N elements            (N + 4) U / 2 + 2 U each
        the step  lr s u / max(1, RMS(u))         |step| (r_u + r_rmsu + r_rmsp + 4 U) + U |p|
    summed over the steps (the error of p feeds back only through RMS(p): second order)."""
    from transformers.optimization import Adafactor
    lr, steps = 1e-2, 5
    for i, shape in enumerate(PIN_SHAPES):
        scale = (1e-3, 1e-2, 1e-1, 1.0, 1e1)[i % 5]
        g0 = torch.Generator().manual_seed(40 + i)
        p0 = torch.randn(shape, generator=g0) * 0.5
        grads = [torch.randn(shape, generator=g0) * scale for _ in range(steps)]
        param = torch.nn.Parameter(p0.clone())
        opt = Adafactor([param], lr=lr, eps=(1e-30, 1e-3), clip_threshold=1.0, decay_rate=-0.8, beta1=None, weight_decay=0.0, scale_parameter=True,
                        relative_step=False, warmup_init=False)
        p, st = p0.double(), ref.zero_state(shape)
        bound, moved = torch.zeros(shape, dtype=F64), torch.zeros(shape, dtype=F64)
        N = p0.numel()
        for k, g in enumerate(grads):
            param.grad = g.clone()
            opt.step()
            beta, omb = ref.decay(k)
            p_new, st, info = ref.update_tensor(p, g, st, 1.0, beta, omb, lr, 0.0)
            if len(shape) == 2:
                r_u = 0.5 * ((shape[1] + 4) * U + (shape[0] + 4) * U + (min(shape) + 2) * U + 6 * (k + 1) * U) + 8 * U
            else:
                r_u = 0.5 * (5 * U + 3 * (k + 1) * U) + 3 * U
            r_rms = 0.5 * (N + 4) * U + 2 * U
            bound += (p_new - p).abs() * (r_u + 2 * r_rms + 4 * U) + U * p_new.abs()
            moved += (p_new - p).abs()
            p = p_new
        err = (param.detach().double() - p).abs()
        assert bool((err <= bound).all()), (shape, float((err / bound).max()))
        assert bool((moved > 50 * bound).all())          # (every element moved by fifty times its bound: a definition that is off by a few per cent of a step does not pass)


# ---- the two deliberate differences, by hand ------------------------------------------------------------------------------------------
def test_matrix_below_the_threshold_keeps_a_full_second_moment():
    """(127, 300): optax does not factor it (transformers would).  First step, coef 1: v = g^2 + 1e-30, u = g / sqrt(v) = sign(g),
    RMS(u) = 1, so p' = p - lr max(RMS(p), 1e-3) sign(g)"""
    g0 = torch.Generator().manual_seed(1)
    p, g = torch.randn(127, 300, generator=g0).double(), torch.randn(127, 300, generator=g0).double()
    assert set(ref.state_shapes((127, 300))) == {"v"} and set(ref.state_shapes((128, 300))) == {"v_row", "v_col"}
    beta, omb = ref.decay(0)
    pn, st, info = ref.update_tensor(p, g, ref.zero_state((127, 300)), 1.0, beta, omb, 1e-2, 0.0)
    assert torch.equal(st["v"], g * g + 1e-30)
    s = float(torch.sqrt((p * p).mean()))
    assert torch.allclose(pn, p - 1e-2 * s * torch.sign(g), rtol=1e-12, atol=1e-15) and abs(info["rms_u"] - 1.0) < 1e-12


def test_weight_decay_is_not_scaled_by_the_learning_rate():
    """g = 0: u = 0, and what is left of the update is the decay alone, p' = p - wd p = (1 - wd) p whatever lr is; without the decay
    flag p' = p"""
    p = torch.tensor([1.0, -2.0, 0.5, 4.0], dtype=F64)
    g = torch.zeros(4, dtype=F64)
    for lr in (1e-2, 10.0):
        out = ref.step([p, p], [g, g], [ref.zero_state((4,)), ref.zero_state((4,))], [ac.DECAY, 0], 0, lr, 0.25, None)
        assert torch.equal(out["params"][0], p - 0.25 * p) and torch.equal(out["params"][1], p)
    # and with a gradient: the decay adds -wd p to the lr-scaled step, it is not lr wd p
    g = torch.tensor([1.0, 1.0, -1.0, 1.0], dtype=F64)
    a = ref.step([p], [g], [ref.zero_state((4,))], [ac.DECAY], 0, 1e-2, 0.25, None)["params"][0]
    b = ref.step([p], [g], [ref.zero_state((4,))], [0], 0, 1e-2, 0.25, None)["params"][0]
    assert torch.allclose(b - a, 0.25 * p, rtol=1e-12, atol=0.0)


def test_global_clip_counts_frozen_tensors():
    p = [torch.ones(3, dtype=F64), torch.ones(2, dtype=F64)]
    g = [torch.tensor([3.0, 0.0, 0.0], dtype=F64), torch.tensor([4.0, 0.0], dtype=F64)]
    out = ref.step(p, g, [ref.zero_state((3,)), {}], [0, ac.FROZEN], 2, 1e-2, 0.0, 1.0)
    assert out["norm"] == 5.0 and out["coef"] == 0.2 and out["t"] == 3 and torch.equal(out["params"][1], p[1])
    assert ref.step(p, g, [ref.zero_state((3,)), {}], [0, ac.FROZEN], 2, 1e-2, 0.0, 5.0)["coef"] == 1.0          # norm == max_grad_norm: 5 / 5
    bad = ref.step(p, [g[0], torch.tensor([float("nan"), 0.0], dtype=F64)], [ref.zero_state((3,)), {}], [0, ac.FROZEN], 2, 1e-2, 0.0, 1.0)
    assert bad["skipped"] == 1 and bad["t"] == 2 and torch.equal(bad["params"][0], p[0])


# ---- the C ABI and the build ---------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(REPO, "include", "zett_hip.h")).read()


def test_abi_is_additive_and_declared_once():
    from zett_amd import _lib, build
    header = _header()
    for name in ("zett_op_adafactor_workspace_floats", "zett_op_adafactor_step"):
        assert re.search(r"\bint " + name + r"\(", header) and name in _lib.ABI_SYMBOLS and hasattr(_lib.load(), name)
    assert int(re.search(r"#define ZETT_ABI_VERSION (\d+)", header).group(1)) == _lib.ABI_VERSION == 8
    for macro, value in (("ZETT_ADAFACTOR_TILE_ROWS", _lib.ADAFACTOR_TILE_ROWS), ("ZETT_ADAFACTOR_TILE_COLS", _lib.ADAFACTOR_TILE_COLS), ("ZETT_ADAFACTOR_GROUP", _lib.ADAFACTOR_GROUP)):
        assert int(re.search(r"#define " + macro + r" (\d+)", header).group(1)) == value
    assert (ac.TILE_ROWS, ac.TILE_COLS, ac.GROUP, ac.MT_CHUNK) == (_lib.ADAFACTOR_TILE_ROWS, _lib.ADAFACTOR_TILE_COLS, _lib.ADAFACTOR_GROUP, _lib.MT_CHUNK)
    assert "train_adafactor.hip" in build.SOURCES and "train_adafactor.hip" in build.TRAINING_ONLY
    assert re.search(r"train\.py:631-656", header) and "scale_by_factored_rms" in header and "add_decayed_weights" in header
    src = open(os.path.join(build.CSRC, "train_adafactor.hip")).read()
    assert "atomic" not in src.replace("no atomics", "")          # fixed-order sums only


def _arr(ctype, vals):
    return (ctype * max(1, len(vals)))(*vals)


def test_workspace_size_and_argument_checks():
    """zett_op_adafactor_workspace_floats restated (it runs on the host), and what zett_op_adafactor_step refuses before any launch"""
    from zett_amd import _lib
    lib = _lib.load()
    entries = ac.mixed_list()
    rows, cols, flags = ([ac.shape2(e["shape"])[0] for e in entries], [ac.shape2(e["shape"])[1] for e in entries], [e["flags"] for e in entries])
    up = lambda n: (n + 15) // 16 * 16
    want = 0
    for e in entries:
        R, Cc = ac.shape2(e["shape"])
        if R * Cc and ac.is_factored(e["shape"], e["flags"]):
            want += up(-(-Cc // ac.TILE_COLS) * R + -(-R // ac.TILE_ROWS) * Cc + -(-min(R, Cc) // ac.SEG))
    items = sum(ac.items_of(e["shape"], e["flags"]) for e in entries)
    want += 3 * up(items) + up(4 * sum(1 for e in entries if ac.items_of(e["shape"], e["flags"])))
    got = C.c_int64(-1)
    assert lib.zett_op_adafactor_workspace_floats(_arr(C.c_int64, rows), _arr(C.c_int64, cols), _arr(C.c_uint8, flags), len(entries), C.byref(got)) == 0
    assert got.value == want
    assert lib.zett_op_adafactor_workspace_floats(None, None, None, 0, C.byref(got)) == 0 and got.value == 16
    one = (_arr(C.c_int64, [4]), _arr(C.c_int64, [4]), _arr(C.c_uint8, [0]))
    assert lib.zett_op_adafactor_workspace_floats(*one, 1, None) == _lib.E_INVALID
    assert lib.zett_op_adafactor_workspace_floats(_arr(C.c_int64, [-1]), one[1], one[2], 1, C.byref(got)) == _lib.E_INVALID
    assert lib.zett_op_adafactor_workspace_floats(one[0], one[1], _arr(C.c_uint8, [4]), 1, C.byref(got)) == _lib.E_INVALID          # an unknown flag
    # the step: every refusal returns before a launch (no device is touched: the pointers are made-up, 16-byte aligned numbers)
    fake = lambda v: _arr(C.c_void_p, [v])
    ok = dict(params=fake(4096), grads=fake(8192), v_row=fake(None), v_col=fake(None), v=fake(12288))
    def call(workspace=16384, floats=64, record=20480, max_norm=1.0, **over):
        a = dict(ok, **over)
        return lib.zett_op_adafactor_step(a["params"], a["grads"], a["v_row"], a["v_col"], a["v"], *one, 1, 1e-2, 0.0, max_norm, 0, workspace, floats, record, None)
    for kw in (dict(record=None), dict(workspace=None), dict(floats=8), dict(workspace=16388), dict(max_norm=0.0), dict(max_norm=float("nan")), dict(grads=fake(None)),
               dict(params=fake(None)), dict(v=fake(None)), dict(params=fake(4098)), dict(params=None)):
        assert call(**kw) == _lib.E_INVALID, kw
        assert lib.zett_last_error()
    fact = (_arr(C.c_int64, [128]), _arr(C.c_int64, [128]), _arr(C.c_uint8, [1]))
    assert lib.zett_op_adafactor_step(ok["params"], ok["grads"], fake(None), fake(64), fake(None), *fact, 1, 1e-2, 0.0, 1.0, 0, 16384, 1 << 20, 20480, None) == _lib.E_INVALID      # a factored tensor without v_row


# ---- the optimizer's host side ------------------------------------------------------------------------------------------------------------
class _Toy(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.big = torch.nn.Linear(300, 128)                 # weight [128, 300]: factored; bias: no_decay
        self.small = torch.nn.Linear(300, 127, bias=False)   # [127, 300]: a full second moment
        self.scaler = torch.nn.Linear(4, 4)                  # frozen by its name
        self.refreshed = 0

    def refresh_weights(self):
        self.refreshed += 1


def test_state_shapes_follow_the_factoring_rule():
    from zett_amd import training
    for shape in ac.SHAPES + ((300, 300), (5000, 128)):
        assert training.adafactor_state_shapes(shape) == ref.state_shapes(shape), shape
    with pytest.raises(ValueError):
        training.adafactor_state_shapes((2, 3, 4))


def test_optimizer_refuses_on_the_host_before_any_launch():
    from zett_amd import training
    def opt_for(mutate):
        m = _Toy()
        for p in m.parameters():
            p.grad = torch.zeros_like(p)
        mutate(m)
        return training.HypernetAdafactor(m, lr=1e-3), m
    def conv(m):
        m.conv = torch.nn.Conv1d(2, 2, 3)
        for p in m.conv.parameters():
            p.grad = torch.zeros_like(p)
    def half(m):
        m.big.weight.data = m.big.weight.data.half()
        m.big.weight.grad = torch.zeros_like(m.big.weight)
    def strided(m):
        m.small.weight.grad = torch.zeros(300, 127).t()
    def other_device(m):
        m.extra = torch.nn.Linear(3, 3, device="meta")          # a parameter (and its gradient) on another device than the first one's
        for p in m.extra.parameters():
            p.grad = torch.zeros_like(p)
    for mutate in (conv, half, strided, other_device):
        opt, m = opt_for(mutate)
        with pytest.raises(ValueError):
            opt.step()
        assert m.refreshed == 0 and not opt.state
    with pytest.raises(TypeError):
        training.HypernetAdafactor(torch.nn.Linear(2, 2), lr=1e-3)
    with pytest.raises(ValueError):
        training.HypernetAdafactor(_Toy(), lr=1e-3, max_grad_norm=0.0)


def test_state_dict_round_trip_and_shape_check():
    from zett_amd import training
    m = _Toy()
    opt = training.HypernetAdafactor(m, lr=2e-3, weight_decay=0.05, max_grad_norm=None)
    assert opt.labels["big.weight"] == "decay" and opt.labels["big.bias"] == "no_decay" and opt.labels["scaler.weight"] == "frozen"
    assert opt.last_step_stats() == {"grad_norm": 0.0, "clip_coef": 1.0, "skipped": 0, "step": 0}
    state = {"big.weight": {"v_row": torch.rand(128), "v_col": torch.rand(300)}, "big.bias": {"v": torch.rand(128)}, "small.weight": {"v": torch.rand(127, 300)}}
    sd = {"step": 7, "state": state, "hyper": {"lr": 1e-2, "weight_decay": 0.0, "max_grad_norm": 0.5}, "labels": dict(opt.labels, **{"big.bias": "decay"})}
    opt.load_state_dict(sd)
    back = opt.state_dict()
    assert back["step"] == 7 and back["hyper"] == sd["hyper"] and back["labels"]["big.bias"] == "decay"
    assert set(back) == {"step", "state", "hyper", "labels"}
    for n in state:
        assert set(back["state"][n]) == set(state[n]) and all(torch.equal(back["state"][n][k], state[n][k]) for k in state[n])
    other = training.HypernetAdafactor(_Toy(), lr=1.0)
    other.load_state_dict(back)
    assert other.state_dict()["hyper"] == sd["hyper"] and other.last_step_stats()["step"] == 7
    for wrong in ({"big.weight": {"v": torch.rand(128, 300)}},                                   # a factored parameter with a full moment
                  {"big.weight": {"v_row": torch.rand(300), "v_col": torch.rand(128)}},          # the two statistics swapped
                  {"small.weight": {"v_row": torch.rand(127), "v_col": torch.rand(300)}},        # factored below the threshold
                  {"big.bias": {"v": torch.rand(127)}}):
        with pytest.raises(ValueError):
            opt.load_state_dict({"step": 1, "state": wrong})
    with pytest.raises(KeyError):
        opt.load_state_dict({"step": 1, "state": {"nope": {"v": torch.rand(1)}}})
    with pytest.raises(KeyError):
        opt.load_state_dict({"state": {}})
    with pytest.raises(ValueError):
        opt.load_state_dict({"step": -1, "state": {}})
    assert opt.state_dict()["step"] == 7          # (the refused loads left the optimizer as it was)


def test_make_optimizer_maps_the_training_arguments():
    from types import SimpleNamespace
    from zett_amd import training
    m = _Toy()
    a = training.make_optimizer(m, SimpleNamespace(use_adafactor=True, learning_rate=[3e-4, 1e-5], weight_decay=0.01, max_grad_norm=0.1, adam_beta1=0.8, adam_beta2=0.9, adam_epsilon=1e-6))
    assert type(a) is training.HypernetAdafactor and (a.lr, a.weight_decay, a.max_grad_norm) == (3e-4, 0.01, 0.1)
    b = training.make_optimizer(m, SimpleNamespace(use_adafactor=False, learning_rate=6e-5, weight_decay=0.02, max_grad_norm=None, adam_beta1=0.8, adam_beta2=0.9, adam_epsilon=1e-6))
    assert type(b) is training.HypernetAdamW and (b.lr, b.betas, b.eps, b.weight_decay, b.max_grad_norm) == (6e-5, (0.8, 0.9), 1e-6, 0.02, None)
    c = training.make_optimizer(m, {"learning_rate": 1e-3})          # the reference's defaults (train.py:91-101)
    assert type(c) is training.HypernetAdamW and (c.betas, c.eps, c.weight_decay, c.max_grad_norm) == ((0.9, 0.999), 1e-8, 0.0, None)
    d = training.make_optimizer(m, {"use_adafactor": True}, labels={"big.": "frozen"})
    assert type(d) is training.HypernetAdafactor and d.lr == 3e-4 and d.labels["big.weight"] == "frozen"
    for name in ("step", "zero_grad", "last_step_stats", "state_dict", "load_state_dict"):
        assert callable(getattr(a, name)) and callable(getattr(b, name))
    with pytest.raises(ValueError):
        training.make_optimizer(m, {"learning_rate": []})
