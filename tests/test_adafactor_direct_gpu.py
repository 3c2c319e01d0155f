"""The Adafactor step (zett_amd/csrc/train_adafactor.hip) called directly through the C ABI and checked ELEMENT BY ELEMENT against
float64 on the same values (tests/adafactor_check.py, whose definition is tests/adafactor_ref.py), at the edges: the factoring
threshold on either dimension, one row / column short of, at and past a tile, the 256-entry statistics segment and the vector width,
pointers that break the 16-byte alignment one at a time, frozen / decaying / non-decaying tensors in one list across three launch
groups with empty tensors in it, zero gradients, the parameter-scale floor, both sides of the block clip and of the global clip, and
the skipped step.

Buffers follow tests/test_loss_step_direct_gpu.py: every parameter, gradient and statistic is a view INSIDE a larger allocation with
canary slack that is checked after each call; the workspace is NaN before the call.  Nothing here is meant to fault.

The case tables are tests/adafactor_check.py's, built without a GPU; tests/test_adafactor_check_host.py asserts that they reach every
branch.
"""
import ctypes as C
import os

import pytest
import torch

from tests import adafactor_check as ac
from tests import adafactor_ref as ref
from tests import loss_step_check as lc
from tests import test_train_ops_direct_gpu as d
from tests import train_ops_check as tc

DEV = d.DEV
gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
NULL = d.NULL
O = d.O
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _record():
    before = dict(tc.RECORD)
    yield
    path = os.environ.get(ac.RECORD_ENV)          # figures for profiles/adafactor_check.md
    mine = {k: v for k, v in tc.RECORD.items() if k not in before}
    if path and mine:
        everything = dict(tc.RECORD)
        tc.RECORD.clear()
        tc.RECORD.update(mine)
        try:
            tc.write_record(path)
        finally:
            tc.RECORD.clear()
            tc.RECORD.update(everything)


def _lib():
    return d._lib()[1]


def _arr(ctype, vals):
    return (ctype * max(1, len(vals)))(*vals)


def _flat(shape):
    n = 1
    for s in shape:
        n *= s
    return n


class Run:
    """one call of zett_op_adafactor_step on framed buffers: .p / .g / .st the values before it, .got_* what it left"""

    def __init__(self, entries, t0, max_norm, zero_grad, what, lr=ac.HYPER["lr"], wd=ac.HYPER["wd"], zero_state=False, seed=0, host=None):
        self.entries, self.t0, self.max_norm, self.zero_grad, self.what, self.lr, self.wd = entries, t0, max_norm, zero_grad, what, lr, wd
        n = len(entries)
        self.p, self.g, self.st, self.P, self.G, self.S = [], [], [], [], [], []
        for i, e in enumerate(entries):
            p, g, st = host[i] if host is not None else (ac.values(e, i, 0, seed), ac.values(e, i, 1, seed), ac.values(e, i, 2, seed))
            if zero_state:
                st = {k: torch.zeros_like(v) for k, v in st.items()}
            self.p.append(p), self.g.append(g), self.st.append(st)
            self.P.append(O(None, _flat(e["shape"]), values=p.reshape(-1), shift=e["off"][0]))
            self.G.append(O(None, _flat(e["shape"]), values=g.reshape(-1), shift=e["off"][1]))
            self.S.append({k: O(None, v.numel(), values=v.reshape(-1), shift=e["off"][2]) for k, v in st.items()})
        rows = [ac.shape2(e["shape"])[0] for e in entries]
        cols = [ac.shape2(e["shape"])[1] for e in entries]
        flags = [e["flags"] for e in entries]

        def ptrs(get):
            return _arr(C.c_void_p, [get(i) for i in range(n)])

        gone = lambda i: entries[i]["null"]
        arrs = (ptrs(lambda i: None if gone(i) else self.P[i].ptr()), ptrs(lambda i: self.G[i].ptr()),
                ptrs(lambda i: self.S[i]["v_row"].ptr() if "v_row" in self.S[i] and not gone(i) else None),
                ptrs(lambda i: self.S[i]["v_col"].ptr() if "v_col" in self.S[i] and not gone(i) else None),
                ptrs(lambda i: self.S[i]["v"].ptr() if "v" in self.S[i] and not gone(i) else None))
        R, Cc, Fl = _arr(C.c_int64, rows), _arr(C.c_int64, cols), _arr(C.c_uint8, flags)
        need = C.c_int64(-1)
        d._ok(_lib().zett_op_adafactor_workspace_floats(R, Cc, Fl, n, C.byref(need)), what + " workspace")
        assert need.value >= 16
        self.ws = torch.full((need.value + 64,), NAN, dtype=F32, device=DEV)
        seed_rec = torch.zeros(8, dtype=F32)
        seed_rec.view(torch.int32)[3] = t0
        seed_rec[6], seed_rec[7] = 5.0, 6.0
        self.REC = O(None, 8, values=seed_rec)
        d._ok(_lib().zett_op_adafactor_step(*arrs, R, Cc, Fl, n, lr, wd, max_norm, zero_grad, C.c_void_p(self.ws.data_ptr()), need.value, self.REC.ptr(), d._stream()), what)
        self.words = self.REC.back(what + " record", inside=False)          # (the norm of a skipped step is not finite)
        self.iw = self.words.view(torch.int32)
        self.got_p = [self.P[i].back(f"{what} p {i}").reshape(e["shape"]) for i, e in enumerate(entries)]
        self.got_g = [self.G[i].back(f"{what} g {i}", inside=False).reshape(e["shape"]) for i, e in enumerate(entries)]
        self.got_s = [{k: o.back(f"{what} {k} {i}").reshape(self.st[i][k].shape) for k, o in self.S[i].items()} for i in range(n)]
        assert bool(torch.isnan(self.ws[need.value:]).all().cpu()), what + ": the workspace was written past the size the library asked for"

    def verify(self, key):
        """the record, then every tensor against float64 from the record's scalars.  -> the per-tensor references"""
        what, entries = self.what, self.entries
        want = ac.record_ref(self.g, self.max_norm, self.t0)
        tc.exact(self.iw[2:4], torch.tensor([want["skip"], want["t"]], dtype=torch.int32), what + " skip, count", key=("adafactor skip, count", key))
        tc.exact(self.words[6:], torch.zeros(2), what + " words 6, 7", key=("adafactor skip, count", key))
        names = ("coef", "beta", "omb") if want["skip"] else ("norm", "coef", "beta", "omb")
        idx = dict(norm=0, coef=1, beta=4, omb=5)
        tc.check(torch.stack([self.words[idx[nm]] for nm in names]), torch.stack([want[nm][0] for nm in names]), torch.stack([torch.as_tensor(want[nm][1], dtype=F64) for nm in names]),
                 what + " " + ", ".join(names), key=("adafactor record", key))
        coef, beta, omb = float(self.words[1]), float(self.words[4]), float(self.words[5])
        refs = []
        for i, e in enumerate(entries):
            name = f"{what} tensor {i} {e['shape']} flags {e['flags']} offsets {e['off']}"
            if _flat(e["shape"]) == 0:
                refs.append(None)
                continue
            kind = "factored" if ac.is_factored(e["shape"], e["flags"]) else "flat"
            layout = kind + (" vector" if all(o % 4 == 0 for o in e["off"]) and ac.shape2(e["shape"])[1] % 4 == 0 else " element")
            cleared = bool(self.zero_grad)
            tc.exact(self.got_g[i], torch.zeros(e["shape"]) if cleared else self.g[i], name + (": the gradient is cleared" if cleared else ": the gradient is unchanged"), key=("adafactor gradient", layout))
            if want["skip"] or e["flags"] & ac.FROZEN:
                tc.exact(self.got_p[i], self.p[i], name + ": p of a frozen tensor or a skipped step is untouched", key=("adafactor untouched", layout))
                for k in self.st[i]:
                    tc.exact(self.got_s[i][k], self.st[i][k], name + f": {k} of a frozen tensor or a skipped step is untouched", key=("adafactor untouched", layout))
                refs.append(None)
                continue
            r = ac.tensor_step(self.p[i], self.g[i], self.st[i], e["flags"], coef, beta, omb, self.lr, self.wd, e["off"])
            for k in r["state"]:          # (recorded apart on the first step from zero statistics: there v_row / v_col ARE the long sums)
                tc.check(self.got_s[i][k], r["state"][k], r["b_state"][k], f"{name} {k}", key=(f"adafactor {k}", layout + (", first step" if key == "t = 0" else "")))
            tc.check(self.got_p[i], r["p"], r["b_p"], f"{name} p", key=("adafactor p", layout))
            refs.append(r)
        return refs


# ---- every shape alone ---------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("i", range(len(ac.single_cases())), ids=lambda i: "{}-{}".format("x".join(map(str, ac.single_cases()[i]["shape"])), "".join(map(str, ac.single_cases()[i]["off"]))))
def test_one_tensor(i):
    """the first step from zero statistics (beta = 0: the statistics are the plain means of q, held to the sum bounds) without a clip,
    then a sixth step from given statistics under the global clip, gradients cleared"""
    e = ac.single_cases()[i]
    Run([e], 0, 1e6, 0, f"adafactor first step {e['shape']}", zero_state=True).verify("t = 0")
    Run([e], 5, 0.05, 1, f"adafactor sixth step {e['shape']}", seed=1).verify("t = 5")


@gpu
def test_first_step_of_a_flat_tensor_is_exact():
    """t = 0, below the clip: beta = 0, 1 - beta = 1 and coef = 1, so v = fl(fl(g^2) + 1e-30) to the bit (no addition to round)"""
    for shape in ((127, 300), (4097,), (5,)):
        for off in ((0, 0, 0), (1, 1, 1)):
            e = ac.entry(shape, off=off)
            run = Run([e], 0, 1e6, 0, f"adafactor exact first step {shape} {off}", zero_state=True)
            tc.exact(run.words[1:2], torch.ones(1), "coef below the clip", key=("adafactor exact", "coef"))
            tc.exact(run.words[4:6], torch.tensor([0.0, 1.0]), "beta, 1 - beta at t = 0", key=("adafactor exact", "beta"))
            g = run.g[0]
            tc.exact(run.got_s[0]["v"], g * g + torch.tensor(1e-30, dtype=F32), f"v = q at t = 0 {shape} {off}", key=("adafactor exact", "v = q"))


# ---- the list ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("zero_grad", (0, 1))
def test_mixed_list(zero_grad):
    """every shape in one list with frozen, decaying and non-decaying tensors, NULL parameters of frozen ones, two empty tensors and three
    launch groups: each tensor as if it were alone, the norm over all of them; a second run gives the same bits"""
    entries = ac.mixed_list()
    assert len(ac.launches(entries)) == 3
    a = Run(entries, 3, 2.0, zero_grad, f"adafactor mixed list zero_grad={zero_grad}")
    a.verify(f"list zero_grad={zero_grad}")
    b = Run(entries, 3, 2.0, zero_grad, "adafactor mixed list, again")
    for i in range(len(entries)):
        if _flat(entries[i]["shape"]) == 0:
            continue
        tc.exact(b.got_p[i], a.got_p[i], f"tensor {i}: p of a second run", key=("adafactor rerun", "p"))
        for k in a.got_s[i]:
            tc.exact(b.got_s[i][k], a.got_s[i][k], f"tensor {i}: {k} of a second run", key=("adafactor rerun", k))
    tc.exact(b.words, a.words, "the record of a second run", key=("adafactor rerun", "record"))


@gpu
def test_item_stride():
    """2 049 tiles in one launch of at most 2 048 workgroups: the first workgroup takes a second item; every element of p, v_row, v_col"""
    assert ac.items_of(ac.STRIDE_SHAPE, ac.DECAY) == ac.MT_GRID + 1
    Run([ac.entry(ac.STRIDE_SHAPE, g_scale=0.05)], 2, 0.5, 1, "adafactor item stride").verify("item stride")


# ---- special values --------------------------------------------------------------------------------------------------------------------
@gpu
def test_zero_gradient():
    """g == 0 on a factored and on a flat tensor without decay: q = 1e-30, u = 0, p keeps its bits, the statistics stay finite"""
    entries = [ac.entry((130, 260), flags=0, g_zero=True), ac.entry((127, 300), flags=0, g_zero=True), ac.entry((77,), flags=0, g_zero=True)]
    for t0, zero_state in ((0, True), (4, False)):
        run = Run(entries, t0, 1.0, 0, f"adafactor zero gradient t0={t0}", zero_state=zero_state)
        run.verify(f"g = 0, t = {t0}")
        tc.exact(run.words[:2], torch.tensor([0.0, 1.0]), "norm 0, coef 1", key=("adafactor exact", "g = 0 record"))
        for i in range(len(entries)):
            tc.exact(run.got_p[i], run.p[i], f"tensor {i}: the update of a zero gradient is zero", key=("adafactor exact", "g = 0 p"))
            for k, v in run.got_s[i].items():
                assert bool(torch.isfinite(v).all()) and bool((v > 0).all()), (i, k)


@gpu
def test_parameter_scale_floor():
    """p == 0 (s = 1e-3), and RMS(p) a part in a thousand below and above 1e-3, on a factored and on a flat tensor"""
    for shape in ((128, 256), (300,)):
        for level, floor in ((0.0, True), (0.999e-3, True), (1.001e-3, False)):
            e = ac.entry(shape)
            p = torch.full(shape, level) * torch.where(torch.arange(_flat(shape)).reshape(shape) % 2 == 0, 1.0, -1.0)
            host = [(p, ac.values(e, 0, 1), ac.values(e, 0, 2))]
            r = Run([e], 2, 1e6, 0, f"adafactor RMS(p) = {level} {shape}", host=host).verify(f"RMS(p) = {level}")[0]
            assert (r["s_raw"] <= lc.f32(ref.EPS_SCALE)) == floor and (r["s"] == lc.f32(ref.EPS_SCALE)) == floor, (shape, level, r["s"], r["s_raw"])


@gpu
def test_block_clip_on_both_sides():
    """RMS(u) well below 1 (u passes unscaled) and well above 1 (u is divided by it), factored and flat"""
    for shape in ((129, 257), (4097,)):
        for g_scale, above in ((1e-3, False), (10.0, True)):
            r = Run([ac.entry(shape, g_scale=g_scale)], 5, 1e6, 0, f"adafactor RMS(u) {shape} g_scale={g_scale}").verify(f"RMS(u) {'>' if above else '<'} 1")[0]
            assert (r["rms_u"] > 1.0) == above, (shape, g_scale, r["rms_u"])


@gpu
def test_global_clip_on_both_sides_and_at_the_threshold():
    """norm < max_norm: coef exactly 1; norm > max_norm; and sum g^2 == max_norm^2 exactly (3, 4 -> 5.0), where `<` is false and
    coef = 5 / 5 is 1.0 all the same"""
    e = ac.entry((5,), flags=0)
    g = torch.tensor([3.0, 4.0, 0.0, 0.0, 0.0])
    host = [(ac.values(e, 0, 0), g, ac.values(e, 0, 2))]
    for max_norm, coef in ((6.0, 1.0), (5.0, 1.0), (2.5, 0.5)):
        run = Run([e], 1, max_norm, 0, f"adafactor max_norm={max_norm}", host=host)
        run.verify(f"max_norm = {max_norm}")
        tc.exact(run.words[:2], torch.tensor([5.0, coef]), f"norm, coef at max_norm = {max_norm}", key=("adafactor exact", "clip"))
    run = Run([e], 1, float("inf"), 0, "adafactor without a clip", host=host)
    run.verify("max_norm = inf")
    tc.exact(run.words[1:2], torch.ones(1), "coef without a clip", key=("adafactor exact", "clip"))


@gpu
@pytest.mark.parametrize("zero_grad", (0, 1))
def test_skipped_step(zero_grad):
    """one inf, one NaN, one overflow of g * g, each in a factored, a flat or a frozen tensor of a short list: skip = 1, coef 0, no
    parameter, no statistic and not the count written; the gradients are cleared only where the call asks for it"""
    entries = [ac.entry((128, 130)), ac.entry((70,), flags=0), ac.entry((40,), flags=ac.FROZEN), ac.entry((127, 129))]
    for where, bad in ((0, float("inf")), (1, NAN), (2, float("inf")), (3, 1e20)):
        host = [[ac.values(e, i, 0), ac.values(e, i, 1), ac.values(e, i, 2)] for i, e in enumerate(entries)]
        host[where][1].view(-1)[3] = bad
        run = Run(entries, 7, 1.0, zero_grad, f"adafactor {bad} in tensor {where} zero_grad={zero_grad}", host=host)
        tc.exact(run.iw[2:4], torch.tensor([1, 7], dtype=torch.int32), "skip, count", key=("adafactor skip, count", "not finite"))
        tc.exact(run.words[1:2], torch.zeros(1), "coef of a skipped step", key=("adafactor exact", "skip coef"))
        assert not bool(torch.isfinite(run.words[0]))
        for i, e in enumerate(entries):
            tc.exact(run.got_p[i], run.p[i], f"tensor {i}: p after a skipped step", key=("adafactor untouched", "skip"))
            for k in run.st[i]:
                tc.exact(run.got_s[i][k], run.st[i][k], f"tensor {i}: {k} after a skipped step", key=("adafactor untouched", "skip"))
            if zero_grad:
                tc.exact(run.got_g[i], torch.zeros(e["shape"]), f"tensor {i}: the gradient is cleared", key=("adafactor gradient", "skip"))
            else:
                assert torch.equal(lc._bits(run.got_g[i]), lc._bits(run.g[i])), f"tensor {i}: the gradient of a skipped step without zero_grad changed"
