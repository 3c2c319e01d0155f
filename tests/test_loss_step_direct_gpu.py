"""The loss kernels (zett_amd/csrc/train_loss.hip) and the distance losses and optimizer step (zett_amd/csrc/train_step.hip) called
directly through the C ABI and checked ELEMENT BY ELEMENT against float64 on the same values (tests/loss_step_check.py), at the
edges: every register layout of the rows pass at, one vector below and one vector past its limit, both paths, leading dimensions
wider than the data, every form of the gradient operand, ties of the maximum in every place two maxima can meet, every term that
switches the 4-element accesses of the distance kernels off, ids outside the int32 range, the 64-tensor launch boundary with empty
tensors in the list, every grid at a size past its cap.

Buffers follow tests/test_train_ops_direct_gpu.py (OnDev, I, O): every floating-point input is a view INSIDE a larger allocation
whose slack — the columns cols .. ld - 1 included — is NaN, every output has canary slack that is checked after each call, integer
inputs have slack of a sentinel that would be a wild index if it were read.  Nothing here is meant to fault: a wrong index stays
inside this test's own allocation.

The case tables are tests/loss_step_check.py's, built without a GPU; tests/test_loss_step_check_host.py asserts that they reach
every branch.
"""
import ctypes as C
import os

import pytest
import torch

from tests import loss_step_check as lc
from tests import test_train_ops_direct_gpu as d
from tests import train_ops_check as tc

DEV = d.DEV
gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
NULL = d.NULL
I, O, OnDev = d.I, d.O, d.OnDev
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _record():
    before = dict(tc.RECORD)                      # (the record is shared with tests/test_train_ops_direct_gpu.py: only this file's keys are written)
    yield
    path = os.environ.get(lc.RECORD_ENV)          # figures for profiles/loss_step_check.md
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


def _ok(rc, what):
    d._ok(rc, what)


class Ints:
    """an integer input on the device, 64 elements of `sentinel` in front of and behind it"""

    def __init__(self, values, sentinel):
        flat = values.contiguous().flatten()
        host = torch.full((flat.numel() + 128,), sentinel, dtype=values.dtype)
        host[64:64 + flat.numel()] = flat
        self.buf = host.to(DEV)

    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 64 * self.buf.element_size())


def _opt(x):
    return NULL if x is None else x.ptr()


def _ints(out, what):
    """an int32 output kept in a canary-framed fp32 vector: -> its words (a word left at the canary is a NaN and fails in back())"""
    return out.back(what).view(torch.int32)


# ---- zett_op_ce_rows -------------------------------------------------------------------------------------------------------------
def _ce_call(z, labels, weight, v, ld_z, ld_g, gform, path, what):
    """one call on fresh framed buffers -> dict(lse, loss, argmax, G or None) on the host, canaries and untouched buffers checked"""
    lib = _lib()
    rows, vp = z.shape
    slack = 256 if vp <= 64 else 8
    Z = OnDev(lc.Slim(rows, vp, ld_z, F32, NAN, slack, values=z))
    LAB, W = Ints(labels, 2 ** 31 - 5), None if weight is None else I(weight)
    loss, lse, am = O(None, rows), O(None, rows), O(None, rows)
    G = None
    if gform in ("f32", "bf16", "f16"):
        G = OnDev(lc.Slim(rows, vp, ld_g, lc.DT[gform], "canary", slack))
    g_ptr = NULL if gform is None else Z.ptr() if gform == "inplace" else G.ptr()
    code = lc.DT_CODE["f32" if gform in (None, "inplace") else gform]
    _ok(lib.zett_op_ce_rows(Z.ptr(), ld_z, LAB.ptr(), _opt(W), rows, v, vp, g_ptr, code, ld_g, loss.ptr(), lse.ptr(), am.ptr(), path, d._stream()), what)
    out = dict(lse=lse.back(what + " lse"), loss=loss.back(what + " row_loss"), argmax=_ints(am, what + " argmax"), G=None)
    after = Z.buf.cpu()
    if gform == "inplace":
        lc.check_outside(Z.f, after, what + " logits overwritten by G")
        out["G"] = Z.f.view(after).clone()
    else:
        lc.unchanged(after, Z.f.buf, what + " logits")
        if G is not None:
            out["G"] = G.back(what + " G")
    return out


def _ce_verify(got, z, labels, weight, v, gform, what, layout, slice_rel=lc.REL_LOSS, want_argmax=None):
    vp = z.shape[1]
    ref = lc.ce_rows_ref(z, labels, weight, v)
    bnd = lc.ce_rows_bound(ref, vp)
    tc.exact(got["argmax"], ref["argmax"] if want_argmax is None else want_argmax, what + " argmax", key=("ce_rows argmax", layout))
    if want_argmax is not None:
        assert torch.equal(ref["argmax"], want_argmax), (ref["argmax"], want_argmax)
    tc.check(got["lse"], ref["lse"], bnd["lse"], what + " lse", key=("ce_rows lse", layout), slice_rel=slice_rel)
    tc.check(got["loss"], ref["loss"], bnd["loss"], what + " row_loss", key=("ce_rows row_loss", layout), slice_rel=slice_rel)
    dead = ~ref["live"]
    if bool(dead.any()):
        tc.exact(got["loss"][dead], torch.zeros(int(dead.sum())), what + " row_loss of the rows of weight 0", key=("ce_rows zero rows", layout))
    if gform is None:
        return
    gt = F32 if gform == "inplace" else lc.DT[gform]
    G = got["G"]
    b = bnd["G"] if gt == F32 else tc.lo_bound(ref["G"], bnd["G"], gt)
    tc.check(G[:, :v], ref["G"][:, :v], b[:, :v], what + " G", key=(f"ce_rows G {gform}", layout))
    normal = ref["w"].abs() >= 2.0 ** -100          # (a row of subnormal values has no relative accuracy to hold a norm to: its elements are held above)
    if gt == F32 and slice_rel is not None and bool(normal.any()):
        tc.check(G[normal][:, :v], ref["G"][normal][:, :v], b[normal][:, :v], what + " G, rows and columns", key=(f"ce_rows G {gform}", layout), slice_rel=slice_rel)
    if vp > v:
        tc.exact(G[:, v:].contiguous(), torch.zeros(G.shape[0], vp - v, dtype=gt), what + " G pad columns", key=("ce_rows G pad", layout))
    if bool(dead.any()):
        tc.exact(G[dead].contiguous(), torch.zeros(int(dead.sum()), vp, dtype=gt), what + " G of the rows of weight 0", key=("ce_rows zero rows", layout))


def _ce_both_paths(z, labels, weight, v, ld_z, ld_g, gform, what, slice_rel=lc.REL_LOSS, want_argmax=None):
    vp = z.shape[1]
    first = None
    for path in ((lc.CE_AUTO, lc.CE_TWICE) if vp <= lc.CE_ONCE_MAX else (lc.CE_AUTO,)):
        nv = lc.ce_nv(vp, path)
        name = f"{what} {'twice' if nv == 0 else 'once NV=' + str(nv)}"
        got = _ce_call(z, labels, weight, v, ld_z, ld_g, gform, path, name)
        _ce_verify(got, z, labels, weight, v, gform, name, f"NV={nv}", slice_rel, want_argmax)      # each path against float64: their equality alone proves nothing
        if first is None:
            first = got
        else:
            for k in ("lse", "loss", "argmax", "G"):
                if got[k] is not None:
                    tc.exact(got[k], first[k], f"{what}: the two-read path against the read-once path, {k}", key=("ce_rows once == twice", k))


@gpu
@pytest.mark.parametrize("case", lc.ce_cases(), ids=lambda c: f"vp{c['vp']}-v{c['v']}-{c['g']}")
def test_ce_rows(case):
    """lse, row_loss, argmax (every row, no gap filter) and every element of G in every register layout, read once and read twice"""
    z, labels, weight = lc.ce_inputs(case)
    vp = case["vp"]
    what = f"ce_rows v={case['v']} v_padded={vp} rows={case['rows']} ld_z={vp + case['d_z']} ld_g={vp + case['d_g']} g={case['g']} pad={case['pad']}"
    _ce_both_paths(z, labels, weight, case["v"], vp + case["d_z"], vp + case["d_g"], case["g"], what)


@gpu
@pytest.mark.parametrize("gform", ("f32", "bf16", "inplace"))
def test_ce_rows_ties_and_ranges(gform):
    """bit-identical maxima inside a float4, in two vectors of one lane, in two lanes, in two waves, in the first and last real column,
    a constant row, a larger value in the pad column: always the lowest real column; the mask fill, magnitude 1e4, a loss of 0"""
    z, labels, want = lc.ce_special()
    vp, v = lc.CE_SPECIAL["vp"], lc.CE_SPECIAL["v"]
    weight = None if gform == "bf16" else torch.tensor([lc.CE_WEIGHTS[r % 5] for r in range(z.shape[0])], dtype=F32)
    _ce_both_paths(z, labels, weight, v, vp + 4, vp + 4, gform, f"ce_rows ties and ranges g={gform}", slice_rel=None, want_argmax=want)


@gpu
def test_ce_rows_grid_stride():
    """more rows than the 65 536 workgroups of the grid: a workgroup takes a second row (and meets the loop's trailing barrier)"""
    z, labels, weight = lc.ce_stride()
    got = _ce_call(z, labels, weight, lc.CE_STRIDE["v"], 8, 8, "bf16", lc.CE_AUTO, "ce_rows grid stride")
    _ce_verify(got, z, labels, weight, lc.CE_STRIDE["v"], "bf16", "ce_rows grid stride", "NV=1, grid stride", slice_rel=None)


# ---- ce_addend, ce_finalize, ce_colsum, ce_scale, ce_cast ----------------------------------------------------------------------------
ADDEND_V = (1, 255, 256, 257)
ADDEND_STRIDE = (2048 * 256 + 5, 2048 * 256 + 8)


def _addend(v, vp, combo, seed):
    g = torch.Generator().manual_seed(seed)
    bias, priors = torch.randn(v, generator=g), torch.randn(v, generator=g) * 3
    mask = torch.tensor([0, 1, 255], dtype=torch.uint8)[torch.randint(0, 3, (v,), generator=g)]
    bias, priors, mask = (bias if combo & 1 else None), (priors if combo & 2 else None), (mask if combo & 4 else None)
    B, P, M = (None if bias is None else I(bias)), (None if priors is None else I(priors)), (None if mask is None else Ints(mask, 7))
    out = O(None, vp)
    what = f"ce_addend v={v} v_padded={vp} bias={bias is not None} priors={priors is not None} mask={mask is not None}"
    _ok(_lib().zett_op_ce_addend(_opt(B), _opt(P), _opt(M), v, vp, out.ptr(), d._stream()), what)
    tc.exact(out.back(what), lc.addend_ref(bias, priors, mask, v, vp), what, key=("ce_addend", f"combo {combo}"))


@gpu
@pytest.mark.parametrize("v", ADDEND_V)
def test_ce_addend(v):
    for vp in sorted({lc.up4(v), (v + 63) // 64 * 64}):
        for combo in range(8):
            _addend(v, vp, combo, 10 * v + combo)


@gpu
def test_ce_addend_grid_stride():
    _addend(ADDEND_STRIDE[0], ADDEND_STRIDE[1], 7, 3)


FINALIZE_N = (1, 255, 256, 257, 1000)


def _record_words(out, what):
    words = out.back(what, inside=False)
    return words, words.view(torch.int32)


@gpu
@pytest.mark.parametrize("n", FINALIZE_N)
def test_ce_finalize(n):
    """the record per word: weights NULL, real (0, -0.0 and a negative weight among them: w > 0 counts) and all zero"""
    g = torch.Generator().manual_seed(n)
    row_loss = torch.rand(n, generator=g) * 5
    labels = torch.randint(0, 50, (n,), generator=g, dtype=torch.int32)
    argmax = torch.where(torch.rand(n, generator=g) < 0.5, labels, labels + 1)
    real = torch.tensor([1.0, 0.0, -0.0, -0.5, 2.5])[torch.arange(n) % 5] * (torch.rand(n, generator=g) + 0.5)
    RL, LAB, AM = I(row_loss), Ints(labels, 2 ** 31 - 5), Ints(argmax, 2 ** 31 - 9)
    for name, w in (("null", None), ("real", real), ("zero", torch.where(torch.arange(n) % 2 == 0, 0.0, -0.0))):
        rl = row_loss if name != "zero" else torch.zeros(n)
        RLx, W = (RL if name != "zero" else I(rl)), (None if w is None else I(w))
        rec = O(None, 8)
        what = f"ce_finalize n={n} weights {name}"
        _ok(_lib().zett_op_ce_finalize(RLx.ptr(), _opt(W), LAB.ptr(), AM.ptr(), n, rec.ptr(), d._stream()), what)
        words, iw = _record_words(rec, what)
        vals, bnd, nc, nn = lc.ce_finalize_ref(rl, w, labels, argmax)
        if name == "zero":
            tc.exact(words, torch.zeros(8), what + ": the record of an all-zero weight", key=("ce_finalize", "all zero"))
            continue
        tc.check(words[:3], vals, bnd, what + " loss, sum w, 1 / sum w", key=("ce_finalize", f"weights {name}"))
        tc.exact(iw[3:5], torch.tensor([nc, nn], dtype=torch.int32), what + " n_correct, n_counted", key=("ce_finalize counts", f"weights {name}"))
        tc.exact(words[5:], torch.zeros(3), what + " words 5..7", key=("ce_finalize counts", f"weights {name}"))


COLSUM_ROWS = (0, 1, 3, 4, 5, 1000)
COLSUM_V = (1, 63, 64, 65, 130)


@gpu
@pytest.mark.parametrize("kind", ("f32", "bf16", "f16"))
def test_ce_colsum(kind):
    """the bias gradient over G in its three types; zero rows: out unchanged (accumulate) or zero.  (fp32 at 0 and 5 rows only: the
    row-primitive file walks the fp32 shapes through zett_op_colsum_f32, the same kernel)"""
    dt = lc.DT[kind]
    for rows in ((0, 5) if kind == "f32" else COLSUM_ROWS):
        for v in COLSUM_V:
            g = torch.Generator().manual_seed(rows * 131 + v)
            x, out0 = torch.randn(rows, v, generator=g).to(dt), torch.randn(v, generator=g)
            for ld in (v, v + 3):
                X = I(x if rows else torch.zeros(1, v, dtype=dt), ld)
                for acc in (0, 1):
                    out = O(None, v, values=out0)
                    what = f"ce_colsum {kind} [{rows}, {v}] ld={ld} accumulate={acc}"
                    _ok(_lib().zett_op_ce_colsum(X.ptr(), lc.DT_CODE[kind], ld, rows, v, out.ptr(), acc, d._stream()), what)
                    got = out.back(what)
                    if rows == 0:
                        tc.exact(got, out0 if acc else torch.zeros(v), what, key=(f"ce_colsum {kind}", "no rows"))
                    else:
                        ref, bnd = tc.colsum_ref(x.float(), out0 if acc else None)
                        tc.check(got, ref, bnd, what, key=(f"ce_colsum {kind}", f"accumulate {acc}"), slice_rel=tc.REL_SUM)


SCALE_N = (1, 3, 4, 5, 1027)
SCALE_STRIDE = 2 ** 21 + 1029


def _scale(kind, n, shift_in, shift_out, record2, seed, layout):
    x = torch.randn(n, generator=torch.Generator().manual_seed(seed))
    upstream = 1.7
    X = OnDev(tc.Frame(None, n, n, F32, NAN, shift=shift_in, values=x))
    REC, UP = I(torch.tensor([0.25, 3.0, record2, 0, 0, 0, 0, 0], dtype=F32)), I(torch.tensor([upstream], dtype=F32))
    out = O(None, n, dtype=lc.DT[kind], shift=shift_out)
    what = f"ce_scale {kind} n={n} in+{shift_in} out+{shift_out} record[2]={record2}"
    _ok(_lib().zett_op_ce_scale(X.ptr(), n, REC.ptr(), UP.ptr(), out.ptr(), lc.DT_CODE[kind], d._stream()), what)
    got = out.back(what)
    if record2 == 0:
        # The header promises a zero, not its sign: the f16 element path forms the product and the conversion in one fused
        # instruction with a +0 addend and gives +0 where the IEEE product of a negative input is -0 (seen on gfx950).
        tc.exact(got.abs(), torch.zeros(n, dtype=lc.DT[kind]), what + ": 1 / sum(w) = 0 must give an exactly zero output", key=(f"ce_scale {kind}", layout))
    else:
        tc.exact(got, lc.scale_ref(x, record2, upstream, lc.DT[kind]), what, key=(f"ce_scale {kind}", layout))


@gpu
@pytest.mark.parametrize("kind", ("f32", "bf16", "f16"))
def test_ce_scale(kind):
    for n in SCALE_N:
        for shift_in, shift_out, layout in ((0, 0, "vector"), (1, 0, "scalar, in shifted"), (0, 1, "scalar, out shifted")):
            _scale(kind, n, shift_in, shift_out, 0.0625 + 1e-3, n, layout)
        _scale(kind, n, 0, 0, 0.0, n, "vector, record[2] = 0")


@gpu
def test_ce_scale_grid_stride():
    _scale("bf16", SCALE_STRIDE, 0, 0, 0.37, 1, "vector, grid stride")


CAST_COLS = (1, 5, 64)
CAST_STRIDE = (32771, 65, 68)


@gpu
def test_ce_cast():
    """all nine pairs of types.  Same-type pairs go through float here too: values are kept, NaN payloads need not be — no NaN is fed"""
    for (ki, ko) in ((a, b) for a in lc.DT for b in lc.DT):
        for cols in CAST_COLS:
            x = (torch.randn(7, cols, generator=torch.Generator().manual_seed(cols)) * 4).to(lc.DT[ki])
            for cp, ld_in, ld_out in ((cols, cols + 1, cols + 2), (cols + 3, cols, cols + 3), (cols + 3, cols + 3, cols + 6)):
                X, out = I(x, ld_in), O(7, cp, ld_out, lc.DT[ko])
                what = f"ce_cast {ki} -> {ko} [7, {cols}] cols_padded={cp} ld_in={ld_in} ld_out={ld_out}"
                _ok(_lib().zett_op_ce_cast(X.ptr(), lc.DT_CODE[ki], ld_in, out.ptr(), lc.DT_CODE[ko], ld_out, 7, cols, cp, d._stream()), what)
                tc.exact(out.back(what), lc.cast_ref(x, cp, lc.DT[ko]), what, key=(f"ce_cast {ki} -> {ko}", "padded" if cp > cols else "tight"))


@gpu
def test_ce_cast_grid_stride():
    rows, cols, cp = CAST_STRIDE
    x = torch.randn(rows, cols, generator=torch.Generator().manual_seed(2))
    X, out = I(x, cols + 1), O(rows, cp, cp, torch.bfloat16)
    _ok(_lib().zett_op_ce_cast(X.ptr(), 0, cols + 1, out.ptr(), 2, cp, rows, cols, cp, d._stream()), "ce_cast grid stride")
    tc.exact(out.back("ce_cast grid stride"), lc.cast_ref(x, cp, torch.bfloat16), "ce_cast grid stride", key=("ce_cast f32 -> bf16", "grid stride"))


# ---- the distance losses ---------------------------------------------------------------------------------------------------------
RECORD1, UPSTREAM = 0.37, 1.7


def _dist_run(c, inp, what):
    lib, st = _lib(), d._stream()
    n, e, kind = inp["pred"].shape[0], inp["pred"].shape[1], c["kind"]
    SRC = I(inp["src"], c["ld_src"], shift=c["src_shift"])
    PRED = I(inp["pred"], c["ld_pred"], shift=c["pred_shift"])
    IDS = Ints(inp["ids"], 2 ** 45 if c["ids64"] else 10 ** 9)
    M = None if inp["mask"] is None else I(inp["mask"])
    code, ib = lc.DT_CODE[c["sd"]], 8 if c["ids64"] else 4
    src_rows = inp["src"].shape[0]
    dist, tnorm = O(None, n), O(None, n)
    _ok(lib.zett_op_embed_dist_rows(PRED.ptr(), c["ld_pred"], SRC.ptr(), code, c["ld_src"], src_rows, c["col0"], IDS.ptr(), ib, c["ids_stride"], _opt(M), n, e, kind, dist.ptr(),
                                    tnorm.ptr(), st), what)
    ref = lc.dist_rows_ref(inp["pred"], inp["tgt"], inp["mask"], kind, lc.dist_vec_ok(c, False))
    layout = f"kind {kind}, {c['sd']}, {'vector' if lc.dist_vec_ok(c, False) else 'scalar'}"
    tc.check(dist.back(what + " row_dist"), ref["dist"], ref["b_dist"], what + " row_dist", key=("embed_dist_rows row_dist", layout), slice_rel=lc.REL_LOSS)
    tc.check(tnorm.back(what + " row_tnorm"), ref["tnorm"], ref["b_tnorm"], what + " row_tnorm", key=("embed_dist_rows row_tnorm", layout), slice_rel=lc.REL_LOSS)

    rd = ref["dist"].float()
    RD, REC, UP = I(rd), I(torch.tensor([0.5, RECORD1, 0.25, 0.0], dtype=F32)), I(torch.tensor([UPSTREAM], dtype=F32))
    val, bnd = lc.dist_grad_ref(inp["pred"], inp["tgt"], inp["mask"], rd, kind, RECORD1, UPSTREAM)
    layout = f"kind {kind}, {c['sd']}, {'vector' if lc.dist_vec_ok(c, True) else 'scalar'}"
    before = torch.randn(n, e, generator=torch.Generator().manual_seed(c["i"])) * 1e-2
    plain = None
    for acc in (0, 1):
        dp = O(n, e, c["ld_dpred"], values=before if acc else None, shift=c["dpred_shift"])
        name = f"{what} dpred accumulate={acc}"
        _ok(lib.zett_op_embed_dist_grad(PRED.ptr(), c["ld_pred"], SRC.ptr(), code, c["ld_src"], src_rows, c["col0"], IDS.ptr(), ib, c["ids_stride"], _opt(M), RD.ptr(), n, e, kind,
                                        REC.ptr(), UP.ptr(), dp.ptr(), c["ld_dpred"], acc, st), name)
        got = dp.back(name)
        if acc == 0:
            plain = got
            tc.check(got, val, bnd, name, key=("embed_dist_grad", layout), slice_rel=lc.REL_DIST_GRAD)
            if kind == lc.RMSE and n > 1 and bool((inp["pred"][1] == inp["tgt"][1]).all()):
                tc.exact(got[1], torch.zeros(e), name + ": the RMSE gradient of a row equal to its target", key=("embed_dist_grad zero row", layout))
        else:
            tc.exact(got, before + plain, name + ": before + what a plain call writes, one fp32 addition", key=("embed_dist_grad accumulate", layout))


@gpu
@pytest.mark.parametrize("c", lc.dist_cases(), ids=lambda c: f"e{c['e']}-k{c['kind']}-{c['sd']}-{c['switch']}")
def test_embed_dist_rows_and_grad(c):
    """every element of row_dist, row_tnorm and dpred: every kind and source type, the 4-element accesses on and switched off by each
    of their conditions alone, int32 / int64 ids that are clamped (never an address), every mask"""
    inp = lc.dist_inputs(c)
    _dist_run(c, inp, f"embed_dist e={c['e']} n={c['n']} kind={c['kind']} {c['sd']} {c['switch']} ids{'64' if c['ids64'] else '32'} stride {c['ids_stride']} mask={c['mask']}")


@gpu
def test_embed_dist_grid_stride():
    """more rows than four times the 2048 workgroups: the grid-stride loop of both kernels runs"""
    n, e = lc.DIST_STRIDE["n"], lc.DIST_STRIDE["e"]
    c = dict(i=999, e=e, kind=lc.MSE, sd="bf16", switch="none", n=n, ids64=False, ids_stride=1, mask="real", col0=4, pred_shift=0, ld_pred=e + 4, src_shift=0, dpred_shift=0,
             ld_dpred=e, ld_src=16)
    g = torch.Generator().manual_seed(8)
    src = torch.full((37, 16), NAN, dtype=torch.bfloat16)
    block = (torch.randn(37, e, generator=g) * 0.05).to(torch.bfloat16)
    src[:, 4:4 + e] = block
    ids = torch.randint(-3, 41, (n, 1), generator=g, dtype=torch.int32)
    tgt = block.float()[lc.clamp_rows(ids[:, 0], 37)]
    inp = dict(src=src, ids=ids, pred=tgt + 1.5e-3 * torch.randn(n, e, generator=g), mask=torch.where(torch.arange(n) % 3 == 0, 0.5, 2.0).float(), tgt=tgt)
    _dist_run(c, inp, "embed_dist grid stride")


@gpu
@pytest.mark.parametrize("n", FINALIZE_N)
def test_embed_dist_finalize(n):
    g = torch.Generator().manual_seed(n)
    rd, rt = torch.rand(n, generator=g), torch.rand(n, generator=g) + 0.5
    RD, RT = I(rd), I(rt)
    for mode in (lc.MEAN, lc.LEXICAL):
        for name, mask in (("null", None), ("partial", (torch.arange(n) % 3 != 0).float()), ("zero", torch.zeros(n))):
            M = None if mask is None else I(mask)
            rec = O(None, 4)
            what = f"embed_dist_finalize n={n} mode={mode} mask {name}"
            _ok(_lib().zett_op_embed_dist_finalize(RD.ptr(), RT.ptr(), _opt(M), n, mode, rec.ptr(), d._stream()), what)
            vals, bnd = lc.dist_finalize_ref(rd, rt, mask, mode)
            tc.check(rec.back(what), vals, bnd, what, key=("embed_dist_finalize", f"mode {mode}, mask {name}"))


MASK_STRIDE = 2048 * 256 + 300


def _token_mask(n, width, ld, ids64, seed):
    idt = torch.int64 if ids64 else torch.int32
    pad = 3
    g = torch.Generator().manual_seed(seed)
    ids = torch.full((n, ld), 10 ** 9, dtype=idt)
    ids[:, :width] = torch.randint(2, 5, (n, width), generator=g).to(idt)
    ids[::2, 0] = pad                                  # the pad id also occurs in column 0, which does not count
    out = O(None, n)
    what = f"single_token_mask n={n} width={width} ld={ld} ids{'64' if ids64 else '32'}"
    IDS = Ints(ids, pad)                               # (a row read from the slack would look like a single token)
    _ok(_lib().zett_op_single_token_mask(IDS.ptr(), 8 if ids64 else 4, n, width, ld, pad, out.ptr(), d._stream()), what)
    tc.exact(out.back(what), lc.single_token_mask_ref(ids, width, pad), what, key=("single_token_mask", f"width {width}"))


@gpu
def test_single_token_mask():
    for width in (1, 2, 5):
        for ld in (width, width + 2):
            for ids64 in (False, True):
                _token_mask(40, width, ld, ids64, width + ld)
    _token_mask(MASK_STRIDE, 2, 2, False, 1)


# ---- zett_op_grad_norm / zett_op_adamw ---------------------------------------------------------------------------------------------
HYPER = dict(lr=1e-2, b1=0.9, b2=0.999, eps=1e-8, wd=0.01)


def _arr(ctype, values):
    return (ctype * max(1, len(values)))(*values)


def _mt_buffers():
    """-> per tensor of lc.mt_list() the four framed device buffers (p, g, m, v), each a canary-framed vector moved `off` elements
    into its allocation, and their host values"""
    entries = lc.mt_list()
    bufs, host = [], []
    for i, en in enumerate(entries):
        vals = [lc.mt_values(en, i, w) for w in range(4)]
        host.append(vals)
        bufs.append([O(None, en["n"], values=vals[w], shift=en["off"][w]) for w in range(4)])
    return entries, bufs, host


def _record_in(coef, skip, step, b1, b2):
    rec = torch.zeros(8, dtype=F32)
    rec[0], rec[1] = 1.0, coef
    rec.view(torch.int32)[2], rec.view(torch.int32)[3] = skip, step
    rec[4], rec[5] = 1.0 - b1 ** step, 1.0 - b2 ** step
    return rec


def _grad_norm(grads, offsets, ptrs, max_norm, step0, what, key, slots=16):
    """one call; the partials at their documented places, the slots beyond them canary, the record per word -> the record's reference"""
    k = len(grads)
    total = sum(lc.mt_items(g.shape[0]) for g in grads)
    seed = torch.zeros(8, dtype=F32)
    seed.view(torch.int32)[3] = step0
    seed[6], seed[7] = 5.0, 6.0                       # (words 6, 7 are written as zeros)
    rec, parts = O(None, 8, values=seed), O(None, total + slots)
    _ok(_lib().zett_op_grad_norm(_arr(C.c_void_p, ptrs), _arr(C.c_int64, [g.shape[0] for g in grads]), k, max_norm, HYPER["b1"], HYPER["b2"], parts.ptr(), total + slots, rec.ptr(),
                                 d._stream()), what)
    got = parts.back(what + " partials", inside=False)
    tc.exact(got[total:].view(torch.int32), torch.full((slots,), tc.CANARY_BITS, dtype=torch.int32), what + ": the slots of partials beyond the work items", key=(key[0] + " partials", "beyond total"))
    ref, bnd = lc.partials_ref(grads, offsets)
    finite = torch.isfinite(ref) & (ref <= float(torch.finfo(F32).max))          # (a square that overflows fp32 is an inf partial)
    if total and bool(finite.all()):
        tc.check(got[:total], ref, bnd, what + " partials", key=(key[0] + " partials", key[1]), slice_rel=lc.REL_LOSS)
    else:
        assert not bool(torch.isfinite(got[:total][~finite]).any()), what + ": a partial over an inf, a NaN or an overflowing square is finite"
    words, iw = _record_words(rec, what + " record")
    want = lc.norm_record_ref(got[:total], max_norm, HYPER["b1"], HYPER["b2"], step0)
    tc.exact(iw[2:4], torch.tensor([want["skip"], want["step"]], dtype=torch.int32), what + " skip, step", key=(key[0] + " skip, step", key[1]))
    tc.exact(words[6:], torch.zeros(2), what + " words 6, 7", key=(key[0] + " skip, step", key[1]))
    names = ("coef", "c1", "c2") if want["skip"] else ("norm", "coef", "c1", "c2")
    idx = dict(norm=0, coef=1, c1=4, c2=5)
    tc.check(torch.stack([words[idx[nm]] for nm in names]), torch.stack([want[nm][0] for nm in names]), torch.stack([torch.as_tensor(want[nm][1], dtype=F64) for nm in names]),
             what + " " + ", ".join(names), key=(key[0] + " record", key[1]))
    if want["skip"]:
        assert not bool(torch.isfinite(words[0])), what + ": skip is set but the norm is finite"
    return want, words


@gpu
@pytest.mark.parametrize("k", lc.MT_PREFIXES)
def test_grad_norm_over_the_tensor_list(k):
    """the first k tensors of the 130: every chunk's partial at partial_base + item in list order with the empty tensors skipped,
    across the 64-tensor launch boundary; then norm, coef, skip, step and the bias corrections"""
    entries, bufs, host = _mt_buffers()
    grads = [host[i][1] for i in range(k)]
    ptrs = [None if (entries[i]["n"] == 0 and i % 2 == 0) else bufs[i][1].ptr() for i in range(k)]
    step0 = (0, 1, 999)[lc.MT_PREFIXES.index(k) % 3]
    if k == 0:
        seed = torch.zeros(8, dtype=F32)
        seed.view(torch.int32)[3] = step0
        rec = O(None, 8, values=seed)
        _ok(_lib().zett_op_grad_norm(NULL, NULL, 0, 1.0, HYPER["b1"], HYPER["b2"], NULL, 0, rec.ptr(), d._stream()), "grad_norm of no tensors, partials NULL")
        words, iw = _record_words(rec, "grad_norm of no tensors")
        tc.exact(words[:2], torch.tensor([0.0, 1.0]), "grad_norm of no tensors: norm 0, coef 1", key=("grad_norm record", "no tensors"))
        tc.exact(iw[2:4], torch.tensor([0, step0 + 1], dtype=torch.int32), "grad_norm of no tensors: skip, step", key=("grad_norm skip, step", "no tensors"))
        return
    for max_norm in (1e6, 0.5):                         # norm < max_norm (coef exactly 1) and norm > max_norm
        want, _ = _grad_norm(grads, [entries[i]["off"][1] for i in range(k)], ptrs, max_norm, step0, f"grad_norm k={k} max_norm={max_norm} step0={step0}", ("grad_norm", f"k={k}"))
        assert k == 1 or (float(want["norm"][0]) < max_norm) == (max_norm == 1e6)          # (k = 1 is the empty first tensor alone: norm 0)
    for i in range(k):
        lc.unchanged(bufs[i][1].buf.cpu(), bufs[i][1].f.buf, f"grad_norm k={k}: gradient {i}")


@gpu
def test_grad_norm_at_the_clip_threshold_and_not_finite():
    """sum of the partials == max_norm^2 exactly (3, 4 -> 25; 5.0): the kernel's `norm < max_norm` is false and coef = 5 / 5, which IS 1.0
    — `<` and `<=` give the same bits there, so what is pinned is coef == 1.0 exactly on both sides of equality.  One inf, one NaN and
    one overflow of g * g: skip = 1, the step count unchanged, coef 0"""
    def one(values, max_norm, step0, what):
        G = O(None, len(values), values=torch.tensor(values, dtype=F32))
        return _grad_norm([torch.tensor(values, dtype=F32)], [0], [G.ptr()], max_norm, step0, what, ("grad_norm", what), slots=4)

    want, words = one([3.0, 4.0, 0.0], 5.0, 7, "norm == max_norm")
    tc.exact(words[:2], torch.tensor([5.0, 1.0]), "grad_norm at norm == max_norm", key=("grad_norm record", "norm == max_norm"))
    for name, bad in (("inf", float("inf")), ("nan", NAN), ("overflow", 1e20)):
        want, words = one([1.0, bad, 2.0, 0.5, 0.25], 1.0, 4, name)
        assert want["skip"] == 1 and want["step"] == 4
        tc.exact(words[1:2], torch.zeros(1), f"grad_norm {name}: coef", key=("grad_norm record", name))


def _adamw(k, zero_grad, step, coef, skip, what):
    entries, bufs, host = _mt_buffers()
    rec = _record_in(coef, skip, step, HYPER["b1"], HYPER["b2"])
    REC = I(rec)
    arrs = [_arr(C.c_void_p, [None if (entries[i]["null"] and w != 1) or (entries[i]["n"] == 0 and i % 2 == 0) else bufs[i][w].ptr() for i in range(k)]) for w in range(4)]
    _ok(_lib().zett_op_adamw(arrs[0], arrs[1], arrs[2], arrs[3], _arr(C.c_int64, [en["n"] for en in entries[:k]]), _arr(C.c_uint8, [en["flags"] for en in entries[:k]]), k,
                             HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], HYPER["wd"], zero_grad, REC.ptr(), d._stream()), what)
    h = lc.adam_hyper(**HYPER)
    for i, en in enumerate(entries):
        n = en["n"]
        got = [bufs[i][w].back(f"{what} tensor {i} {'pgmv'[w]}") for w in range(4)]
        name = f"{what} tensor {i} (n={n}, offsets {en['off']}, flags {en['flags']})"
        layout = "vector" if all(o % 4 == 0 for o in en["off"]) else "scalar"
        touched = i < k and not skip and not (en["flags"] & lc.FROZEN)
        cleared = i < k and zero_grad
        tc.exact(got[1], torch.zeros(n) if cleared else host[i][1], name + (": the gradient is cleared" if cleared else ": the gradient is unchanged"), key=("adamw gradient", layout))
        if not touched:
            for w in (0, 2, 3):
                tc.exact(got[w], host[i][w], name + f": {'pgmv'[w]} of a frozen, skipped or unlisted tensor is untouched", key=("adamw untouched", layout))
            continue
        if n == 0:
            continue
        ref = lc.adamw_ref(host[i][0], host[i][1], host[i][2], host[i][3], h, float(rec[1]), float(rec[4]), float(rec[5]), bool(en["flags"] & lc.DECAY))
        for w, nm in ((0, "p"), (2, "m"), (3, "v")):
            tc.check(got[w], ref[nm], ref["b_" + nm], f"{name} {nm}", key=(f"adamw {nm}", layout))
        tc.check(got[0] - host[i][0], ref["p"] - host[i][0].double(), ref["b_p"] + tc.U * host[i][0].double().abs(), name + " displacement", key=("adamw displacement", layout), slice_rel=lc.REL_ADAMW)


@gpu
@pytest.mark.parametrize("k", lc.MT_PREFIXES)
def test_adamw_over_the_tensor_list(k):
    """the first k tensors of the 130 updated from a record this test writes: every element of p, m, v; gradients bit-unchanged or all
    zero bits; frozen tensors and the tensors beyond k untouched; step-1 and step-1000 corrections, clipped and unclipped"""
    j = lc.MT_PREFIXES.index(k)
    _adamw(k, zero_grad=j % 2, step=(1, 1000)[j % 2], coef=(1.0, 0.3125)[(j // 2) % 2], skip=0, what=f"adamw k={k}")


@gpu
@pytest.mark.parametrize("zero_grad", (0, 1))
def test_adamw_skipped_step(zero_grad):
    _adamw(65, zero_grad=zero_grad, step=3, coef=0.0, skip=1, what=f"adamw skipped zero_grad={zero_grad}")


def _tiled(pattern, n, fill_bits):
    """[256 | n | 256] floats on the device: the pattern repeated, the slack a bit pattern"""
    buf = torch.empty(n + 512, dtype=F32, device=DEV)
    buf.view(torch.int32)[:256] = fill_bits
    buf.view(torch.int32)[256 + n:] = fill_bits
    L = pattern.shape[0]
    buf[256:256 + n] = pattern.to(DEV).repeat(n // L + 1)[:n]
    return buf


def _slack_intact(buf, n, fill_bits, what):
    bits = buf.view(torch.int32)
    assert bool((bits[:256] == fill_bits).all()) and bool((bits[256 + n:] == fill_bits).all()), f"{what}: the slack around the buffer changed"


def _tiled_check(buf, n, ref, bnd, what):
    """the elements against the tiled float64 reference, on the device"""
    L = ref.shape[0]
    ref, bnd = ref.to(DEV), bnd.to(DEV)
    body = buf[256:256 + n]
    worst = 0.0
    tiles = n // L
    for t0 in range(0, tiles + 1, 512):
        t1 = min(t0 + 512, tiles)
        parts = [(body[t0 * L:t1 * L].view(t1 - t0, L), ref[None], bnd[None])] if t1 > t0 else []
        if t1 == tiles and n > tiles * L:
            parts.append((body[tiles * L:], ref[:n - tiles * L], bnd[:n - tiles * L]))
        for got, r, b in parts:
            err = (got.double() - r).abs()
            err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
            worst = max(worst, float((err / b).max()))
    print(f"{what}: largest err / bound {worst:.3f}")
    assert worst <= 1.0, f"{what}: largest err / bound {worst:.3f}"
    tc._note((what, "item stride"), worst, 0.0)


@gpu
def test_grad_norm_item_stride():
    """one tensor of more chunks than the 2048 workgroups: a workgroup takes a second work item.  The gradient is a pattern of 65 537
    elements repeated (65 536 = -1 mod 65 537: every chunk starts at another phase); each partial against float64 from the pattern"""
    n, L = lc.MT_STRIDE_N, lc.MT_PATTERN
    pat = torch.randn(L, generator=torch.Generator().manual_seed(1)) * 0.1
    G = _tiled(pat, n, 0x7FC00000)
    items = lc.mt_items(n)
    sq = pat.double() ** 2
    cs = torch.cat([torch.zeros(1, dtype=F64), torch.cat([sq, sq]).cumsum(0)])
    starts = (torch.arange(items) * lc.MT_CHUNK) % L
    lens = torch.full((items,), lc.MT_CHUNK)
    lens[-1] = n - (items - 1) * lc.MT_CHUNK
    ref = cs[starts + lens] - cs[starts]
    rec, parts = O(None, 8, values=torch.zeros(8)), O(None, items + 16)
    _ok(_lib().zett_op_grad_norm(_arr(C.c_void_p, [G.data_ptr() + 1024]), _arr(C.c_int64, [n]), 1, 1.0, 0.9, 0.999, parts.ptr(), items + 16, rec.ptr(), d._stream()), "grad_norm item stride")
    got = parts.back("grad_norm item stride partials", inside=False)
    _slack_intact(G, n, 0x7FC00000, "grad_norm item stride")
    tc.exact(got[items:].view(torch.int32), torch.full((16,), tc.CANARY_BITS, dtype=torch.int32), "grad_norm item stride: beyond the work items")
    tc.check(got[:items], ref, (lc.sumsq_depth(True) + 3) * tc.U * ref + lc.TINY, "grad_norm item stride partials", key=("grad_norm partials", "item stride"), slice_rel=lc.REL_LOSS)
    words, iw = _record_words(rec, "grad_norm item stride record")
    want = lc.norm_record_ref(got[:items], 1.0, 0.9, 0.999, 0)
    tc.check(words[:2], torch.stack([want["norm"][0], want["coef"][0]]), torch.stack([want["norm"][1], want["coef"][1]]), "grad_norm item stride norm, coef", key=("grad_norm record", "item stride"))
    tc.exact(iw[2:4], torch.tensor([0, 1], dtype=torch.int32), "grad_norm item stride skip, step")


@gpu
def test_adamw_item_stride():
    """the same length through adamw_kernel: p, g, m, v are patterns of 65 537 elements repeated, the float64 reference is computed on
    the pattern and compared, tiled, on the device; the gradient is cleared in the same pass"""
    n, L = lc.MT_STRIDE_N, lc.MT_PATTERN
    g = torch.Generator().manual_seed(2)
    pats = [torch.randn(L, generator=g) * 0.5, torch.randn(L, generator=g) * 0.1, torch.randn(L, generator=g) * 0.05, torch.rand(L, generator=g) * 0.01]
    bufs = [_tiled(p, n, tc.CANARY_BITS) for p in pats]
    rec = _record_in(0.3125, 0, 10, HYPER["b1"], HYPER["b2"])
    REC = I(rec)
    arrs = [_arr(C.c_void_p, [b.data_ptr() + 1024]) for b in bufs]
    _ok(_lib().zett_op_adamw(arrs[0], arrs[1], arrs[2], arrs[3], _arr(C.c_int64, [n]), _arr(C.c_uint8, [lc.DECAY]), 1, HYPER["lr"], HYPER["b1"], HYPER["b2"], HYPER["eps"], HYPER["wd"], 1,
                             REC.ptr(), d._stream()), "adamw item stride")
    torch.cuda.synchronize()
    ref = lc.adamw_ref(pats[0], pats[1], pats[2], pats[3], lc.adam_hyper(**HYPER), float(rec[1]), float(rec[4]), float(rec[5]), True)
    for b in bufs:
        _slack_intact(b, n, tc.CANARY_BITS, "adamw item stride")
    for w, nm in ((0, "p"), (2, "m"), (3, "v")):
        _tiled_check(bufs[w], n, ref[nm], ref["b_" + nm], f"adamw {nm}")
    assert bool((bufs[1][256:256 + n].view(torch.int32) == 0).all()), "adamw item stride: the gradient is not all zero bits"
