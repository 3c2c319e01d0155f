"""zett_op_gemm_f32 / zett_op_gemm_lo called directly through the C ABI and checked ELEMENT BY ELEMENT against float64 on the
same rounded operands (tests/gemm_check.py), at the shapes where the three tiles start, end and hand over to each other.

Buffers: every operand, bias, residual and output is a view INSIDE a larger allocation of this test (gemm_check.Framed) with a
full tile of slack — 256 rows of the leading dimension, 256 elements for a vector — in front of and behind it.  The slack of what
a kernel reads is NaN (rows >= m and >= n, the columns k .. ld - 1), the slack of the output is a canary bit pattern (the columns
n .. ld_out - 1 of every row and the rows past m included): a kernel that indexes a whole tile too far still touches only this
test's memory, a value fetched from outside the operands poisons the result, and a store outside [m, n] breaks the canary.
Nothing here is meant to fault.

The GEMM log does not exist on these entry points, so the tile a call runs on is not observed: expected_tile below restates the
dispatch rule, and the tests use it to prove that their cases reach all four code paths and to file the measured margins.
"""
import ctypes as C
import os

import pytest
import torch

from tests import gemm_check as gc

DEV = "cuda:0"
gpu = pytest.mark.gpu
KINDS = ("f32", "bf16", "f16")

T128, TREG, TLDS, TLDS_GENERIC = "128x128", "256x256 register-staged", "256x256 direct-to-LDS, streamlined epilogue", "256x256 direct-to-LDS, generic drain"


def expected_tile(kind, m, n, k, act, has_res, ld_out, ld_res, out_align=16, res_align=16, bias_align=16):
    """The tile a call takes.  Mirrors, line for line,

        zett_amd/csrc/train_gemm.hip gemm_wide_ok:      n % 8 == 0 && ld_out % 4 == 0 && (!residual || ld_res % 4 == 0)
                                                        && out, residual, bias 16-byte aligned
                                     gemm_tile_for:     fp32:   variant = (m > 128 && n > 128 && wide_ok) ? 2 : 1
                                                        16-bit: variant = (m > 128 && n > 128 && wide_ok) ? (k >= 512 ? 7 : 2) : 1
        zett_amd/csrc/gemm4d.hip.h   gemm4d_epi_mode:   fp32 output, no scale / shift: G4D_EPI_F32 (streamlined) for
                                                        act == none, or tanh-GELU WITH a residual; G4D_EPI_GENERIC otherwise
    (variant 1 = 128x128, 2 = gemm8r, 7 = gemm4d)."""
    wide_ok = n % 8 == 0 and ld_out % 4 == 0 and (not has_res or ld_res % 4 == 0) and out_align % 16 == 0 and res_align % 16 == 0 and bias_align % 16 == 0
    if not (m > 128 and n > 128 and wide_ok):
        return T128
    if kind == "f32" or k < 512:
        return TREG
    return TLDS if act == 0 or (act == 1 and has_res) else TLDS_GENERIC


MS = (1, 127, 128, 129, 255, 256, 257, 300, 513)
NS = (8, 64, 120, 128, 129, 136, 256, 257, 264, 520)
KS = {"f32": (32, 96, 480, 544), "bf16": (64, 448, 512, 576, 2112), "f16": (64, 448, 512, 576, 2112)}
EPILOGUE_SHAPES = ((129, 136, 64), (257, 264, 448), (257, 264, 576), (300, 257, 576), (100, 264, 576), (513, 520, 2112))
EPILOGUES = tuple((act, b, r) for act in (0, 1, 2) for b in (False, True) for r in (False, True))


def test_the_cases_reach_every_tile_and_drain():
    """(no GPU) shape -> expected tile of the cases below: all four paths, in each 16-bit type; both fp32 tiles"""
    sweep = {kind: {expected_tile(kind, m, n, k, 0, True, n + 4, n + 8) for k in KS[kind] for m in MS for n in NS} for kind in KINDS}
    epi = {kind: {expected_tile(kind, m, n, k, act, r, n, n) for m, n, k in EPILOGUE_SHAPES for act, _, r in EPILOGUES} for kind in KINDS}
    assert sweep["f32"] == epi["f32"] == {T128, TREG}
    for kind in ("bf16", "f16"):
        assert sweep[kind] == {T128, TREG, TLDS}
        assert epi[kind] == {T128, TREG, TLDS, TLDS_GENERIC}
    table = {(m, n, k, act, r): expected_tile("bf16", m, n, k, act, r, n, n) for m, n, k in EPILOGUE_SHAPES for act, _, r in EPILOGUES}
    assert table[129, 136, 64, 0, False] == TREG and table[257, 264, 448, 2, True] == TREG
    assert table[300, 257, 576, 0, True] == T128 and table[100, 264, 576, 1, True] == T128          # n % 8, m <= 128
    assert table[257, 264, 576, 0, False] == table[257, 264, 576, 0, True] == table[513, 520, 2112, 1, True] == TLDS
    assert table[257, 264, 576, 1, False] == table[257, 264, 576, 2, False] == table[513, 520, 2112, 2, True] == TLDS_GENERIC
    # the cut-overs of the sweep: m <= 128 and n <= 128, n % 8, K = 512
    assert expected_tile("f16", 128, 136, 512, 0, True, 140, 144) == T128 and expected_tile("f16", 129, 136, 512, 0, True, 140, 144) == TLDS
    assert expected_tile("f16", 129, 128, 512, 0, True, 132, 136) == T128 and expected_tile("f16", 129, 129, 512, 0, True, 133, 137) == T128
    assert expected_tile("f16", 129, 136, 448, 0, True, 140, 144) == TREG
    # unaligned leading dimensions and bases fall back
    assert expected_tile("f16", 257, 264, 576, 0, True, 267, 272) == T128 and expected_tile("f16", 257, 264, 576, 0, True, 268, 265) == T128
    assert expected_tile("f16", 257, 264, 576, 0, True, 268, 272, out_align=4) == T128
    assert expected_tile("f16", 257, 264, 576, 0, True, 268, 272, res_align=4) == T128
    assert expected_tile("f16", 257, 264, 576, 0, True, 268, 272, bias_align=4) == T128


# ---- plumbing ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = os.environ.get("ZETT_GEMM_CHECK_RECORD")          # figures for profiles/gemm_direct_check.md
    if path and gc.RECORD:
        gc.write_record(path)


def _lib():
    from zett_amd import _lib
    return _lib, _lib.load()


class OnDev:
    """a gemm_check.Framed and its copy on the device"""

    def __init__(self, frame):
        self.f = frame
        self.buf = frame.buf.to(DEV)
        assert self.buf.data_ptr() % 256 == 0

    def ptr(self, col0=0, byte_shift=0):
        return C.c_void_p(self.buf.data_ptr() + self.f.byte_offset() + col0 * self.buf.element_size() + byte_shift)


def _nan_matrix(values, ld, dtype):
    rows, cols = values.shape
    return OnDev(gc.Framed(rows, cols, ld, dtype, float("nan"), values=values))


def _nan_vector(values, shift=0):
    return OnDev(gc.Framed(None, values.shape[0], values.shape[0], torch.float32, float("nan"), shift=shift, values=values))


def _raw(kind, a, lda, w, ldw, m, n, k, bias, act, res, ld_res, out, ld_out):
    """the entry point of `kind` on raw pointers -> its return code"""
    L, lib = _lib()
    null = C.c_void_p(0)
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    if kind == "f32":
        return lib.zett_op_gemm_f32(a, lda, w, ldw, m, n, k, bias or null, act, res or null, ld_res, out, ld_out, st)
    return lib.zett_op_gemm_lo(L.PREC_BF16 if kind == "bf16" else L.PREC_F16, a, lda, w, ldw, m, n, k, bias or null, act, res or null, ld_res, out, ld_out, st)


def _run(kind, A, W, m, n, k, bias=None, act=0, res=None, ld_out=None, out_shift=0, a_col0=0, w_col0=0, what=""):
    """One call on framed buffers -> the [m, n] result on the host, after the canary check.  A, W: OnDev matrices (m and n rows);
    bias: OnDev vector; res: OnDev [m, n] matrix with its own leading dimension."""
    ld_out = n if ld_out is None else ld_out
    out = OnDev(gc.Framed(m, n, ld_out, torch.float32, "canary", shift=out_shift))
    rc = _raw(kind, A.ptr(a_col0), A.f.ld, W.ptr(w_col0), W.f.ld, m, n, k, bias and bias.ptr(), act, res and res.ptr(), res.f.ld if res else 0, out.ptr(), ld_out)
    if rc != 0:
        raise AssertionError(f"{what}: return code {rc}: {_lib()[1].zett_last_error().decode()}")
    torch.cuda.synchronize()
    back = out.buf.cpu()
    gc.check_canary(out.f, back, what)
    return out.f.view(back).clone()


_OPERANDS = {}


def _operands(kind, k):
    """a [513, k], w [520, k], bias [520], residual [513, 520] and their float64 reference — made once per (type, K); every smaller
    case takes leading rows of them, and its reference is the leading block of this one"""
    if (kind, k) not in _OPERANDS:
        if len(_OPERANDS) > 3:
            _OPERANDS.clear()
        a, w, bias, res = gc.operands(kind, 513, 520, k, seed=7 * k + KINDS.index(kind))
        _OPERANDS[kind, k] = (a, w, bias, res, {})
    return _OPERANDS[kind, k]


def _reference(kind, k, m, n, has_bias, act, has_res):
    a, w, bias, res, refs = _operands(kind, k)
    key = (has_bias, act, has_res)
    if key not in refs:
        if "products" not in refs:
            refs["products"] = gc.products(a, w)
        refs[key] = gc.reference(a, w, bias if has_bias else None, act, res if has_res else None, prod=refs["products"])
    return gc.sub_reference(refs[key], m, n)


# ---- the tile edges ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind,k", [(kind, k) for kind in KINDS for k in KS[kind]])
def test_every_tile_edge(kind, k):
    """M x N over the sizes at which a tile is one row or column short of, exactly at, and one past its edge (128, 256), the
    cut-over to the 128 tile (m <= 128, n <= 128, n % 8), two and three tiles per side; bias and residual given, the output
    with four canary columns behind every row and the residual with its own leading dimension."""
    a, w, bias, res, _ = _operands(kind, k)
    dt = gc.LO_DTYPES[kind]
    Ws = {n: _nan_matrix(w[:n], k, dt) for n in NS}
    Bs = {n: _nan_vector(bias[:n]) for n in NS}
    for m in MS:
        A = _nan_matrix(a[:m], k, dt)
        for n in NS:
            R = _nan_matrix(res[:m, :n], n + 8, torch.float32)
            what = f"{kind} [{m}, {n}] k={k}"
            got = _run(kind, A, Ws[n], m, n, k, Bs[n], 0, R, ld_out=n + 4, what=what)
            gc.check(got, _reference(kind, k, m, n, True, 0, True), k, 0, what, key=(kind, k, expected_tile(kind, m, n, k, 0, True, n + 4, n + 8)))


@gpu
@pytest.mark.parametrize("m,n,k", EPILOGUE_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_every_epilogue(kind, m, n, k):
    """act {none, tanh-GELU, erf-GELU} x bias {none, given} x residual {none, given}: on the direct-to-LDS tile the streamlined
    epilogue (no activation with and without a residual, tanh + residual) and the generic drain (tanh alone, erf)"""
    a, w, bias, res, _ = _operands(kind, k)
    dt = gc.LO_DTYPES[kind]
    A, W, B, R = _nan_matrix(a[:m], k, dt), _nan_matrix(w[:n], k, dt), _nan_vector(bias[:n]), _nan_matrix(res[:m, :n], n, torch.float32)
    for act, has_b, has_r in EPILOGUES:
        what = f"{kind} [{m}, {n}] k={k} act={act} bias={has_b} residual={has_r}"
        got = _run(kind, A, W, m, n, k, B if has_b else None, act, R if has_r else None, what=what)
        gc.check(got, _reference(kind, k, m, n, has_b, act, has_r), k, act, what, key=(kind, k, expected_tile(kind, m, n, k, act, has_r, n, n)))


@gpu
@pytest.mark.parametrize("m,n,k", EPILOGUE_SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_leading_dimensions(kind, m, n, k):
    """lda = k + 64 and ldw = k + 128 (different from each other), ld_out in {n, n + 4, n + 3}, ld_res in {n, n + 8, n + 1} with
    ld_res != ld_out (n + 3 and n + 1: the 128 tile), and operands that are column slices [:, c0 : c0 + k] of a wider matrix
    whose neighbouring columns hold finite non-zero values, as Ops.wgrad passes them"""
    a, w, bias, res, _ = _operands(kind, k)
    dt = gc.LO_DTYPES[kind]
    A, W, B = _nan_matrix(a[:m], k + 64, dt), _nan_matrix(w[:n], k + 128, dt), _nan_vector(bias[:n])
    g = torch.Generator().manual_seed(k + m)
    wide_a = (torch.randn(m, k + 192, generator=g) + 3.0).to(dt)
    wide_a[:, 64:64 + k] = a[:m]
    wide_w = (torch.randn(n, k + 256, generator=g) - 3.0).to(dt)
    wide_w[:, 128:128 + k] = w[:n]
    SA, SW = _nan_matrix(wide_a, k + 192, dt), _nan_matrix(wide_w, k + 256, dt)
    Rs = {ld: _nan_matrix(res[:m, :n], ld, torch.float32) for ld in (n, n + 8, n + 1)}
    pairs = [(lo, lr) for lo in (n, n + 4, n + 3) for lr in (n, n + 8, n + 1) if lo != lr]
    for i, (ld_out, ld_res) in enumerate(pairs):
        act = i % 3
        ref = _reference(kind, k, m, n, True, act, True)
        key = (kind, k, expected_tile(kind, m, n, k, act, True, ld_out, ld_res))
        what = f"{kind} [{m}, {n}] k={k} act={act} lda={k + 64} ldw={k + 128} ld_out={ld_out} ld_res={ld_res}"
        gc.check(_run(kind, A, W, m, n, k, B, act, Rs[ld_res], ld_out=ld_out, what=what), ref, k, act, what, key=key)
        if i < 3:
            what = f"{kind} [{m}, {n}] k={k} act={act} column slices at 64 / 128 of [{k + 192}] / [{k + 256}] ld_out={ld_out} ld_res={ld_res}"
            gc.check(_run(kind, SA, SW, m, n, k, B, act, Rs[ld_res], ld_out=ld_out, a_col0=64, w_col0=128, what=what), ref, k, act, what, key=key)


# ---- identical bits whichever tile ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", (448, 576))
@pytest.mark.parametrize("kind", KINDS)
def test_bit_identity_through_the_entry_point(kind, k):
    """The same operand rows give the same bits whatever else the launch holds — hence whichever tile it takes: rows [:100] of an
    m = 300 call against an m = 100 call (128 tile), columns [:128] of n = 264 against n = 128 (128 tile), columns [:256] of
    n = 257 (128 tile: n % 8) against n = 256; at K = 448 the large tile is the register-staged one, at K = 576 (16-bit) the
    direct-to-LDS one with both of its drains.  And the same call twice."""
    a, w, bias, res, _ = _operands(kind, k)
    dt = gc.LO_DTYPES[kind]
    A = {m: _nan_matrix(a[:m], k, dt) for m in (100, 300)}
    W = {n: _nan_matrix(w[:n], k, dt) for n in (128, 256, 257, 264)}
    B = {n: _nan_vector(bias[:n]) for n in W}
    R = {(m, n): _nan_matrix(res[:m, :n], n, torch.float32) for m, n in ((300, 264), (100, 264), (300, 128), (300, 257), (300, 256))}
    tiles = set()
    for act, has_b, has_r in EPILOGUES:
        def run(m, n):
            tiles.add(expected_tile(kind, m, n, k, act, has_r, n, n))
            return _run(kind, A[m], W[n], m, n, k, B[n] if has_b else None, act, R[m, n] if has_r else None, what=f"{kind} [{m}, {n}] k={k} {act, has_b, has_r}")
        big = run(300, 264)
        what = f"{kind} k={k} act={act} bias={has_b} residual={has_r}"
        assert torch.equal(big.view(torch.int32), run(300, 264).view(torch.int32)), f"{what}: two runs differ"
        assert torch.equal(big[:100].view(torch.int32), run(100, 264).view(torch.int32)), f"{what}: rows [:100] of m = 300 differ from m = 100"
        assert torch.equal(big[:, :128].contiguous().view(torch.int32), run(300, 128).view(torch.int32)), f"{what}: columns [:128] of n = 264 differ from n = 128"
        assert torch.equal(run(300, 257)[:, :256].contiguous().view(torch.int32), run(300, 256).view(torch.int32)), f"{what}: columns [:256] of n = 257 differ from n = 256"
    assert tiles == ({T128, TREG} if kind == "f32" or k < 512 else {T128, TLDS, TLDS_GENERIC})


# ---- the sliced weight gradient ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ("bf16", "f16"))
def test_sliced_wgrad_in_16_bit_arithmetic(kind):
    """Ops.wgrad on dy_t [192, 8256], x_t [320, 8256]: four column slices of 2112 / 1920 on side streams (operands with lda > k)
    and a deterministic sum.  Held per element to the bound of ONE accumulation over k = 8256, against float64 on the rounded
    operands: a slice rounds at most 2112 times on its own part of mag and the sum of four partials adds three roundings on
    at most mag, which together stay below the (k + 2) of one accumulation.  Bit-equal on a second run."""
    from zett_amd.autograd import Ops
    k = 8256
    dy_t, x_t, _, _ = gc.operands(kind, 192, 320, k, seed=5)
    ops = Ops(torch.device(DEV), kind)
    d, x = dy_t.to(DEV), x_t.to(DEV)
    n_slices = min(16, 256 // 2, k // 2048)
    assert n_slices == 4                                          # the sliced path (autograd.Ops.wgrad: s_max >= 2)
    got = ops.wgrad(d, x)
    torch.cuda.synchronize()
    gc.check(got.cpu(), gc.reference(dy_t, x_t), k, 0, f"{kind} sliced wgrad", key=(kind, k, "sliced wgrad: " + TLDS))
    again = ops.wgrad(d, x)
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))


# ---- arguments and pointers ----------------------------------------------------------------------------------------------
def _refused(rc, *words):
    L, lib = _lib()
    assert rc == L.E_INVALID, rc
    msg = lib.zett_last_error().decode()
    assert all(w in msg for w in words), msg


def _untouched(out, what):
    torch.cuda.synchronize()
    back = out.buf.cpu()
    assert torch.equal(back.view(torch.int32), out.f.buf.view(torch.int32)), f"{what}: the output allocation was written"


@gpu
def test_bad_arguments_are_refused_and_empty_calls_write_nothing():
    a16 = _nan_matrix(torch.ones(8, 128).to(torch.bfloat16), 128, torch.bfloat16)
    a32 = _nan_matrix(torch.ones(8, 128), 128, torch.float32)
    out = OnDev(gc.Framed(8, 8, 12, torch.float32, "canary"))
    for kind, A in (("bf16", a16), ("f16", a16)):
        _refused(_raw(kind, A.ptr(), 128, A.ptr(), 128, 8, 8, 96, None, 0, None, 0, out.ptr(), 12), "multiple of 64")
        _refused(_raw(kind, A.ptr(), 132, A.ptr(), 128, 8, 8, 64, None, 0, None, 0, out.ptr(), 12), "multiples of 8")
        _refused(_raw(kind, A.ptr(), 128, A.ptr(), 132, 8, 8, 64, None, 0, None, 0, out.ptr(), 12), "multiples of 8")
    _refused(_raw("f32", a32.ptr(), 128, a32.ptr(), 128, 8, 8, 48, None, 0, None, 0, out.ptr(), 12), "multiple of 32")
    _refused(_raw("f32", a32.ptr(), 130, a32.ptr(), 128, 8, 8, 32, None, 0, None, 0, out.ptr(), 12), "multiples of 4")
    _refused(_raw("f32", a32.ptr(), 128, a32.ptr(), 130, 8, 8, 32, None, 0, None, 0, out.ptr(), 12), "multiples of 4")
    for kind, A, k in (("bf16", a16, 64), ("f16", a16, 64), ("f32", a32, 32)):
        assert _raw(kind, A.ptr(), 128, A.ptr(), 128, 0, 8, k, None, 0, None, 0, out.ptr(), 12) == 0          # m = 0
        assert _raw(kind, A.ptr(), 128, A.ptr(), 128, 8, 0, k, None, 0, None, 0, out.ptr(), 12) == 0          # n = 0
    _untouched(out, "refused and empty calls")


def test_misaligned_pointers_are_refused_before_any_launch():
    """(no GPU: a refused call launches nothing, so host addresses do) the pointer contract of include/zett_hip.h at the boundary"""
    L, lib = _lib()
    store = (C.c_float * 8192)()
    base = (C.addressof(store) + 255) & ~255
    p = lambda off: C.c_void_p(base + off)
    null = C.c_void_p(0)
    for kind, k in (("f32", 32), ("bf16", 64), ("f16", 64)):
        def call(a=0, w=0, bias=None, res=None, out=0):
            args = (p(a), k, p(4096 + w), k, 4, 8, k, null if bias is None else p(8192 + bias), 0, null if res is None else p(12288 + res), 8, p(16384 + out), 8, null)
            return lib.zett_op_gemm_f32(*args) if kind == "f32" else lib.zett_op_gemm_lo(L.PREC_BF16 if kind == "bf16" else L.PREC_F16, *args)
        for off in (2, 4, 8, 12):
            _refused(call(a=off), "a and w", "16-byte")
            _refused(call(w=off), "a and w", "16-byte")
        for off in (1, 2, 3):
            _refused(call(bias=off), "4-byte")
            _refused(call(res=off), "4-byte")
            _refused(call(out=off), "4-byte")
        _refused(call(a=8, out=2), "16-byte")


@gpu
@pytest.mark.parametrize("kind", KINDS)
def test_base_pointer_alignment(kind):
    """include/zett_hip.h: a and w 16-byte aligned, bias / residual / out 4-byte aligned, or ZETT_E_INVALID before any launch;
    out, residual or bias that are only 4-byte aligned send the call to the 128 tile (the float4 drains of both 256 tiles need
    16).  Refused pointers are refused with the output untouched; every accepted combination passes the check."""
    m, n, k = 257, 264, 576
    a, w, bias, res, _ = _operands(kind, k)
    dt = gc.LO_DTYPES[kind]
    A, W = _nan_matrix(a[:m], k, dt), _nan_matrix(w[:n], k, dt)
    out = OnDev(gc.Framed(m, n, n + 4, torch.float32, "canary"))
    B, R = _nan_vector(bias[:n]), _nan_matrix(res[:m, :n], n + 8, torch.float32)
    # (k - 64 columns: a moved operand, were it ever launched, still ends inside its rows)
    for shift in (8, 4) if kind == "f32" else (8, 4, 2):          # bytes: multiples of the element size below 16
        _refused(_raw(kind, A.ptr(byte_shift=shift), k, W.ptr(), k, m, n, k - 64, B.ptr(), 0, R.ptr(), n + 8, out.ptr(), n + 4), "16-byte")
        _refused(_raw(kind, A.ptr(), k, W.ptr(byte_shift=shift), k, m, n, k - 64, B.ptr(), 0, R.ptr(), n + 8, out.ptr(), n + 4), "16-byte")
    _refused(_raw(kind, A.ptr(), k, W.ptr(), k, m, n, k, B.ptr(byte_shift=2), 0, R.ptr(), n + 8, out.ptr(), n + 4), "4-byte")
    _refused(_raw(kind, A.ptr(), k, W.ptr(), k, m, n, k, B.ptr(), 0, R.ptr(byte_shift=2), n + 8, out.ptr(), n + 4), "4-byte")
    _refused(_raw(kind, A.ptr(), k, W.ptr(), k, m, n, k, B.ptr(), 0, R.ptr(), n + 8, out.ptr(byte_shift=2), n + 4), "4-byte")
    _untouched(out, "refused pointers")
    # accepted: each of out / residual / bias moved by one, two and four floats (4-, 8- and 16-byte aligned), alone and together
    for act in (0, 2):
        ref = _reference(kind, k, m, n, True, act, True)
        for so, sr, sb in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 0, 0), (0, 2, 0), (0, 0, 2), (1, 3, 2), (4, 4, 4)):
            Bs = OnDev(gc.Framed(None, n, n, torch.float32, float("nan"), shift=sb, values=bias[:n]))
            Rs = OnDev(gc.Framed(m, n, n + 8, torch.float32, float("nan"), shift=sr, values=res[:m, :n]))
            assert Bs.ptr().value % 16 == (4 * sb) % 16 and Rs.ptr().value % 16 == (4 * sr) % 16
            tile = expected_tile(kind, m, n, k, act, True, n + 4, n + 8, out_align=4 * so if so % 4 else 16, res_align=4 * sr if sr % 4 else 16,
                                 bias_align=4 * sb if sb % 4 else 16)
            assert tile == (T128 if (so, sr, sb) != (4, 4, 4) else (TREG if kind == "f32" else (TLDS if act == 0 else TLDS_GENERIC)))
            what = f"{kind} [{m}, {n}] k={k} act={act} out / residual / bias moved by {so} / {sr} / {sb} floats"
            got = _run(kind, A, W, m, n, k, Bs, act, Rs, ld_out=n + 4, out_shift=so, what=what)
            gc.check(got, ref, k, act, what, key=(kind, k, tile))
