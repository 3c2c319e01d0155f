"""The training row primitives of zett_amd/csrc/train_{operands,layernorm,attention,gather}.hip called directly through the C ABI and checked ELEMENT BY ELEMENT
against float64 on the same values (tests/train_ops_check.py), at the layout edges: leading dimensions wider than the data and not
multiples of four, row and column counts one short of, at and one past a tile, padding bands, grid-stride loops that stride, every
register layout of LayerNorm and attention in the dense, packed and position-0-only forms.

Buffers: every floating-point input and every output is a view INSIDE a larger allocation of this test (gemm_check.Framed /
train_ops_check.Frame) with 256 rows of its leading dimension (256 elements for a vector) in front of and behind it.  The slack of
what a kernel reads is NaN, the slack of what it writes — the columns cols .. ld - 1 of every row included — a canary bit pattern:
an index one tile too far still touches only this test's memory, a value fetched from outside poisons the result and a store
outside the output breaks the canary.  Nothing here is meant to fault.

The case tables are module constants and generators without a GPU in them: tests/test_train_ops_check_host.py restates the
dispatch rules of the kernels and asserts that the tables reach every branch.
"""
import ctypes as C
import itertools
import os

import pytest
import torch

from tests import train_ops_check as tc

DEV = "cuda:0"
gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
PRECS = ("bf16", "f16")


# ---- case tables (no GPU) ------------------------------------------------------------------------------------------------
T_ROWS = (1, 63, 64, 65, 130)
T_COLS = (1, 5, 60, 64, 68, 130)
LD_DELTAS = (0, 4, 1, 2)             # tight, + 4 (vector forms), + 1 / + 2 (scalar forms)


def transpose_cases(rows):
    """R x rows_padded in {R, next multiple of 64, R + 3} x C, and for each the leading-dimension surplus of the input, the
    transposed output, the plain copy and the pre-activation: every one of the four cycles through LD_DELTAS with its own phase,
    so that each meets each value and the vector and scalar forms of every load and store run.  act_kind alternates 1 / 2."""
    out = []
    for i, (rp, c) in enumerate(itertools.product((0, 1, 2), T_COLS)):
        rpad = (rows, (rows + 63) // 64 * 64, rows + 3)[rp]
        j = i + T_ROWS.index(rows)
        out.append(dict(R=rows, Rpad=rpad, C=c, d_in=LD_DELTAS[j % 4], d_out=LD_DELTAS[(j // 4 + j) % 4], d_plain=LD_DELTAS[(j + 1) % 4],
                        d_z=LD_DELTAS[(j + 2) % 4], kind=1 + j % 2, cols_padded=c + (0, 3, 4)[j % 3]))
    return out


CONVERT_STRIDE = (65535 + 70, 8)     # rows x cols: convert_lo4_kernel's grid is capped at 65 535 rows

EW_SHAPES = ((7, 30, 0), (33, 1028, 0), (33, 1028, 1))      # rows, cols, elements the output is moved into its storage (1: V = 1)
EW_STRIDE = {"wide": 4 * (65535 * 256 + 300), "scalar": 65535 * 256 + 301}      # just past grid_for's cap, in work items
GELU_LO_N = (3084, 3085, 211)        # n % 4 = 0, 1, 3

LN_H = (4, 64, 1020, 1024, 1028, 2048, 2052, 4096, 4100, 8192)
LN_ROWS = (1, 3, 37)
LN_STRIDE = (16384 + 5, 64)          # rows x h: ln_fwd_kernel's grid is capped at 16 384 rows


def ln_nparts(rows):
    return sorted({1, 2, rows, rows + 5})


ATT_N = 7
ATT_SEQ = {2: (1, 2), 4: (3, 4), 8: (5, 8), 16: (9, 16), 32: (17, 32)}        # LMAX -> the two sequence lengths of the issue that take it
ATT_D = {1: (8, 64), 2: (72, 128), 4: (136, 256)}                             # DV -> head dims
ATT_FORMS = ("dense", "packed", "cls")


def attention_cases():
    """every (LMAX, DV) pair in each of the three forms, 45 cases: the two sequence lengths and head dims of a pair, the head counts
    1 / 3 / 5, fused and separate q k v, tight and + 4 leading dimensions of the outputs and the 16-bit context alternate along
    the table so that every value of every one of them occurs in every form"""
    out = []
    for f, form in enumerate(ATT_FORMS):
        for i, (lmax, dv) in enumerate(itertools.product(ATT_SEQ, ATT_D)):
            j = i + f
            out.append(dict(form=form, seq=ATT_SEQ[lmax][(i // 3 + f) % 2], d=ATT_D[dv][j % 2], heads=(1, 3, 5)[j % 3], fused=form != "cls" and j % 2 == 0,
                            wide_ld=(j // 2) % 2 == 1, ctx_lo=(None, "bf16", None, "f16")[j % 4], seed=100 * f + i))
    return out


def attention_lengths(case):
    """-> the positions of each of the ATT_N rows: seq everywhere (dense), or drawn from 1 .. seq with row 0 of length seq and row 3
    of length 1 (packed, cls)"""
    seq = case["seq"]
    if case["form"] == "dense":
        return [seq] * ATT_N
    g = torch.Generator().manual_seed(case["seed"])
    lens = torch.randint(1, seq + 1, (ATT_N,), generator=g).tolist()
    lens[0], lens[3] = seq, 1
    return lens


IDX_COLS = (1, 30, 256, 260, 516)
IDX_SRC_ROWS, IDX_ROWS = 23, 90
GATHER_V0, GATHER_FB, GATHER_T = 11, 4, 40
GATHER_EDGE_IDS = (0, GATHER_V0 - 1, GATHER_V0, GATHER_V0 + GATHER_FB - 1)
ROWDOT_SHAPES = ((1, 4), (50, 64), (9, 300), (5, 1030))
COLSUM_ROWS = (1, 63, 64, 65, 1000)


def index_rows():
    """idx [IDX_ROWS]: every source row at least once, row 5 fifty times, the first and the last row"""
    g = torch.Generator().manual_seed(3)
    idx = list(range(IDX_SRC_ROWS)) + [5] * 49 + [0, IDX_SRC_ROWS - 1]
    idx += torch.randint(0, IDX_SRC_ROWS, (IDX_ROWS - len(idx),), generator=g).tolist()
    perm = torch.randperm(IDX_ROWS, generator=g)
    return torch.tensor(idx, dtype=torch.int32)[perm]


def gather_ids():
    g = torch.Generator().manual_seed(4)
    ids = list(GATHER_EDGE_IDS) + torch.randint(0, GATHER_V0 + GATHER_FB, (GATHER_T - 4,), generator=g).tolist()
    return torch.tensor(ids, dtype=torch.int32)[torch.randperm(GATHER_T, generator=g)]


# ---- plumbing ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = os.environ.get(tc.RECORD_ENV)          # figures for profiles/train_ops_check.md
    if path and tc.RECORD:
        tc.write_record(path)


def _lib():
    from zett_amd import _lib
    return _lib, _lib.load()


NULL = C.c_void_p(0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _prec(kind):
    L, _ = _lib()
    return L.PREC_BF16 if kind == "bf16" else L.PREC_F16


class OnDev:
    """a Frame and its copy on the device"""

    def __init__(self, frame):
        self.f = frame
        self.buf = frame.buf.to(DEV)
        assert self.buf.data_ptr() % 256 == 0

    def ptr(self, col0=0):
        return C.c_void_p(self.buf.data_ptr() + self.f.byte_offset() + col0 * self.buf.element_size())

    def back(self, what, inside=True):
        """after a call: the canary check, -> the view on the host"""
        torch.cuda.synchronize()
        host = self.buf.cpu()
        (tc.check_canary if inside else tc.check_slack)(self.f, host, what)
        return self.f.view(host).clone()


def I(values, ld=None, shift=0):
    """an input: NaN around it and in the columns cols .. ld - 1"""
    if values.dim() == 1:
        return OnDev(tc.Frame(None, values.shape[0], values.shape[0], values.dtype, float("nan"), shift=shift, values=values))
    return OnDev(tc.Frame(values.shape[0], values.shape[1], ld or values.shape[1], values.dtype, float("nan"), shift=shift, values=values))


def O(rows, cols, ld=None, dtype=F32, values=None, shift=0):
    """an output: the canary around it and in the columns cols .. ld - 1 (values: what it holds before the call)"""
    return OnDev(tc.Frame(rows, cols, ld or cols, dtype, "canary", shift=shift, values=values))


def _ok(rc, what):
    if rc != 0:
        raise AssertionError(f"{what}: return code {rc}: {_lib()[1].zett_last_error().decode()}")


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _uniform(g, *shape):
    return torch.rand(*shape, generator=g) * 2 - 1


# ---- transposes and conversions --------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("rows", T_ROWS)
@pytest.mark.parametrize("kind", PRECS)
def test_transposes_and_conversions(kind, rows):
    """zett_op_transpose_f32 / _lo / _lo16, zett_op_grad_operands_lo without and with a pre-activation, zett_op_convert_lo: bit
    equality with torch's transposition and round-to-nearest-even conversion (zero bands included); behind gelu' the 16-bit rule of
    train_ops_check.lo_bound; every band's column-sum partial per element and their sum against float64"""
    _, lib = _lib()
    lo, prec, st = tc.LO[kind], _prec(kind), _stream()
    for case in transpose_cases(rows):
        R, Rpad, Cc = case["R"], case["Rpad"], case["C"]
        g = torch.Generator().manual_seed(R * 1000 + Rpad * 7 + Cc)
        x, z = _uniform(g, R, Cc), (_randn(g, R, Cc) * 2.5).clamp(-7.99, 7.99)
        ld_in, ld_out, ld_plain, ld_z = Cc + case["d_in"], Rpad + case["d_out"], Cc + case["d_plain"], Cc + case["d_z"]
        what = f"{kind} R={R} Rpad={Rpad} C={Cc} ld_in={ld_in} ld_out={ld_out} ld_plain={ld_plain} ld_z={ld_z}"
        layout = f"in {'vector' if ld_in % 4 == 0 else 'scalar'}, out {'vector' if ld_out % 4 == 0 else 'scalar'}"
        X, X16, Z = I(x, ld_in), I(x.to(lo), ld_in), I(z, ld_z)

        out = O(Cc, Rpad, ld_out)
        _ok(lib.zett_op_transpose_f32(X.ptr(), ld_in, out.ptr(), ld_out, R, Cc, Rpad, st), what)
        tc.exact(out.back(f"transpose_f32 {what}"), tc.transpose_ref(x, Rpad, F32), f"transpose_f32 {what}", key=("transpose_f32", layout))

        out = O(Cc, Rpad, ld_out, lo)
        _ok(lib.zett_op_transpose_lo(prec, X.ptr(), ld_in, out.ptr(), ld_out, R, Cc, Rpad, st), what)
        tc.exact(out.back(f"transpose_lo {what}"), tc.transpose_ref(x, Rpad, lo), f"transpose_lo {what}", key=(f"transpose_lo {kind}", layout))

        out = O(Cc, Rpad, ld_out, lo)
        _ok(lib.zett_op_transpose_lo16(prec, X16.ptr(), ld_in, out.ptr(), ld_out, R, Cc, Rpad, st), what)
        tc.exact(out.back(f"transpose_lo16 {what}"), tc.transpose_ref(x.to(lo), Rpad, lo), f"transpose_lo16 {what}", key=(f"transpose_lo16 {kind}", layout))

        bands = (R + 63) // 64
        for zed in (None, Z):
            name = f"grad_operands_lo{'' if zed is None else ' act ' + str(case['kind'])} {what}"
            key = (f"grad_operands_lo {kind}{'' if zed is None else ' gelu'}", layout + f", plain {'vector' if ld_plain % 4 == 0 else 'scalar'}")
            t, plain, part = O(Cc, Rpad, ld_out, lo), O(R, Cc, ld_plain, lo), O(bands, Cc)
            _ok(lib.zett_op_grad_operands_lo(prec, X.ptr(), ld_in, NULL if zed is None else zed.ptr(), ld_z if zed is not None else 0, case["kind"] if zed is not None else 0,
                                             R, Cc, Rpad, plain.ptr(), ld_plain, t.ptr(), ld_out, part.ptr(), st), name)
            v, b32 = tc.grad_operands_ref(x, None if zed is None else z, case["kind"])
            got_t, got_plain, got_part = t.back(name + " dy_t"), plain.back(name + " dy_lo"), part.back(name + " colsum_part")
            if zed is None:
                tc.exact(got_plain, x.to(lo), name + " dy_lo", key=key)
                tc.exact(got_t, tc.transpose_ref(x, Rpad, lo), name + " dy_t", key=key)
            else:
                tc.check(got_plain, v, tc.lo_bound(v, b32, lo), name + " dy_lo", key=key)
                tc.check(got_t[:, :R], v.T, tc.lo_bound(v, b32, lo).T, name + " dy_t", key=key)
                tc.exact(got_t[:, R:].contiguous(), torch.zeros(Cc, Rpad - R, dtype=lo), name + " dy_t zero band", key=key)
            ref_part, b_part = tc.colpart_ref(v, b32)
            tc.check(got_part, ref_part, b_part, name + " colsum_part", key=(key[0] + " colsum_part", "band partials"))
            tc.check(got_part.double().sum(0), v.sum(0), b_part.sum(0), name + " sum of colsum_part", key=(key[0] + " colsum_part", "sum of bands"), slice_rel=tc.REL_SUM)

        cp = case["cols_padded"]
        for d_out in (0, 4, 1):
            out = O(R, cp, cp + d_out, lo)
            name = f"convert_lo {kind} [{R}, {Cc}] cols_padded={cp} ld_in={ld_in} ld_out={cp + d_out}"
            _ok(lib.zett_op_convert_lo(prec, X.ptr(), ld_in, out.ptr(), cp + d_out, R, Cc, cp, st), name)
            tc.exact(out.back(name), tc.convert_ref(x, cp, lo), name, key=(f"convert_lo {kind}", "rows of four" if convert_wide(Cc, cp, ld_in, cp + d_out) else "general cast"))


def convert_wide(cols, cols_padded, ld_in, ld_out):
    """zett_op_convert_lo: convert_lo4_kernel (bases aligned as the frames here are), else launch_cast"""
    return cols_padded == cols and cols % 4 == 0 and ld_in % 4 == 0 and ld_out % 4 == 0


@gpu
@pytest.mark.parametrize("kind", PRECS)
def test_convert_lo_grid_stride(kind):
    """more rows than convert_lo4_kernel's grid: the workgroups take a second row"""
    _, lib = _lib()
    rows, cols = CONVERT_STRIDE
    assert convert_wide(cols, cols, cols, cols)
    x = _randn(torch.Generator().manual_seed(9), rows, cols)
    X, out = I(x), O(rows, cols, cols, tc.LO[kind])
    _ok(lib.zett_op_convert_lo(_prec(kind), X.ptr(), cols, out.ptr(), cols, rows, cols, cols, _stream()), "convert_lo grid stride")
    tc.exact(out.back("convert_lo grid stride"), x.to(tc.LO[kind]), f"convert_lo {kind} [{rows}, {cols}]", key=(f"convert_lo {kind}", "rows of four, grid stride"))


# ---- element-wise and GELU -------------------------------------------------------------------------------------------------
def elementwise_wide(rows, cols, shift):
    """zett_op_elementwise_f32 / zett_op_gelu_*: V = 4 for cols % 4 == 0, n % 4 == 0 and 16-byte aligned bases"""
    return cols % 4 == 0 and (rows * cols) % 4 == 0 and shift % 4 == 0


@gpu
@pytest.mark.parametrize("rows,cols,shift", EW_SHAPES)
def test_elementwise_and_gelu(rows, cols, shift):
    """ops 0 - 4 with every null form, both GELUs forward and backward, on the wide and the scalar path"""
    _, lib = _lib()
    st, n = _stream(), rows * cols
    g = torch.Generator().manual_seed(rows + cols + shift)
    a, b, vec, vec2, s = _randn(g, rows, cols), _randn(g, rows, cols), _randn(g, cols), _randn(g, cols), _randn(g, rows)
    A, B, V, V2, S = I(a.flatten()), I(b.flatten()), I(vec), I(vec2), I(s)
    layout = "wide" if elementwise_wide(rows, cols, shift) else "scalar"

    def run(op, pa, pb, pv, pv2, ps, name):
        out = O(None, n, shift=shift)
        _ok(lib.zett_op_elementwise_f32(op, pa, pb, pv, pv2, ps, out.ptr(), n, cols, st), name)
        return out.back(f"{name} [{rows}, {cols}] {layout}").view(rows, cols)

    key = lambda name: (name, layout)
    tc.exact(run(0, A.ptr(), B.ptr(), NULL, NULL, NULL, "add"), a + b, "add", key=key("add"))
    tc.exact(run(1, A.ptr(), B.ptr(), NULL, NULL, NULL, "mul"), a * b, "mul", key=key("mul"))
    tc.exact(run(2, A.ptr(), NULL, V.ptr(), NULL, NULL, "affine_cols vec"), a * vec, "affine_cols vec", key=key("affine_cols, one operand"))
    tc.exact(run(2, A.ptr(), NULL, NULL, V2.ptr(), NULL, "affine_cols vec2"), a + vec2, "affine_cols vec2", key=key("affine_cols, one operand"))
    tc.check(run(2, A.ptr(), NULL, V.ptr(), V2.ptr(), NULL, "affine_cols"), a.double() * vec.double() + vec2.double(), tc.fma_bound(a.double() * vec.double(), vec2.double().expand(rows, cols)),
             "affine_cols", key=key("affine_cols"), slice_rel=tc.REL_SUM)
    sw = s.double()[:, None] * vec.double()[None, :]
    tc.check(run(3, A.ptr(), NULL, V.ptr(), NULL, S.ptr(), "add_outer"), a.double() + sw, tc.fma_bound(sw, a.double()), "add_outer", key=key("add_outer"), slice_rel=tc.REL_SUM)
    tc.exact(run(4, A.ptr(), NULL, NULL, NULL, S.ptr(), "scale_rows"), a * s[:, None], "scale_rows", key=key("scale_rows"))
    tc.exact(run(4, NULL, NULL, V.ptr(), NULL, S.ptr(), "outer"), s[:, None] * vec[None, :], "outer", key=key("scale_rows, a null"))

    z, dh = (_randn(g, n) * 2.5).clamp(-7.99, 7.99), _uniform(g, n)
    Z, DH = I(z), I(dh)
    for kind in (1, 2):
        out = O(None, n, shift=shift)
        _ok(lib.zett_op_gelu_fwd_f32(Z.ptr(), out.ptr(), n, kind, st), "gelu_fwd")
        tc.check(out.back(f"gelu_fwd kind {kind} {layout}"), tc.gelu(z.double(), kind), torch.full((n,), tc.ACT_ABS, dtype=F64), f"gelu_fwd kind {kind} [{n}] {layout}", key=key("gelu_fwd"))
        out = O(None, n, shift=shift)
        _ok(lib.zett_op_gelu_bwd_f32(Z.ptr(), DH.ptr(), out.ptr(), n, kind, st), "gelu_bwd")
        ref, bnd = tc.gelu_bwd_ref(z, dh, kind)
        tc.check(out.back(f"gelu_bwd kind {kind} {layout}"), ref, bnd, f"gelu_bwd kind {kind} [{n}] {layout}", key=key("gelu_bwd"))


@gpu
@pytest.mark.parametrize("n", GELU_LO_N)
@pytest.mark.parametrize("kind", PRECS)
def test_gelu_fwd_lo(kind, n):
    """the activation as a 16-bit operand: groups of four and the element tail (n % 4 = 0, 1, 3)"""
    _, lib = _lib()
    z = (_randn(torch.Generator().manual_seed(n), n) * 2.5).clamp(-7.99, 7.99)
    Z = I(z)
    for act in (1, 2):
        out = O(None, n, dtype=tc.LO[kind])
        _ok(lib.zett_op_gelu_fwd_lo(_prec(kind), Z.ptr(), out.ptr(), n, act, _stream()), "gelu_fwd_lo")
        ref = tc.gelu(z.double(), act)
        tc.check(out.back(f"gelu_fwd_lo {kind} n={n}"), ref, tc.lo_bound(ref, torch.full((n,), tc.ACT_ABS, dtype=F64), tc.LO[kind]), f"gelu_fwd_lo {kind} kind {act} n={n}",
                 key=(f"gelu_fwd_lo {kind}", f"n % 4 = {n % 4}"))


def _device_frame(n, fill_bits):
    """[256 | n | 256] floats on the device, the slack filled with a bit pattern"""
    buf = torch.empty(n + 512, dtype=F32, device=DEV)
    buf.view(torch.int32)[:256] = fill_bits
    buf.view(torch.int32)[256 + n:] = fill_bits
    return buf


@gpu
@pytest.mark.parametrize("path", ("wide", "scalar"))
def test_elementwise_and_gelu_grid_stride(path):
    """just past 65 535 * 256 work items (grid_for's cap): the grid-stride loops of elementwise_kernel and gelu_fwd_kernel take a
    second pass.  Compared on the device: add bit-equal to torch fp32, GELU within its absolute allowance of float64 torch."""
    _, lib = _lib()
    n = EW_STRIDE[path]
    work = n // 4 if path == "wide" else n
    assert elementwise_wide(1, n, 0) == (path == "wide") and work > 65535 * 256
    nan_bits = 0x7FC00000
    a, b, out = _device_frame(n, nan_bits), _device_frame(n, nan_bits), _device_frame(n, tc.CANARY_BITS)
    g = torch.Generator(device=DEV).manual_seed(11)
    a[256:256 + n].normal_(generator=g)
    b[256:256 + n].normal_(generator=g).mul_(2.5).clamp_(-7.99, 7.99)
    out.view(torch.int32)[256:256 + n] = tc.CANARY_BITS
    ptr = lambda t: C.c_void_p(t.data_ptr() + 1024)

    def intact(what):
        bits = out.view(torch.int32)
        assert bool((bits[:256] == tc.CANARY_BITS).all()) and bool((bits[256 + n:] == tc.CANARY_BITS).all()), f"{what}: the canary around the output is broken"

    _ok(lib.zett_op_elementwise_f32(0, ptr(a), ptr(b), NULL, NULL, NULL, ptr(out), n, n, _stream()), "add")
    torch.cuda.synchronize()
    intact("add")
    got, want = out[256:256 + n], a[256:256 + n] + b[256:256 + n]
    bad = torch.nonzero(got.view(torch.int32) != want.view(torch.int32))
    assert bad.numel() == 0, f"add {path} n={n}: {bad.shape[0]} element(s) differ, first at {int(bad[0])}: got {float(got[int(bad[0])])!r}, expected {float(want[int(bad[0])])!r}"
    del want
    for kind in (1, 2):
        out.view(torch.int32)[256:256 + n] = tc.CANARY_BITS
        _ok(lib.zett_op_gelu_fwd_f32(ptr(b), ptr(out), n, kind, _stream()), "gelu_fwd")
        torch.cuda.synchronize()
        intact("gelu_fwd")
        err = (out[256:256 + n].double() - tc.gelu(b[256:256 + n].double(), kind)).abs()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
        worst = int(torch.argmax(err))
        print(f"gelu_fwd kind {kind} {path} n={n}: largest |err| {float(err[worst]):.3e} at {worst}")
        assert float(err[worst]) <= tc.ACT_ABS, f"gelu_fwd kind {kind} {path} n={n}: |err| {float(err[worst]):.3e} at element {worst} over {tc.ACT_ABS}"
        del err


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------
def ln_j(h):
    """the register layout of ln_fwd_kernel / ln_bwd_kernel: J = ceil(h / 1024) rounded up to 1 / 2 / 4 / 8"""
    j = (h + 1023) // 1024
    return 1 if j <= 1 else 2 if j <= 2 else 4 if j <= 4 else 8


def _ln_inputs(rows, h, seed):
    g = torch.Generator().manual_seed(seed)
    x = _randn(g, rows, h) * 1.5 + 0.3
    if rows >= 3:
        x[1] = 0.5                    # variance 0: mean and every difference exact, rstd = 1 / sqrt(eps), y = beta
    return x, 1 + 0.1 * _randn(g, h), 0.1 * _randn(g, h), _randn(g, rows, h), _randn(g, rows, h)


def _ln_forward(lib, x, gamma, beta, ld, lo_kind, what, key):
    rows, h = x.shape
    X, G, B = I(x, ld), I(gamma), I(beta)
    y, stats = O(rows, h), O(rows, 2)
    y_lo = None if lo_kind is None else O(rows, h, h, tc.LO[lo_kind])
    _ok(lib.zett_op_layernorm_fwd_f32(X.ptr(), ld, G.ptr(), B.ptr(), 1e-5, y.ptr(), stats.ptr(), rows, h, NULL if y_lo is None else y_lo.ptr(),
                                      _prec(lo_kind or "bf16"), _stream()), what)
    ref = tc.layernorm_ref(x, gamma, beta, 1e-5)
    bnd = tc.layernorm_bound(x, gamma, beta, 1e-5, ref)
    got_stats = stats.back(what + " stats")
    tc.check(y.back(what + " y"), ref["y"], bnd["y"], what + " y", key=key, slice_rel=tc.REL_FWD, whole_rel=tc.REL_LN_FWD)
    tc.check(got_stats[:, 0], ref["mean"], bnd["mean"], what + " mean", key=(key[0] + " stats", key[1]))
    tc.check(got_stats[:, 1], ref["rstd"], bnd["rstd"], what + " rstd", key=(key[0] + " stats", key[1]))
    if y_lo is not None:
        tc.check(y_lo.back(what + " y_lo"), ref["y"], tc.lo_bound(ref["y"], bnd["y"], tc.LO[lo_kind]), what + f" y_lo {lo_kind}", key=(key[0] + " y_lo " + lo_kind, key[1]))
    return X, G, got_stats


@gpu
@pytest.mark.parametrize("h", LN_H)
def test_layernorm_forward_and_backward(h):
    """every register layout (J = 1, 2, 4, 8; a partly filled last pass at 1020, 1028, 2052, 4100), x contiguous and as a column slice
    of a wider matrix (ld = h + 4, NaN beside it), y_lo in both types, a row of variance 0; the backward with n_part = 1, 2, rows and
    rows + 5 (workgroups without rows write zeros), with and without the residual gradient, from the statistics of the forward"""
    _, lib = _lib()
    for rows in LN_ROWS:
        x, gamma, beta, dy, dy2 = _ln_inputs(rows, h, 31 * h + rows)
        DY, DY2 = I(dy), I(dy2)
        for ld, lo_kind in ((h, "bf16"), (h + 4, "f16")):
            layout = f"J={ln_j(h)}, ld {'= h' if ld == h else '> h'}"
            what = f"layernorm [{rows}, {h}] ld={ld}"
            X, G, stats = _ln_forward(lib, x, gamma, beta, ld, lo_kind, what, ("layernorm_fwd", layout))
            if rows >= 3:
                assert float(stats[1, 0]) == 0.5 and bool(torch.isfinite(stats[1, 1])), stats[1]          # (rstd itself: held per element above)
            ST = I(stats)
            for i, n_part in enumerate(ln_nparts(rows)):
                with_dy2 = (i + (ld != h)) % 2 == 1
                name = f"layernorm_bwd [{rows}, {h}] ld={ld} n_part={n_part} dy2={with_dy2}"
                dx, parts = O(rows, h), O(2 * n_part, h)
                _ok(lib.zett_op_layernorm_bwd_f32(DY.ptr(), DY2.ptr() if with_dy2 else NULL, X.ptr(), ld, ST.ptr(), G.ptr(), dx.ptr(), parts.ptr(), n_part, rows, h, _stream()), name)
                ref = tc.layernorm_bwd_ref(dy, dy2 if with_dy2 else None, x, stats, gamma, n_part)
                bnd = tc.layernorm_bwd_bound(dy, dy2 if with_dy2 else None, x, stats, gamma, n_part)
                key = ("layernorm_bwd", layout + f", n_part {'1' if n_part == 1 else '> rows' if n_part > rows else '<= rows'}")
                tc.check(dx.back(name + " dx"), ref["dx"], bnd["dx"], name + " dx", key=key, slice_rel=tc.REL_BWD)
                got = parts.back(name + " partials").reshape(n_part, 2, h)
                tc.check(got.reshape(2 * n_part, h), ref["partials"].reshape(2 * n_part, h), bnd["partials"].reshape(2 * n_part, h), name + " partials", key=(key[0] + " partials", key[1]))
                for j, param in enumerate(("dgamma", "dbeta")):
                    tc.check(got.double().sum(0)[j], ref["partials"].sum(0)[j], bnd["partials"].sum(0)[j], f"{name} {param}", key=(f"{key[0]} {param}", key[1]), slice_rel=tc.REL_PARAM)


@gpu
def test_layernorm_forward_grid_stride():
    """more rows than ln_fwd_kernel's grid: the workgroups take a second row; y and stats per element"""
    _, lib = _lib()
    rows, h = LN_STRIDE
    x, gamma, beta, _, _ = _ln_inputs(rows, h, 5)
    _ln_forward(lib, x, gamma, beta, h + 4, None, f"layernorm [{rows}, {h}] grid stride", ("layernorm_fwd", "J=1, ld > h, grid stride"))


# ---- attention -------------------------------------------------------------------------------------------------------------
def att_lmax(seq):
    return 2 if seq <= 2 else 4 if seq <= 4 else 8 if seq <= 8 else 16 if seq <= 16 else 32


def att_dv(d):
    return 1 if d <= 64 else 2 if d <= 128 else 4


def att_bwd_refused(seq, d):
    return d > 128 and seq > 16


def _attention_inputs(case):
    lens = attention_lengths(case)
    offs = [0]
    for n in lens:
        offs.append(offs[-1] + n)
    T, hd = offs[-1], case["heads"] * case["d"]
    g = torch.Generator().manual_seed(case["seed"])
    cls = case["form"] == "cls"
    Tq = ATT_N if cls else T
    q, k, v, dctx = _randn(g, Tq, hd), _randn(g, T, hd), _randn(g, T, hd), _randn(g, Tq, hd)
    mask = torch.rand(T, generator=g) < 0.7
    mask[offs[1]:offs[2]] = False                   # row 1: every key masked (uniform probabilities)
    mask[offs[2]:offs[3]] = False                   # row 2: only key 0 visible
    mask[offs[2]] = True
    mask[offs[4]:offs[5]] = True                    # row 4: every key visible
    return lens, offs, q, k, v, dctx, mask


@gpu
@pytest.mark.parametrize("case", attention_cases(), ids=lambda c: f"{c['form']}-L{c['seq']}-d{c['d']}-h{c['heads']}")
def test_attention_forward_and_backward(case):
    """ctx, probs, dq, dk, dv per element in every (LMAX, DV) register layout, dense, packed and position-0-only; fused q k v
    (ldq = ld = 3 H) and separate tensors; ld_ctx, ld_dq, ld_d tight and + 4 with canary columns; the 16-bit context with ctx NULL"""
    L_, lib = _lib()
    seq, d, heads, form = case["seq"], case["d"], case["heads"], case["form"]
    cls, hd = form == "cls", heads * d
    lens, offs, q, k, v, dctx, mask = _attention_inputs(case)
    T, Tq = offs[-1], q.shape[0]
    what = f"attention {form} seq={seq} lens={lens} heads={heads} d={d} fused={case['fused']} wide_ld={case['wide_ld']}"
    layout = f"LMAX={att_lmax(seq)}, DV={att_dv(d)}, {form}"
    if case["fused"]:
        QKV = I(torch.cat([q, k, v], 1))
        pq, pk, pv, ldq, ld = QKV.ptr(), QKV.ptr(hd), QKV.ptr(2 * hd), 3 * hd, 3 * hd
    else:
        Q, KV = I(q, hd + 8), I(torch.cat([k, v], 1))
        pq, pk, pv, ldq, ld = Q.ptr(), KV.ptr(), KV.ptr(hd), hd + 8, 2 * hd
    M = mask.to(torch.uint8).to(DEV)
    OFF = None if form == "dense" else torch.tensor(offs, dtype=torch.int32).to(DEV)
    p_off = NULL if OFF is None else C.c_void_p(OFF.data_ptr())
    extra = 4 if case["wide_ld"] else 0
    ld_ctx = hd + extra
    probs = O(ATT_N * heads * seq, seq)
    ctx = O(Tq, hd, ld_ctx)
    st = _stream()
    _ok(lib.zett_op_attention_fwd_f32(pq, ldq, pk, pv, ld, C.c_void_p(M.data_ptr()), p_off, ATT_N, seq, heads, d, int(cls), ctx.ptr(), ld_ctx, probs.ptr(), NULL, 0, st), what)
    ref = tc.attention_ref(q, k, v, mask, offs, heads, d, cls)
    tc.check(ctx.back(what + " ctx"), ref["ctx"], ref["b_ctx"], what + " ctx", key=("attention_fwd ctx", layout), slice_rel=tc.REL_FWD)
    got_probs = tc.probs_from_buffer(probs.back(what + " probs", inside=False), offs, seq, heads, cls)
    for r, (gp, rp, bp) in enumerate(zip(got_probs, ref["probs"], ref["b_probs"])):
        L = lens[r]
        name = f"{what} probs of row {r}"
        tc.check(gp.reshape(-1, L), rp.reshape(-1, L), bp.reshape(-1, L), name, key=("attention_fwd probs", layout))
        assert float((gp.double().sum(-1) - 1).abs().max()) <= seq * tc.U, f"{name}: a row sums to 1 + {float((gp.double().sum(-1) - 1).abs().max()):.3e}"
        m = mask[offs[r]:offs[r + 1]]
        if bool(m.any()):
            assert bool((gp[..., ~m] == 0).all()), f"{name}: a masked key has a non-zero probability"
    if case["ctx_lo"]:
        lo = tc.LO[case["ctx_lo"]]
        ctx16, probs2 = O(Tq, hd, ld_ctx, lo), O(ATT_N * heads * seq, seq)
        _ok(lib.zett_op_attention_fwd_f32(pq, ldq, pk, pv, ld, C.c_void_p(M.data_ptr()), p_off, ATT_N, seq, heads, d, int(cls), NULL, ld_ctx, probs2.ptr(), ctx16.ptr(),
                                          _prec(case["ctx_lo"]), st), what + " ctx_lo")
        tc.check(ctx16.back(what + " ctx_lo"), ref["ctx"], tc.lo_bound(ref["ctx"], ref["b_ctx"], lo), what + f" ctx_lo {case['ctx_lo']}", key=(f"attention_fwd ctx_lo {case['ctx_lo']}", layout))
        assert torch.equal(probs2.back(what + " probs, ctx_lo", inside=False).view(torch.int32), probs.back(what + " probs", inside=False).view(torch.int32))

    DC = I(dctx, ld_ctx)
    ld_dq, ld_d = hd + extra, hd + (0 if case["wide_ld"] else 4)
    dq, dk, dv = O(Tq, hd, ld_dq), O(T, hd, ld_d), O(T, hd, ld_d)
    rc = lib.zett_op_attention_bwd_f32(DC.ptr(), ld_ctx, pq, ldq, pk, pv, ld, probs.ptr(), p_off, ATT_N, seq, heads, d, int(cls), dq.ptr(), ld_dq, dk.ptr(), dv.ptr(), ld_d, st)
    if att_bwd_refused(seq, d):
        assert rc == L_.E_INVALID and "up to 16 positions" in lib.zett_last_error().decode()
        for o in (dq, dk, dv):
            torch.cuda.synchronize()
            assert torch.equal(o.buf.cpu().view(torch.int32), o.f.buf.view(torch.int32)), what + ": a refused backward wrote to its outputs"
        return
    _ok(rc, what + " backward")
    bref = tc.attention_bwd_ref(dctx, q, k, v, got_probs, offs, heads, d, cls)
    for name, o in (("dq", dq), ("dk", dk), ("dv", dv)):
        tc.check(o.back(f"{what} {name}"), bref[name], bref["b_" + name], f"{what} {name}", key=(f"attention_bwd {name}", layout), slice_rel=tc.REL_BWD, whole_rel=tc.REL_ATT_BWD)


@gpu
def test_attention_refuses_what_it_cannot_hold():
    """seq = 33 and head_dim = 257 in both directions: ZETT_E_INVALID, the canary-filled outputs untouched"""
    L_, lib = _lib()
    x = I(torch.zeros(40, 520))
    M = torch.ones(40, dtype=torch.uint8, device=DEV)
    outs = [O(40, 520) for _ in range(4)]
    probs = O(33 * 33, 33)
    st = _stream()
    for seq, d, word in ((33, 8, "positions"), (1, 257, "head dims")):
        rc = lib.zett_op_attention_fwd_f32(x.ptr(), 520, x.ptr(), x.ptr(), 520, C.c_void_p(M.data_ptr()), NULL, 1, seq, 1, d, 0, outs[0].ptr(), 520, probs.ptr(), NULL, 0, st)
        assert rc == L_.E_INVALID and word in lib.zett_last_error().decode()
        rc = lib.zett_op_attention_bwd_f32(x.ptr(), 520, x.ptr(), 520, x.ptr(), x.ptr(), 520, probs.ptr(), NULL, 1, seq, 1, d, 0, outs[1].ptr(), 520, outs[2].ptr(), outs[3].ptr(), 520, st)
        assert rc == L_.E_INVALID and word in lib.zett_last_error().decode()
    torch.cuda.synchronize()
    for o in outs + [probs]:
        assert torch.equal(o.buf.cpu().view(torch.int32), o.f.buf.view(torch.int32)), "a refused call wrote to its outputs"


# ---- indexed rows and the source gather ------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cols", IDX_COLS)
def test_gather_rows_and_scatter_add_rows(cols):
    """out[r] = a[r] + src[idx[r]] (a null: a copy) and dst[idx[r]] += src[r] into a destination that is not zero; one, two and three
    passes of the column loop, leading dimensions of src / dst tight and wider, a row hit 50 times"""
    _, lib = _lib()
    g = torch.Generator().manual_seed(cols)
    idx = index_rows()
    IDX = idx.to(DEV)
    src, a, upd, dst0 = _randn(g, IDX_SRC_ROWS, cols), _randn(g, IDX_ROWS, cols), _randn(g, IDX_ROWS, cols), _randn(g, IDX_SRC_ROWS, cols)
    A, UPD = I(a), I(upd)
    st = _stream()
    for extra in (0, 3, 4):
        layout = f"{(cols + 255) // 256} pass(es), ld {'tight' if extra == 0 else '+ ' + str(extra)}"
        SRC = I(src, cols + extra)
        for given in (False, True):
            out = O(IDX_ROWS, cols)
            name = f"gather_rows cols={cols} ld_src={cols + extra} a={'given' if given else 'null'}"
            _ok(lib.zett_op_gather_rows_f32(A.ptr() if given else NULL, SRC.ptr(), cols + extra, C.c_void_p(IDX.data_ptr()), out.ptr(), IDX_ROWS, cols, st), name)
            tc.exact(out.back(name), (a if given else torch.zeros_like(a)) + src[idx.long()], name, key=("gather_rows", layout))
        dst = O(IDX_SRC_ROWS, cols, cols + extra, values=dst0)
        name = f"scatter_add_rows cols={cols} ld_dst={cols + extra}"
        _ok(lib.zett_op_scatter_add_rows_f32(dst.ptr(), cols + extra, C.c_void_p(IDX.data_ptr()), UPD.ptr(), IDX_ROWS, cols, st), name)
        ref, bnd = tc.scatter_add_ref(dst0, idx, upd)
        tc.check(dst.back(name), ref, bnd, name, key=("scatter_add_rows", layout), slice_rel=tc.REL_SUM)


@gpu
@pytest.mark.parametrize("e_in", IDX_COLS)
@pytest.mark.parametrize("src_kind", ("f32", "f16", "bf16"))
def test_source_gather_forward_and_backward(src_kind, e_in):
    """x[t] = id < v0 ? sw * src[id] + sb : fallback[id - v0] with ids at 0, v0 - 1, v0 and v0 + n_fallback - 1, with and without the
    rescaler; the backward's prod and keep per element and dfallback under the any-order sum bound"""
    L_, lib = _lib()
    dtype, code = {"f32": (F32, L_.DTYPE_F32), "f16": (torch.float16, L_.DTYPE_F16), "bf16": (torch.bfloat16, L_.DTYPE_BF16)}[src_kind]
    g = torch.Generator().manual_seed(e_in)
    ids = gather_ids()
    assert set(GATHER_EDGE_IDS) <= set(ids.tolist())
    IDS = ids.to(DEV)
    src = _randn(g, GATHER_V0, e_in).to(dtype)
    fb, sw, sb, dx, dfb0 = _randn(g, GATHER_FB, e_in), _randn(g, e_in), _randn(g, e_in), _randn(g, GATHER_T, e_in), _randn(g, GATHER_FB, e_in)
    SRC, FB, SW, SB, DX = I(src), I(fb), I(sw), I(sb), I(dx)
    st = _stream()
    layout = f"{src_kind} source, {(e_in + 255) // 256} pass(es)"
    for scaled in (False, True):
        x = O(GATHER_T, e_in)
        name = f"gather_fwd {src_kind} e_in={e_in} sw={'given' if scaled else 'null'}"
        _ok(lib.zett_op_gather_fwd_f32(C.c_void_p(IDS.data_ptr()), GATHER_T, SRC.ptr(), code, e_in, GATHER_V0, FB.ptr(), SW.ptr() if scaled else NULL, SB.ptr() if scaled else NULL, x.ptr(), st), name)
        ref, bnd = tc.gather_fwd_ref(ids, src, GATHER_V0, fb, sw if scaled else None, sb if scaled else None)
        tc.check(x.back(name), ref, bnd, name, key=("gather_fwd" + (" rescaled" if scaled else ""), layout), slice_rel=tc.REL_SUM)
    dfb, prod, keep = O(GATHER_FB, e_in, values=dfb0), O(GATHER_T, e_in), O(GATHER_T, e_in)
    name = f"gather_bwd {src_kind} e_in={e_in}"
    _ok(lib.zett_op_gather_bwd_f32(C.c_void_p(IDS.data_ptr()), GATHER_T, SRC.ptr(), code, e_in, GATHER_V0, DX.ptr(), dfb.ptr(), prod.ptr(), keep.ptr(), st), name)
    ref = tc.gather_bwd_ref(ids, src, GATHER_V0, GATHER_FB, dx, dfb0)
    tc.exact(prod.back(name + " prod"), ref["prod"], name + " prod", key=("gather_bwd prod", layout))
    tc.exact(keep.back(name + " keep"), ref["keep"], name + " keep", key=("gather_bwd keep", layout))
    tc.check(dfb.back(name + " dfallback"), ref["dfallback"], ref["b_dfallback"], name + " dfallback", key=("gather_bwd dfallback", layout), slice_rel=tc.REL_SUM)


# ---- rowdot, colsum ----------------------------------------------------------------------------------------------------------
@gpu
def test_rowdot_and_colsum():
    """rowdot over one and several passes of its column loop, ld tight and + 4, with and without the scalar; colsum over 1, 63, 64,
    65 and 1000 rows, overwriting and accumulating onto an output that is not zero"""
    _, lib = _lib()
    st = _stream()
    for rows, cols in ROWDOT_SHAPES:
        g = torch.Generator().manual_seed(rows * cols)
        a, w, b, out0 = _randn(g, rows, cols), _randn(g, cols), _randn(g, 1), _randn(g, cols)
        W, B = I(w), I(b)
        for extra in (0, 4):
            A = I(a, cols + extra)
            layout = f"{(cols + 255) // 256} pass(es), ld {'tight' if extra == 0 else '+ 4'}"
            for given in (False, True):
                out = O(None, rows)
                name = f"rowdot [{rows}, {cols}] ld={cols + extra} b={'given' if given else 'null'}"
                _ok(lib.zett_op_rowdot_f32(A.ptr(), cols + extra, W.ptr(), B.ptr() if given else NULL, out.ptr(), rows, cols, st), name)
                ref, bnd = tc.rowdot_ref(a, w, b if given else None)
                tc.check(out.back(name), ref, bnd, name, key=("rowdot", layout), slice_rel=tc.REL_SUM)
            for acc in (0, 1):
                out = O(None, cols, values=out0)
                name = f"colsum [{rows}, {cols}] ld={cols + extra} accumulate={acc}"
                _ok(lib.zett_op_colsum_f32(A.ptr(), cols + extra, rows, cols, out.ptr(), acc, st), name)
                ref, bnd = tc.colsum_ref(a, out0 if acc else None)
                tc.check(out.back(name), ref, bnd, name, key=("colsum", layout + f", accumulate {acc}"), slice_rel=tc.REL_SUM)
    for rows in COLSUM_ROWS:
        g = torch.Generator().manual_seed(rows)
        a, out0 = _randn(g, rows, 70), _randn(g, 70)
        A = I(a, 74)
        for acc in (0, 1):
            out = O(None, 70, values=out0)
            name = f"colsum [{rows}, 70] ld=74 accumulate={acc}"
            _ok(lib.zett_op_colsum_f32(A.ptr(), 74, rows, 70, out.ptr(), acc, st), name)
            ref, bnd = tc.colsum_ref(a, out0 if acc else None)
            tc.check(out.back(name), ref, bnd, name, key=("colsum", f"{rows} rows, accumulate {acc}"), slice_rel=tc.REL_SUM)
