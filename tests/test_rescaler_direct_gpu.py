"""zett_op_col_moments and zett_op_rescaler_fit (zett_amd/csrc/train_init.hip) called one launch at a time and checked ELEMENT BY
ELEMENT against float64 on the same values (tests/rescaler_check.py): rows around the chunk length, widths around the 16-byte vector,
first columns and leading dimensions that keep and break the alignment, the three element types, accumulation over unequal calls,
and the columns the formula E[x^2] - mean^2 fails on.

Buffers as in tests/test_rowops_direct_gpu.py: the matrix is a [rows, cols] view inside a larger allocation whose every other element
— the columns in front of col0 and behind col0 + cols, 256 rows before and after — is NaN, so a value read from outside poisons the
moments; state, workspace, w and b lie in canary frames, so a store outside them shows.  Nothing here is meant to fault.
"""
import ctypes as C

import pytest
import torch

from tests import rescaler_check as rk
from tests import train_ops_check as tc

DEV = "cuda:0"
gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
NULL = C.c_void_p(0)
INIT_RANGE = 0.02


@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = rk.record_path()          # figures for profiles/rescaler_check.md
    if path:
        rk.write_record(path)


def _lib():
    from zett_amd import _lib
    return _lib, _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


class Op:
    """a Frame on the device: .t the whole allocation, .p the pointer of the view"""

    def __init__(self, frame):
        self.f, self.t = frame, frame.buf.to(DEV)
        self.p = C.c_void_p(self.t.data_ptr() + frame.byte_offset())

    def back(self):
        return self.t.cpu()


def vec(n):
    """n fp32 words of output in a canary frame (a state of c columns is 6 c words, read back as doubles)"""
    return Op(tc.Frame(None, n, n, F32, "canary"))


def state_of(op, cols, what):
    """after the synchronize: the canary intact around the state -> [cols, 3] float64"""
    buf = op.back()
    tc.check_slack(op.f, buf, what)
    s = op.f.view(buf).contiguous().view(F64).reshape(cols, 3).clone()
    assert torch.isfinite(s).all(), (what, "a state element is not finite (not written?)")
    return s


def moments(lib, L, x, col0, ld, kind, state, accumulate=0, extra=0):
    """One zett_op_col_moments over the [rows, cols] values x, placed at column col0 of a matrix of leading dimension ld whose base is
    `extra` elements off the allocation's alignment.  The workspace is framed and checked too."""
    rows, cols = x.shape
    op = Op(tc.Frame(rows, cols, ld, rk.DT[kind], float("nan"), shift=col0 + extra, values=x)) if rows else None
    es = 4 if kind == "f32" else 2
    base = C.c_void_p(op.t.data_ptr() + op.f.byte_offset() - col0 * es) if rows else C.c_void_p(state.t.data_ptr())
    need = C.c_int64(0)
    assert lib.zett_op_col_moments_workspace_bytes(rows, cols, C.byref(need)) == 0
    ws = vec(need.value // 4)
    rc_ = lib.zett_op_col_moments(base, {"f32": L.DTYPE_F32, "f16": L.DTYPE_F16, "bf16": L.DTYPE_BF16}[kind], ld, rows, col0, cols, state.p, accumulate, ws.p, need.value,
                                  _stream())
    assert rc_ == 0, lib.zett_last_error().decode()
    torch.cuda.synchronize()
    tc.check_slack(ws.f, ws.back(), "col_moments workspace")
    return op


def fit(lib, cols, x_state, t_state=None, t_std=0.0, t_mean=0.0, expect=0):
    w, b = vec(cols), vec(cols)
    rc_ = lib.zett_op_rescaler_fit(x_state.p, cols, t_state.p if t_state is not None else NULL, t_std, t_mean, w.p, b.p, _stream())
    assert rc_ == expect, (rc_, lib.zett_last_error().decode())
    torch.cuda.synchronize()
    if expect:          # refused: nothing was launched, both outputs still hold the canary everywhere
        for o in (w, b):
            assert not o.f.overwritten(o.back()) and not torch.isfinite(o.f.view(o.back())).any()
        return None, None
    out = []
    for o, name in ((w, "w"), (b, "b")):
        buf = o.back()
        tc.check_canary(o.f, buf, f"rescaler_fit {name}")
        out.append(o.f.view(buf).clone())
    return out


def bits(s):
    return s.contiguous().view(torch.int64)


@gpu
@pytest.mark.parametrize("case", rk.pairwise_cases(), ids=lambda c: "x".join(map(str, c)))
def test_col_moments_and_scalar_fit(case):
    rows, cols, col0, kind, ld = case
    L, lib = _lib()
    i = rk.pairwise_cases().index(case)
    extra = 1 if i % 5 == 0 else 0          # every fifth case: the matrix's base pointer is one element off 16 bytes as well
    x = rk.case_values(rows, col0 + cols, kind)[:, col0:]
    key = ("col_moments", f"{kind} {'aligned' if (col0 * x.element_size()) % 16 == 0 and (ld * x.element_size()) % 16 == 0 and not extra else 'unaligned'}")
    st = vec(6 * cols)
    moments(lib, L, x, col0, ld, kind, st, extra=extra)
    s1 = state_of(st, cols, f"col_moments {case}")
    rk.check_moments(f"col_moments {case}", rk.state_dict_of(s1), x, key=key)
    # the same launch again, into a fresh state: the same bits
    st2 = vec(6 * cols)
    moments(lib, L, x, col0, ld, kind, st2, extra=extra)
    assert torch.equal(bits(state_of(st2, cols, "second launch")), bits(s1)), case
    # in_scaler's form of the fit: scalars for every column
    w, b = fit(lib, cols, st, t_std=INIT_RANGE, t_mean=0.0)
    ref = rk.moments_ref(x)
    bw, bb = rk.fit_bound(ref, rk.moments_bound(x, ref), target_std=INIT_RANGE, target_mean=0.0)
    w64, b64 = rk.scale_to_ref(x, target_stds=torch.full((cols,), INIT_RANGE, dtype=F64), target_means=torch.zeros(cols, dtype=F64))
    rk.check(w, w64[0], bw, f"rescaler_fit w {case}", key=("rescaler_fit", "scalars w"))
    rk.check(b, b64[0], bb, f"rescaler_fit b {case}", key=("rescaler_fit", "scalars b"))


@gpu
@pytest.mark.parametrize("kind", rk.KINDS)
def test_accumulation_over_three_unequal_calls(kind):
    L, lib = _lib()
    cols, col0, ld = 9, 3, 16
    x = rk.case_values(2 * rk.CHUNK + 1, col0 + cols, kind, seed=3)[:, col0:]
    cuts = [x[:70], x[70:70], x[70:]]          # 70 rows, none, 443: unequal, one empty, none a multiple of the chunk

    def three_calls():
        st = vec(6 * cols)
        for n, part in enumerate(cuts):
            moments(lib, L, part, col0, ld, kind, st, accumulate=int(n > 0))
        return state_of(st, cols, f"three calls {kind}")

    s = three_calls()
    rk.check_moments(f"col_moments three calls {kind}", rk.state_dict_of(s), x, key=("col_moments", f"{kind} accumulated"))
    assert torch.equal(bits(three_calls()), bits(s)), "the same three calls gave other bits"
    # One call over the concatenation is within the bound too.  It need NOT be the same bits: the chunks start at other rows (the
    # result depends on how a caller cuts the rows into calls, include/zett_hip.h), so equality is not asserted.
    st = vec(6 * cols)
    moments(lib, L, x, col0, ld, kind, st)
    rk.check_moments(f"col_moments one call {kind}", rk.state_dict_of(state_of(st, cols, "one call")), x, key=("col_moments", f"{kind} one call"))


@gpu
def test_empty_calls_and_the_refused_fit():
    L, lib = _lib()
    cols = 8
    x = rk.case_values(65, cols, "f32", seed=4)
    st = vec(6 * cols)
    moments(lib, L, x[:0], 0, cols, "f32", st)                      # rows = 0, accumulate = 0: the empty state
    assert not state_of(st, cols, "empty state").any()
    fit(lib, cols, st, t_std=INIT_RANGE, t_mean=0.0, expect=L.E_INVALID)
    assert "count 0" in lib.zett_last_error().decode()
    full = vec(6 * cols)
    moments(lib, L, x, 0, cols, "f32", full)
    fit(lib, cols, full, t_state=st, expect=L.E_INVALID)             # an empty TARGET is refused as well
    before = state_of(full, cols, "full")
    moments(lib, L, x[:0], 0, cols, "f32", full, accumulate=1)      # rows = 0, accumulate = 1: untouched
    assert torch.equal(bits(state_of(full, cols, "after an empty accumulate")), bits(before))
    moments(lib, L, x, 0, cols, "f32", st, accumulate=1)            # rows onto the empty state: the rows' own moments, bit for bit
    assert torch.equal(bits(state_of(st, cols, "onto empty")), bits(before))


@gpu
@pytest.mark.parametrize("kind", rk.KINDS)
def test_special_columns(kind):
    """mean 3 / std 0.01 within the bound (E[x^2] - mean^2 is 3.3 bounds off there, tests/test_rescaler_check_host.py); a constant column
    with M2 and std exactly 0 and the reference's own w = t_std / 1e-8; f16 values next to 65504 with finite moments."""
    L, lib = _lib()
    x = rk.special_values(kind)
    cols = x.shape[1]
    st = vec(6 * cols)
    moments(lib, L, x, 0, cols, kind, st)
    s = state_of(st, cols, f"special {kind}")
    got = rk.state_dict_of(s)
    rk.check_moments(f"col_moments special {kind}", got, x, key=("col_moments", f"{kind} special"))
    assert float(got["m2"][1]) == 0.0 and float(got["std"][1]) == 0.0 and float(got["mean"][1]) == float(x[0, 1])
    assert torch.isfinite(s).all()
    if kind == "f16":
        assert float(got["mean"][3]) > 65000.0
    w, b = fit(lib, cols, st, t_std=INIT_RANGE, t_mean=0.0)
    assert float(w[1]) == float(torch.tensor(INIT_RANGE / 1e-8, dtype=F32))
    ref = rk.moments_ref(x)
    bw, bb = rk.fit_bound(ref, rk.moments_bound(x, ref), target_std=INIT_RANGE, target_mean=0.0)
    w64, b64 = rk.scale_to_ref(x, target_stds=torch.full((cols,), INIT_RANGE, dtype=F64), target_means=torch.zeros(cols, dtype=F64))
    rk.check(w, w64[0], bw, f"rescaler_fit w special {kind}", key=("rescaler_fit", "special w"))
    rk.check(b, b64[0], bb, f"rescaler_fit b special {kind}", key=("rescaler_fit", "special b"))


@gpu
@pytest.mark.parametrize("kind,cols", [("f32", 7), ("bf16", 257), ("f16", 64)])
def test_fit_against_a_target_state(kind, cols):
    """scaler's form of the fit: the target's std and mean from a second state — here a column range of a wider state, the way
    init_rescaler takes the targets out of the source matrix's moments"""
    L, lib = _lib()
    x = rk.case_values(97, cols, "f32", seed=5)                      # predictions are fp32
    t_all = rk.case_values(2 * rk.CHUNK + 1, 8 + cols, kind, seed=6)
    sx, st = vec(6 * cols), vec(6 * (8 + cols))
    moments(lib, L, x, 0, cols, "f32", sx)
    moments(lib, L, t_all, 0, 8 + cols, kind, st)
    t = t_all[:, 8:]
    view = Op.__new__(Op)
    view.p = C.c_void_p(st.p.value + 8 * 24)                         # columns [8, 8 + cols) of the state: 24 bytes per column
    w, b = fit(lib, cols, sx, t_state=view)
    xr, tr = rk.moments_ref(x), rk.moments_ref(t)
    bw, bb = rk.fit_bound(xr, rk.moments_bound(x, xr), tr, rk.moments_bound(t, tr))
    w64, b64 = rk.scale_to_ref(x, t)
    rk.check(w, w64[0], bw, f"rescaler_fit w target {kind}", key=("rescaler_fit", "target w"))
    rk.check(b, b64[0], bb, f"rescaler_fit b target {kind}", key=("rescaler_fit", "target b"))
    w2, b2 = fit(lib, cols, sx, t_state=view)
    assert torch.equal(w2.view(torch.int32), w.view(torch.int32)) and torch.equal(b2.view(torch.int32), b.view(torch.int32))


@gpu
def test_python_surface_matches_the_direct_calls():
    """training.column_moments / rescaler_fit: the same bits as the entry points, ranges as views, accumulation through state="""
    from zett_amd import training
    x = rk.case_values(2 * rk.CHUNK + 1, 24, "bf16", seed=7).to(DEV)
    m = training.column_moments(x)
    assert m.state.shape == (24, 3) and m.state.dtype == F64 and m.count.dtype == m.mean().dtype == m.std().dtype == F32
    rk.check_moments("training.column_moments", rk.state_dict_of(m.state), x.cpu())
    part = training.column_moments(x, col0=3, cols=9)
    assert torch.equal(bits(part.state.cpu()), bits(m.columns(3, 12).state.cpu()))          # the result does not depend on col0
    acc = training.column_moments(x[:70], col0=3, cols=9)
    assert training.column_moments(x[70:], col0=3, cols=9, state=acc) is acc
    rk.check_moments("training.column_moments accumulated", rk.state_dict_of(acc.state), x.cpu()[:, 3:12])
    w, b = training.rescaler_fit(part, target_std=INIT_RANGE, target_mean=0.0)
    assert w.shape == b.shape == (1, 9) and w.dtype == b.dtype == F32
    w2, b2 = training.rescaler_fit(m.columns(3, 12), m.columns(12, 21))
    w64, b64 = rk.scale_to_ref(x.cpu()[:, 3:12], x.cpu()[:, 12:21])
    assert torch.allclose(w2.cpu().double(), w64, rtol=1e-5) and torch.allclose(b2.cpu().double(), b64, rtol=1e-4, atol=1e-6)
    with pytest.raises(ValueError, match="count 0"):
        training.rescaler_fit(training.column_moments(x[:0]), target_std=1.0, target_mean=0.0)
