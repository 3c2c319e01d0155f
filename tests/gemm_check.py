"""Element-by-element check of a GEMM result against float64 on the SAME operand values (no GPU in here).

    out[m, n] = act(a[m, :] . w[n, :] + bias[n]) + residual[m, n]

`reference` computes the contraction in float64 torch on the CPU from exactly the tensors the kernel is given (16-bit operands
are made on the host with .to(torch.bfloat16 / torch.float16) and upcast here), so the only thing that separates the two sides is
the kernel's fp32 accumulation and fp32 epilogue.  `check` holds the result to

  * a worst-case PER-ELEMENT bound, derived and not measured: fp32 accumulation of k products with one rounding per operation,
    plus the bias add, gives |err(z)| <= (k + 2) * 2^-23 * mag with mag = |a| . |w|^T + |bias|  (2^-23 rather than the unit
    round-off 2^-24: the bound holds whichever way the MFMA's adder rounds).  A residual adds 2^-23 * (|act(z)| + |residual|).
    Behind a GELU the allowance of z passes through the GELU's Lipschitz constant (1.13) and the activation's own allowance is
    added: 1e-6 absolute, the limit test_layernorm_gelu_rowops_match_torch holds the same gelu_tanh_f / gelu_erf_f formulas
    to (valid for |z| <~ 10, which the operand scales of the tests keep);
  * rel-L2 <= 2e-6 of EVERY ROW and EVERY COLUMN (the project's limit for its fp32 GEMMs, applied to slices so that one bad row
    or column cannot hide in the norm of the matrix; the same in the 16-bit modes, because on identical operands only the fp32
    accumulation separates the two sides).  Behind a GELU, slices whose reference norm is below 1e-3 are held by the per-element
    bound alone; they may be at most 2 % of the slices of a case, which is asserted.  A slice of ONE element (the columns of an
    m = 1 case) is that element's relative error, which cancellation in a . w makes arbitrarily large for any correct fp32
    kernel: such a slice is an element, not a norm something could hide in, and is held by the per-element bound alone.

A failure is a GemmMismatch that names the worst (row, column), both values and the bound, and carries the mask of elements over
their bound and the lists of rows / columns over the slice limit.

`emulate` is the fp32 arithmetic the limits were sized against: K accumulated in chunks of 4 (products and the sum of a chunk
exact, one fp32 rounding per chunk), fp32 epilogue.  Up to K = 2112 it stays below 6e-7 slice rel-L2, a quarter of the limit, and
below 0.04 of the per-element bound in all three operand types (tests/test_gemm_check_host.py asserts the latter and that it
passes).

`Framed` is the buffer discipline of the direct GPU test: every operand and output is a view inside a larger allocation with a
full tile of slack on both sides, the slack filled with NaN (inputs) or a canary bit pattern (outputs).
"""
from __future__ import annotations

import json
import os

import torch
import torch.nn.functional as F

U = 2.0 ** -23              # one fp32 ulp at 1: twice the unit round-off
GELU_LIPSCHITZ = 1.13       # max |gelu'| (1.129 for both forms)
ACT_ABS = 1e-6              # allowance of gelu_tanh_f / gelu_erf_f themselves
SLICE_REL = 2e-6
SMALL_NORM = 1e-3           # act != 0: slices below this reference norm are held per element only ...
SMALL_SHARE = 0.02          # ... and may be at most this share of a case's slices
LO_DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
K_STEP = {"f32": 32, "bf16": 64, "f16": 64}      # contraction widths are multiples of this (128 bytes of K)
SLACK_ROWS = 256            # one full tile
SLACK_VEC = 256
CANARY_BITS = 0x7FC5A5A5    # a quiet NaN with a payload no kernel produces: an element that was not written is not finite


class GemmMismatch(AssertionError):
    """bad: bool [m, n], True where |got - ref| exceeds the element's bound (or got is not finite); rows / cols: the slices over
    SLICE_REL; row, col: the worst element (largest err / bound)."""

    def __init__(self, msg, bad, rows, cols, row, col):
        super().__init__(msg)
        self.bad, self.rows, self.cols, self.row, self.col = bad, rows, cols, row, col


def _gelu(z, act):
    if act == 1:
        return F.gelu(z, approximate="tanh")
    if act == 2:
        return F.gelu(z)
    return z


def products(a, w):
    """-> (a . w^T, |a| . |w|^T) in float64: the part of a reference every epilogue of the same operands shares"""
    a64, w64 = a.detach().cpu().double(), w.detach().cpu().double()
    return a64 @ w64.T, a64.abs() @ w64.abs().T


def reference(a, w, bias=None, act=0, residual=None, prod=None):
    """-> dict(z, y, mag, act_z, residual) in float64, from the operand values as they are (prod: products(a, w), if at hand)."""
    z, mag = products(a, w) if prod is None else prod
    if bias is not None:
        b64 = bias.detach().cpu().double()
        z = z + b64
        mag = mag + b64.abs()
    act_z = _gelu(z, act)
    r64 = None if residual is None else residual.detach().cpu().double()
    y = act_z if r64 is None else act_z + r64
    return dict(z=z, y=y, mag=mag, act_z=act_z, residual=r64)


def sub_reference(ref, m, n):
    """the reference of the leading [m, n] block (rows of a, rows of w, leading bias and residual: the same contraction)"""
    return {key: (None if v is None else v[:m, :n]) for key, v in ref.items()}


def bound(ref, k, act):
    b = (k + 2) * U * ref["mag"]
    if act != 0:
        b = GELU_LIPSCHITZ * b + ACT_ABS
    if ref["residual"] is not None:
        b = b + U * (ref["act_z"].abs() + ref["residual"].abs())
    return b


RECORD = {}      # (operand type, k, tile) -> [worst err / bound, worst slice rel-L2, cases]


def _note(key, ratio, rel):
    if key is None:
        return
    r = RECORD.setdefault(tuple(key), [0.0, 0.0, 0])
    r[0], r[1], r[2] = max(r[0], ratio), max(r[1], rel), r[2] + 1


def write_record(path):
    """the largest observed err / bound and slice rel-L2 per (operand type, K, tile): figures for profiles/gemm_direct_check.md,
    no limit depends on them"""
    rows = [dict(type=t, k=k, tile=tile, err_over_bound=v[0], slice_rel_l2=v[1], cases=v[2]) for (t, k, tile), v in sorted(RECORD.items())]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rows, f, indent=1)


def measure(got, ref, k, act):
    """-> (err [m, n], bound [m, n], row rel-L2 [m], column rel-L2 [n], held rows (bool), held columns (bool))"""
    y = ref["y"]
    g = got.detach().cpu().double()
    assert g.shape == y.shape, (g.shape, y.shape)
    err = (g - y).abs()
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, float("inf")))
    bnd = bound(ref, k, act)
    out = [err, bnd]
    held = []
    for dim in (1, 0):
        norm = y.norm(dim=dim)
        e = torch.where(torch.isfinite(g), g - y, torch.zeros_like(y)).norm(dim=dim)
        keep = torch.ones_like(norm, dtype=torch.bool)
        if act != 0:
            keep &= norm >= SMALL_NORM
        if y.shape[dim] == 1:
            keep &= False                       # one-element slices: the per-element bound alone (see the module docstring)
        out.append(torch.where(keep, e / norm.clamp_min(1e-300), torch.zeros_like(e)))
        held.append(keep)
    return (*out, *held)


def check(got, ref, k, act, what, key=None):
    """Assert the per-element bound and the slice limits (see the module docstring); key = (operand type, k, tile) files the
    observed margins under RECORD."""
    err, bnd, rel_r, rel_c, keep_r, keep_c = measure(got, ref, k, act)
    m, n = err.shape
    if act != 0:
        for keep, size, name in ((keep_r, n, "rows"), (keep_c, m, "columns")):
            if size > 1:
                share = 1.0 - float(keep.double().mean())
                assert share <= SMALL_SHARE, f"{what}: {share:.1%} of the {name} have a reference norm below {SMALL_NORM}: the case is scaled wrongly"
    ratio = err / bnd
    worst = int(torch.argmax(ratio))
    row, col = worst // n, worst % n
    bad = err > bnd
    rows = torch.nonzero(rel_r > SLICE_REL).flatten().tolist()
    cols = torch.nonzero(rel_c > SLICE_REL).flatten().tolist()
    top_ratio, top_rel = float(ratio.max()), max(float(rel_r.max()), float(rel_c.max()))
    if not bool(bad.any()) and not rows and not cols:
        _note(key, top_ratio, top_rel)
        return top_ratio, top_rel
    g = got.detach().cpu().double()
    msg = [f"{what}: [{m}, {n}] k={k} act={act}"]
    if bool(bad.any()):
        msg.append(f"{int(bad.sum())} element(s) over their bound; worst at (row {row}, column {col}): got {float(g[row, col])!r}, "
                   f"reference {float(ref['y'][row, col])!r}, |err| {float(err[row, col]):.3e} > bound {float(bnd[row, col]):.3e}")
    if rows:
        r = max(rows, key=lambda i: float(rel_r[i]))
        msg.append(f"{len(rows)} row(s) over rel-L2 {SLICE_REL:.0e}: worst row {r} at {float(rel_r[r]):.3e} (first {rows[:8]})")
    if cols:
        c = max(cols, key=lambda i: float(rel_c[i]))
        msg.append(f"{len(cols)} column(s) over rel-L2 {SLICE_REL:.0e}: worst column {c} at {float(rel_c[c]):.3e} (first {cols[:8]})")
    if not bool(bad.any()):
        msg.append(f"largest err / bound {top_ratio:.3f} at (row {row}, column {col}): got {float(g[row, col])!r}, reference {float(ref['y'][row, col])!r}")
    raise GemmMismatch("; ".join(msg), bad, rows, cols, row, col)


def emulate_acc(a, w, chunk=4):
    """a . w^T in emulated fp32 accumulation: K in chunks of `chunk`, a chunk's products and their sum exact, then ONE fp32 rounding
    into the accumulator"""
    a64, w64 = a.detach().cpu().double(), w.detach().cpu().double()
    acc = torch.zeros(a64.shape[0], w64.shape[0], dtype=torch.float32)
    for c in range(0, a64.shape[1], chunk):
        acc = (acc.double() + a64[:, c:c + chunk] @ w64[:, c:c + chunk].T).float()
    return acc


def emulate_epilogue(acc, bias=None, act=0, residual=None):
    """the fp32 epilogue of the kernels on an fp32 accumulator: + bias, GELU, + residual, each rounded to fp32"""
    v = acc if bias is None else acc + bias.detach().cpu().float()
    v = _gelu(v, act)
    return v if residual is None else v + residual.detach().cpu().float()


def emulate(a, w, bias=None, act=0, residual=None, chunk=4):
    return emulate_epilogue(emulate_acc(a, w, chunk), bias, act, residual)


def operands(kind, m, n, k, seed, lda=None, ldw=None):
    """The operand scales of the direct tests: a ~ N(0, 1), w ~ N(0, 1) * 3 / sqrt(k) (z has a standard deviation of 3: |z| <~ 10
    for the GELUs), bias ~ 0.5 N(0, 1), residual ~ N(0, 1); a and w rounded to the operand type on the host."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(m, k, generator=g).to(LO_DTYPES[kind])
    w = (torch.randn(n, k, generator=g) * (3.0 / k ** 0.5)).to(LO_DTYPES[kind])
    bias = 0.5 * torch.randn(n, generator=g)
    residual = torch.randn(m, n, generator=g)
    return a, w, bias, residual


# ---- buffers of the direct GPU test ----------------------------------------------------------------------------------
class Framed:
    """A [rows, cols] matrix with leading dimension ld (or, rows = None, a vector of cols elements) that lies INSIDE a larger
    allocation: SLACK_ROWS rows of ld elements (SLACK_VEC elements for a vector) before and after it, `shift` further elements
    in front to move the base pointer.  The slack — and the columns cols .. ld - 1 of every row — holds `fill`: NaN for what
    a kernel only reads, the canary for what it writes.  `buf` is the whole allocation (host), `offset` the first element of the
    view; after .to(device) the kernel gets data_ptr() + offset * itemsize."""

    def __init__(self, rows, cols, ld, dtype, fill, shift=0, values=None):
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        assert ld >= cols and shift >= 0
        if rows is None:
            self.offset = SLACK_VEC + shift
            total = self.offset + cols + SLACK_VEC
        else:
            self.offset = SLACK_ROWS * ld + shift
            total = self.offset + (rows + SLACK_ROWS) * ld
        if fill == "canary":
            assert dtype == torch.float32
            self.buf = torch.full((total,), CANARY_BITS, dtype=torch.int32).view(torch.float32)
        else:
            self.buf = torch.full((total,), float(fill), dtype=dtype)
        if values is not None:
            self.view(self.buf).copy_(values)

    def view(self, buf):
        """the [rows, cols] (or [cols]) view of an allocation laid out like self.buf (the host buffer, or a copy brought back)"""
        if self.rows is None:
            return buf[self.offset:self.offset + self.cols]
        return buf[self.offset:self.offset + self.rows * self.ld].view(self.rows, self.ld)[:, :self.cols]

    def byte_offset(self):
        return self.offset * self.buf.element_size()

    def overwritten(self, buf):
        """-> the (row, column) positions, relative to the view's first element, of the elements outside the view whose bits differ
        from the canary ([] = intact); a vector reports (0, index)"""
        bits = buf.detach().cpu().contiguous().view(torch.int32).clone()
        assert bits.numel() == self.buf.numel()
        self.view(bits).fill_(CANARY_BITS)
        rel = torch.nonzero(bits != CANARY_BITS).flatten() - self.offset
        if self.rows is None:
            return [(0, int(i)) for i in rel]
        return [(int(i) // self.ld, int(i) % self.ld) for i in rel]       # (floor division: rows in front of the view are negative)


class CanaryBroken(AssertionError):
    def __init__(self, msg, where):
        super().__init__(msg)
        self.where = where


def check_canary(frame, buf, what):
    """After a call: the canary bit-intact everywhere outside [rows, cols] — the columns cols .. ld - 1 of every row, the rows past
    the last, the slack in front — and every element inside finite (the canary is a NaN: an element that was not written fails)."""
    where = frame.overwritten(buf)
    if where:
        raise CanaryBroken(f"{what}: {len(where)} element(s) outside the [{frame.rows}, {frame.cols}] output (ld {frame.ld}) were overwritten, "
                           f"first at (row, column) {where[:4]}", where)
    inside = frame.view(buf.detach().cpu())
    finite = torch.isfinite(inside)
    if not bool(finite.all()):
        idx = torch.nonzero(~finite)[0].tolist()
        raise AssertionError(f"{what}: {int((~finite).sum())} output element(s) not finite (not written?), first at {idx}")
