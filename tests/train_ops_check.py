"""Element-by-element check of the training row primitives (zett_amd/csrc/train_{operands,layernorm,attention,gather}.hip) against float64 on the SAME values
(no GPU in here): the sibling of tests/gemm_check.py, whose buffer discipline (Framed, check_canary, CANARY_BITS) and unit U
it uses.

Every reference below is plain torch on the CPU, computed from exactly the tensors the kernel is given.  Each takes `dt`:
float64 is the reference, float32 is the EMULATION the limits are sized against — the same formulas in fp32 with every sum
taken strictly left to right (`_sum`: the last element of a cumulative sum).  tests/test_train_ops_check_host.py asserts that the
emulation stays below a quarter of every bound.

The bounds, all per element, derived and not measured (U = 2^-23, one fp32 ulp at 1, twice the unit round-off, so each holds
whichever way an adder rounds and whether or not a multiply-add is fused):

  * data movement (16-bit transposes, gather without an addend, fallback rows, copies, zero padding): bit equality (`exact`);
  * conversion of an fp32 value to bf16 / f16: bit equality with x.to(dtype), round to nearest even (`exact`);
  * a single IEEE operation: equality with the same operation in torch fp32 (`exact` on the fp32 result);
  * a multiply-add a * b + c that the compiler may or may not fuse: U * (|a b| + |c|)  (`fma_bound`: fused it rounds once, on a
    result no larger than |a b| + |c|; unfused the product and the sum round once each);
  * a sum of n fp32 terms IN ANY ORDER: (n + 2) * U * sum |terms|  (`sum_bound`: every partial sum is at most sum |terms| and is
    rounded once, n - 1 additions; the + 2 leaves room for one rounding of each term and of a final scale or addend).  Where the
    terms are themselves rounded products or carry an allowance of their own, that is added and said so at the function.  Order
    does not enter, which scatter_add_rows and gather_bwd's dfallback need: their float atomics are not order-stable;
  * a 16-bit operand made from fp32 arithmetic (gelu_fwd_lo, LayerNorm's y_lo, attention's ctx_lo, the plain / transposed copies of
    dy * gelu'(z)): `lo_bound` — the fp32 bound b of the value, plus half an ulp of the 16-bit type at the reference value, plus one
    more ulp where [ref - b, ref + b] contains a rounding boundary of the type (the two ends round to different values);
  * GELU: the project's absolute allowance ACT_ABS = 1e-6 of gelu_tanh_f / gelu_erf_f, 2e-6 for the derivative times |dh| plus one
    rounding, never more than 2e-6 (inputs keep |dh| <= 1 and |z| < 8: one fp32 ulp of the result then stays below half the allowance);
  * LayerNorm forward / backward, attention forward / backward: the sum bounds propagated through the formulas on the float64
    intermediates (the docstrings of layernorm_bound, layernorm_bwd_bound, attention_ref and attention_bwd_ref spell them out),
    times ONE explicit constant per op, C_LN_FWD, C_LN_BWD, C_ATT_FWD, C_ATT_BWD.  The rule for the constants: the largest
    err / bound observed on the device over every case of tests/test_train_ops_direct_gpu.py is at most 0.5 (a factor two over
    the reference arithmetic, for the reduction order the emulation does not model).  profiles/train_ops_check.md holds the
    observed ratios and the constants chosen from them.

On top of the per-element bound, `check` applies the project's whole-tensor limits to EVERY ROW and EVERY COLUMN separately
(slice_rel), so that one bad row or column cannot hide in the norm of the matrix; a slice of one element is that element and is
held by its bound alone, as in gemm_check.  `whole_rel` keeps the whole-tensor limit of tests/test_autograd_gpu.py where that is
the tighter figure.

A failure is an OpMismatch that names the op and case, the worst (row, column), both values and the bound.
"""
from __future__ import annotations

import json
import os

import torch
import torch.nn.functional as F

from tests.gemm_check import ACT_ABS, CANARY_BITS, U, CanaryBroken, Framed, check_canary      # noqa: F401 (re-exported for the tests)

F64, F32 = torch.float64, torch.float32
ACT_GRAD_ABS = 2e-6          # allowance of gelu_grad1 (tests/test_autograd_gpu.py holds the same formulas to it)
CANARY16 = 0x7FC5            # the upper half of CANARY_BITS: a quiet NaN in bf16 and in f16
LO = {"bf16": torch.bfloat16, "f16": torch.float16}
LO_P = {torch.bfloat16: (7, -126), torch.float16: (10, -14)}      # fraction bits, smallest normal exponent

# the constants of the four propagated bounds (see the module docstring and profiles/train_ops_check.md)
C_LN_FWD = 1.0
C_LN_BWD = 1.0
C_ATT_FWD = 1.0
C_ATT_BWD = 1.0

# the whole-tensor limits of tests/test_autograd_gpu.py, applied per slice here
REL_FWD, REL_LN_FWD, REL_BWD, REL_ATT_BWD, REL_PARAM, REL_SUM = 2e-6, 1e-6, 2e-5, 5e-6, 1e-5, 1e-6


class OpMismatch(AssertionError):
    """bad: bool [rows, cols], True where |got - ref| exceeds the element's bound (or got is not finite); rows / cols: the slices
    over the slice limit; row, col: the worst element (largest err / bound)."""

    def __init__(self, msg, bad, rows, cols, row, col):
        super().__init__(msg)
        self.bad, self.rows, self.cols, self.row, self.col = bad, rows, cols, row, col


# ---- the record ------------------------------------------------------------------------------------------------------
RECORD = {}      # (op, layout) -> [worst err / bound, worst slice rel-L2, cases]
RECORD_ENV = "ZETT_TRAIN_OPS_CHECK_RECORD"


def _note(key, ratio, rel):
    if key is None:
        return
    r = RECORD.setdefault(tuple(key), [0.0, 0.0, 0])
    r[0], r[1], r[2] = max(r[0], ratio), max(r[1], rel), r[2] + 1


def write_record(path):
    """the largest observed err / bound and slice rel-L2 per (op, layout): figures for profiles/train_ops_check.md"""
    rows = [dict(op=op, layout=layout, err_over_bound=v[0], slice_rel_l2=v[1], cases=v[2]) for (op, layout), v in sorted(RECORD.items())]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(rows, f, indent=1)


# ---- the two checks ----------------------------------------------------------------------------------------------------
def _as2d(t):
    return t.reshape(1, -1) if t.dim() < 2 else t.reshape(t.shape[0], -1)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.element_size() == 4 else t.view(torch.int16)


def exact(got, want, what, key=None):
    """bit equality (data movement, conversions, single IEEE operations: `want` is made by torch in the type of `got`)"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    g, w = _as2d(_bits(got)), _as2d(_bits(want))
    bad = g != w
    if not bool(bad.any()):
        _note(key, 0.0, 0.0)
        return
    row, col = torch.nonzero(bad)[0].tolist()
    gv, wv = _as2d(got.detach().cpu())[row, col], _as2d(want.detach().cpu())[row, col]
    rows, cols = torch.nonzero(bad.any(1)).flatten().tolist(), torch.nonzero(bad.any(0)).flatten().tolist()
    raise OpMismatch(f"{what}: {int(bad.sum())} element(s) differ in their bits; first at (row {row}, column {col}): got {float(gv)!r}, "
                     f"expected {float(wv)!r} (bound: equality)", bad, rows, cols, row, col)


def check(got, ref, bnd, what, key=None, slice_rel=None, whole_rel=None):
    """|got - ref| <= bnd per element (bnd = 0: equality of the values), every row and column of more than one element within
    slice_rel in rel-L2, the whole within whole_rel.  -> (largest err / bound, largest slice rel-L2)"""
    g, y, b = _as2d(got.detach().cpu().to(F64)), _as2d(ref.to(F64)), _as2d(bnd.to(F64))
    assert g.shape == y.shape == b.shape, (what, g.shape, y.shape, b.shape)
    fin = torch.isfinite(g)
    err = torch.where(fin, (g - y).abs(), torch.full_like(y, float("inf")))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    bad = err > b
    m, n = err.shape
    worst = int(torch.argmax(ratio))
    row, col = worst // n, worst % n
    rows, cols, top_rel, rel_r, rel_c = [], [], 0.0, None, None
    diff = torch.where(fin, g - y, torch.zeros_like(y))
    if slice_rel is not None:
        rel_r = diff.norm(dim=1) / y.norm(dim=1).clamp_min(1e-300) if n > 1 else torch.zeros(m, dtype=F64)
        rel_c = diff.norm(dim=0) / y.norm(dim=0).clamp_min(1e-300) if m > 1 else torch.zeros(n, dtype=F64)
        rel_r = torch.where(diff.norm(dim=1) == 0, torch.zeros_like(rel_r), rel_r) if n > 1 else rel_r
        rel_c = torch.where(diff.norm(dim=0) == 0, torch.zeros_like(rel_c), rel_c) if m > 1 else rel_c
        rows, cols = torch.nonzero(rel_r > slice_rel).flatten().tolist(), torch.nonzero(rel_c > slice_rel).flatten().tolist()
        top_rel = max(float(rel_r.max()), float(rel_c.max()))
    whole = float(diff.norm() / y.norm().clamp_min(1e-300)) if whole_rel is not None and float(diff.norm()) > 0 else 0.0
    top_ratio = float(ratio.max())
    if not bool(bad.any()) and not rows and not cols and (whole_rel is None or whole <= whole_rel):
        _note(key, top_ratio, top_rel)
        return top_ratio, top_rel
    msg = [f"{what}: [{m}, {n}]"]
    if bool(bad.any()):
        msg.append(f"{int(bad.sum())} element(s) over their bound; worst at (row {row}, column {col}): got {float(g[row, col])!r}, "
                   f"reference {float(y[row, col])!r}, |err| {float(err[row, col]):.3e} > bound {float(b[row, col]):.3e}")
    if rows:
        r = max(rows, key=lambda i: float(rel_r[i]))
        msg.append(f"{len(rows)} row(s) over rel-L2 {slice_rel:.0e}: worst row {r} at {float(rel_r[r]):.3e} (first {rows[:8]})")
    if cols:
        c = max(cols, key=lambda i: float(rel_c[i]))
        msg.append(f"{len(cols)} column(s) over rel-L2 {slice_rel:.0e}: worst column {c} at {float(rel_c[c]):.3e} (first {cols[:8]})")
    if whole_rel is not None and whole > whole_rel:
        msg.append(f"whole-tensor rel-L2 {whole:.3e} over {whole_rel:.0e}")
    if not bool(bad.any()):
        msg.append(f"largest err / bound {top_ratio:.3f} at (row {row}, column {col}): got {float(g[row, col])!r}, reference {float(y[row, col])!r}, "
                   f"bound {float(b[row, col]):.3e}")
    raise OpMismatch("; ".join(msg), bad, rows, cols, row, col)


# ---- building blocks ---------------------------------------------------------------------------------------------------
def _sum(x, dim):
    """float64: the sum; float32: the terms added strictly left to right in fp32 (the emulation)"""
    if x.dtype == F32:
        return x.cumsum(dim).select(dim, -1) if x.shape[dim] else x.sum(dim)
    return x.sum(dim)


def sum_bound(n, mag):
    """a sum of n fp32 terms in any order: (n + 2) U sum |terms|"""
    return (n + 2) * U * mag


def fma_bound(prod, addend):
    """a * b + c, fused or not: U (|a b| + |c|)"""
    return U * (prod.abs() + addend.abs())


def ulp_lo(x, dtype):
    """the spacing of `dtype` (bf16 / f16) at |x| (float64 in, float64 out; subnormals: the smallest spacing)"""
    p, emin = LO_P[dtype]
    e = torch.frexp(x.abs().to(F64).clamp_min(1e-300))[1].to(F64) - 1.0
    return torch.exp2(e.clamp_min(float(emin)) - p)


def lo_bound(ref, b32, dtype):
    """a 16-bit value made from an fp32 value that is within b32 of ref: b32 + ulp / 2, + 1 ulp where [ref - b32, ref + b32] holds
    a rounding boundary of the type (the rule of the module docstring, one place for gelu_fwd_lo, y_lo, ctx_lo and the gradient
    operands)"""
    ref, b32 = ref.to(F64), b32.to(F64)
    ulp = ulp_lo(ref, dtype)
    straddle = (ref - b32).to(dtype).to(F64) != (ref + b32).to(dtype).to(F64)
    return b32 + 0.5 * ulp + torch.where(straddle, ulp, torch.zeros_like(ulp))


def gelu(z, kind):
    """float64: torch's GELU; float32 (the emulation): the erf form written out, (z / 2) (1 + erf(z / sqrt 2)) — torch's own fp32 erf
    GELU on the CPU is off by more than 1e-6 near z = 3.4 and is no yardstick"""
    if kind == 1:
        return F.gelu(z, approximate="tanh")
    return F.gelu(z) if z.dtype == F64 else (z * 0.5) * (1.0 + torch.erf(z * 0.7071067811865476))


def gelu_grad(z, kind):
    """d gelu / dz in closed form, in the type of z"""
    if kind == 1:
        u = 0.7978845608028654 * (z + 0.044715 * z * z * z)
        t = torch.tanh(u)
        return 0.5 * (1.0 + t) + 0.5 * z * (1.0 - t * t) * 0.7978845608028654 * (1.0 + 3.0 * 0.044715 * z * z)
    return 0.5 * (1.0 + torch.erf(z * 0.7071067811865476)) + z * 0.3989422804014327 * torch.exp(-0.5 * z * z)


def gelu_bwd_ref(z, dh, kind, dt=F64):
    """-> (dz = dh * gelu'(z), bound): ACT_GRAD_ABS |dh| for the derivative plus one rounding of the product, at most ACT_GRAD_ABS
    (the limit the existing test holds the product to; |dh| <= 1 keeps the two the same to within U)"""
    v = dh.to(dt) * gelu_grad(z.to(dt), kind)
    return v, torch.minimum(ACT_GRAD_ABS * dh.to(F64).abs() + U * v.to(F64).abs(), torch.full_like(v, ACT_GRAD_ABS, dtype=F64))


# ---- transposes and conversions ------------------------------------------------------------------------------------------
def pad_rows(t, rows_padded):
    return torch.cat([t, torch.zeros(rows_padded - t.shape[0], t.shape[1], dtype=t.dtype)], 0)


def transpose_ref(x, rows_padded, dtype):
    """out[c, r] = dtype(x[r, c]), rows r >= R zero: exact (x fp32 or already 16-bit; dtype float32 for zett_op_transpose_f32)"""
    return pad_rows(x.to(dtype), rows_padded).T.contiguous()


def convert_ref(x, cols_padded, dtype):
    return torch.cat([x.to(dtype), torch.zeros(x.shape[0], cols_padded - x.shape[1], dtype=dtype)], 1)


def grad_operands_ref(dy, z, kind, dt=F64):
    """the value every result of zett_op_grad_operands_lo is made from: v = dy (exact, bound 0) or dy * gelu'(z) (gelu_bwd_ref's
    bound).  -> (v, b32)"""
    if z is None:
        return dy.to(dt), torch.zeros(dy.shape, dtype=F64)
    return gelu_bwd_ref(z, dy, kind, dt)


def colpart_ref(v, b32):
    """the column sums of each 64-row band: [ceil(R / 64), C], each a sum of at most 64 terms (sum_bound with n = 64: the kernel
    adds the band's 64 tile rows, zeros past R included) plus the allowances of the terms.  -> (sums, bound)"""
    bands = (v.shape[0] + 63) // 64
    s = torch.stack([_sum(v[64 * b:64 * b + 64], 0) for b in range(bands)])
    mag = torch.stack([v[64 * b:64 * b + 64].to(F64).abs().sum(0) for b in range(bands)])
    extra = torch.stack([b32[64 * b:64 * b + 64].sum(0) for b in range(bands)])
    return s, sum_bound(64, mag) + extra


# ---- sums ---------------------------------------------------------------------------------------------------------------
def colsum_ref(x, out0=None, dt=F64):
    """out[c] (+)= sum_r x[r, c]: R terms and the addend: (R + 3) U (sum |x| + |out0|)"""
    s = _sum(x.to(dt), 0) if x.shape[0] else torch.zeros(x.shape[1], dtype=dt)
    mag = x.to(F64).abs().sum(0)
    if out0 is not None:
        s, mag = s + out0.to(dt), mag + out0.to(F64).abs()
    return s, (x.shape[0] + 3) * U * mag


def rowdot_ref(a, w, b=None, dt=F64):
    """out[r] = a[r, :] . w + b: C products (each rounded, or fused into the sum) and the addend: (C + 3) U (|a| . |w| + |b|)"""
    s = _sum(a.to(dt) * w.to(dt), 1)
    mag = a.to(F64).abs() @ w.to(F64).abs()
    if b is not None:
        s, mag = s + b.to(dt)[0], mag + b.to(F64)[0].abs()
    return s, (a.shape[1] + 3) * U * mag


def scatter_add_ref(dst0, idx, src, dt=F64):
    """dst[idx[r]] += src[r]: a destination row hit n times is a sum of n + 1 terms in no fixed order: (n + 3) U (|dst0| + sum |src|)"""
    out = dst0.to(dt).clone()
    mag = dst0.to(F64).abs().clone()
    if dt == F32:
        for r, i in enumerate(idx.tolist()):
            out[i] += src[r].to(dt)
    else:
        out.index_add_(0, idx.long(), src.to(dt))
    mag.index_add_(0, idx.long(), src.to(F64).abs())
    hits = torch.bincount(idx.long(), minlength=dst0.shape[0]).to(F64)[:, None]
    return out, (hits + 3) * U * mag


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------
def f32_value(x):
    return float(torch.tensor(x, dtype=F32))


def layernorm_ref(x, gamma, beta, eps, dt=F64):
    """y = (x - mean) * rstd * gamma + beta, two-pass variance; -> dict(y, mean, rstd)"""
    x, g, b = x.to(dt), gamma.to(dt), beta.to(dt)
    h = x.shape[1]
    mean = _sum(x, 1) / h
    d = x - mean[:, None]
    rstd = 1.0 / torch.sqrt(_sum(d * d, 1) / h + f32_value(eps))
    return dict(y=d * rstd[:, None] * g + b, mean=mean, rstd=rstd)


def layernorm_bound(x, gamma, beta, eps, ref):
    """From the float64 intermediates, with d = x - mean:
        mean:  a sum of h terms and a division:                 bm = (h + 2) U sum |x| / h
        d:     inherits bm, one rounding:                       bd = bm + U |d|
        q = sum d^2: the terms move by 2 |d| bd, then the sum:   bq = sum 2 |d| bd + (h + 2) U sum d^2
        rstd = (q / h + eps)^-1/2: half the relative error of the variance (its own two roundings included), three roundings for
               the square root and the reciprocal:              br = rstd (0.5 (bq / h + 2 U var) / var + 3 U)
        y = fma(d rstd, gamma, beta):                           by = |gamma| (rstd bd + |d| br + U |d| rstd) + U (|y| + |beta|)
    each times C_LN_FWD.  -> dict(y, mean, rstd)"""
    x, g, b = x.to(F64), gamma.to(F64), beta.to(F64)
    h = x.shape[1]
    d = (x - ref["mean"].to(F64)[:, None]).abs()
    rstd = ref["rstd"].to(F64)
    var = 1.0 / (rstd * rstd)
    bm = (h + 2) * U * x.abs().sum(1) / h
    bd = bm[:, None] + U * d
    bq = (2 * d * bd).sum(1) + (h + 2) * U * (d * d).sum(1)
    br = rstd * (0.5 * (bq / h + 2 * U * var) / var + 3 * U)
    by = g.abs() * (rstd[:, None] * bd + d * br[:, None] + U * d * rstd[:, None]) + U * (ref["y"].to(F64).abs() + b.abs())
    return dict(y=C_LN_FWD * by, mean=C_LN_FWD * bm, rstd=C_LN_FWD * br)


def ln_part_rows(rows, n_part):
    """the rows workgroup b of the backward walks: b, b + n_part, ..."""
    return [list(range(b, rows, n_part)) for b in range(n_part)]


def layernorm_bwd_ref(dy, dy2, x, stats, gamma, n_part, dt=F64):
    """dx = rstd (g - mean(g) - xhat mean(g xhat)), g = (dy + dy2) gamma, xhat = (x - mean) rstd with mean, rstd = the `stats` the
    kernel is given; partials [n_part, 2, h]: the sums of (dy + dy2) xhat and of (dy + dy2) over the rows of each workgroup.
    -> dict(dx, partials)"""
    d = dy.to(dt) if dy2 is None else dy.to(dt) + dy2.to(dt)
    x, g0, st = x.to(dt), gamma.to(dt), stats.to(dt)
    rows, h = x.shape
    xh = (x - st[:, 0:1]) * st[:, 1:2]
    g = d * g0
    mg, mgx = _sum(g, 1) / h, _sum(g * xh, 1) / h
    dx = st[:, 1:2] * (g - mg[:, None] - xh * mgx[:, None])
    parts = torch.zeros(n_part, 2, h, dtype=dt)
    for b, rr in enumerate(ln_part_rows(rows, n_part)):
        if rr:
            parts[b, 0], parts[b, 1] = _sum((d * xh)[rr], 0), _sum(d[rr], 0)
    return dict(dx=dx, partials=parts)


def layernorm_bwd_bound(dy, dy2, x, stats, gamma, n_part):
    """With d = dy + dy2 (one rounding), xhat (two roundings), g = d gamma (two roundings with d's):
        sum g, sum g xhat over h terms whose own roundings are at most 2 U |g| and 4 U |g xhat|:
                 bmg = (h + 4) U sum |g| / h,   bmgx = (h + 6) U sum |g xhat| / h
        dx = rstd (g - mg - xhat mgx): the three terms with their errors, four roundings of the expression:
                 bdx = rstd (bmg + |xhat| bmgx + 6 U (|g| + |mg| + |xhat mgx|))
        partials over the n rows of a workgroup: dgamma terms d xhat carry three roundings, dbeta terms d one:
                 (n + 5) U sum |d xhat|,   (n + 3) U sum |d|
    each times C_LN_BWD.  -> dict(dx, partials)"""
    d = dy.to(F64) if dy2 is None else dy.to(F64) + dy2.to(F64)
    x, g0, st = x.to(F64), gamma.to(F64), stats.to(F64)
    rows, h = x.shape
    xh = (x - st[:, 0:1]) * st[:, 1:2]
    g = d * g0
    mg, mgx = g.sum(1) / h, (g * xh).sum(1) / h
    bmg, bmgx = (h + 4) * U * g.abs().sum(1) / h, (h + 6) * U * (g * xh).abs().sum(1) / h
    bdx = st[:, 1:2].abs() * (bmg[:, None] + xh.abs() * bmgx[:, None] + 6 * U * (g.abs() + mg.abs()[:, None] + (xh * mgx[:, None]).abs()))
    parts = torch.zeros(n_part, 2, h, dtype=F64)
    for b, rr in enumerate(ln_part_rows(rows, n_part)):
        if rr:
            parts[b, 0], parts[b, 1] = (len(rr) + 5) * U * (d * xh)[rr].abs().sum(0), (len(rr) + 3) * U * d[rr].abs().sum(0)
    return dict(dx=C_LN_BWD * bdx, partials=C_LN_BWD * parts)


# ---- attention -----------------------------------------------------------------------------------------------------------
def att_scaling(d):
    return float(1.0 / torch.sqrt(torch.tensor(float(d), dtype=F32)))      # the kernel's 1.0f / sqrtf((float)head_dim)


def _heads(t, heads, d):
    return t.reshape(t.shape[0], heads, d).transpose(0, 1)                 # [heads, positions, d]


def attention_ref(q, k, v, mask, offs, heads, d, cls_only, dt=F64):
    """softmax(q k^T / sqrt(d), masked keys out) v per vocabulary row and head, eager semantics: a row whose keys are all masked
    attends uniformly, otherwise masked keys get exactly 0.  q [Tq, heads d] (Tq = rows with cls_only, else T), k, v [T, heads d],
    mask [T] bool, offs [n + 1]: row r holds positions offs[r] .. offs[r + 1].
    -> dict(ctx [Tq, heads d], probs: per row [heads, nq, L], b_ctx, b_probs), the bounds (float64 run only) times C_ATT_FWD:
        score s_j: d products, the scale and the mask addend:    bs_j = (d + 3) U scaling |q| . |k_j|;  B = max over visible j
        e_j = exp(s_j - max): relative error                     eps_j = 2 B + U |s_j - max| + 4 U   (expf within 2 ulp)
        p_j = e_j / sum e: the sum of L terms, the division:     epsp_j = eps_j + max_j eps_j + (L + 3) U;   b_probs = p_j epsp_j
        ctx = sum_j p_j v_j over L terms:                        b_ctx = sum_j p_j |v_j| (epsp_j + (L + 2) U)"""
    n, hd = len(offs) - 1, heads * d
    sc = att_scaling(d)
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    ctx, b_ctx = torch.zeros(q.shape[0], hd, dtype=dt), torch.zeros(q.shape[0], hd, dtype=F64)
    probs, b_probs = [], []
    for r in range(n):
        t0, t1 = int(offs[r]), int(offs[r + 1])
        L = t1 - t0
        qi = _heads(q[r:r + 1] if cls_only else q[t0:t1], heads, d)
        kk, vv = _heads(k[t0:t1], heads, d), _heads(v[t0:t1], heads, d)
        prod = qi[:, :, None, :] * kk[:, None, :, :]                      # [heads, nq, L, d]
        s = _sum(prod, 3) * sc
        m = mask[t0:t1].bool()
        vis = m[None, None, :].expand_as(s) if bool(m.any()) else torch.ones_like(s, dtype=torch.bool)
        s = torch.where(vis, s, torch.full_like(s, -float("inf"))) if bool(m.any()) else torch.zeros_like(s)
        mx = s.max(dim=2, keepdim=True).values
        e = torch.exp(s - mx)
        p = e / _sum(e, 2)[..., None]
        c = _sum(p[..., None] * vv[:, None, :, :], 2)                     # [heads, nq, d]
        rows = slice(r, r + 1) if cls_only else slice(t0, t1)
        ctx[rows] = c.transpose(0, 1).reshape(-1, hd)
        probs.append(p)
        if dt == F64:
            bs = torch.where(vis, (d + 3) * U * sc * prod.abs().sum(3), torch.zeros_like(s)) if bool(m.any()) else torch.zeros_like(s)
            eps = 2 * bs.max(dim=2, keepdim=True).values + U * torch.where(vis, (s - mx).abs(), torch.zeros_like(s)) + 4 * U
            epsp = eps + eps.max(dim=2, keepdim=True).values + (L + 3) * U
            b_probs.append(C_ATT_FWD * p * epsp)
            bc = ((p * (epsp + (L + 2) * U))[..., None] * vv.abs()[:, None, :, :]).sum(2)
            b_ctx[rows] = C_ATT_FWD * bc.transpose(0, 1).reshape(-1, hd)
    return dict(ctx=ctx, probs=probs, b_ctx=b_ctx, b_probs=b_probs)


def attention_bwd_ref(dctx, q, k, v, probs, offs, heads, d, cls_only, dt=F64):
    """dv_j = sum_i p_ij g_i;  dp_ij = g_i . v_j;  ds_ij = p_ij (dp_ij - sum_j' p_ij' dp_ij');  dq_i = scaling sum_j ds_ij k_j;
    dk_j = scaling sum_i ds_ij q_i, from the probabilities the kernel is GIVEN (probs: per row [heads, nq, L]).
    -> dict(dq, dk, dv, b_dq, b_dk, b_dv), the bounds (float64 run only) times C_ATT_BWD:
        dp_j over d products:                    bdp_j = (d + 2) U |g| . |v_j|
        dot = sum_j p_j dp_j over L terms:       bdot = sum_j p_j bdp_j + (L + 2) U sum_j p_j |dp_j|
        ds_j = p_j (dp_j - dot), two roundings:  bds_j = p_j (bdp_j + bdot + 2 U (|dp_j| + |dot|))
        dq over L terms and the scale:           scaling (sum_j bds_j |k_j| + (L + 3) U sum_j |ds_j| |k_j|)
        dk over nq terms and the scale:          scaling (sum_i bds_ij |q_i| + (nq + 3) U sum_i |ds_ij| |q_i|)
        dv over nq terms:                        (nq + 2) U sum_i p_ij |g_i|"""
    n, hd = len(offs) - 1, heads * d
    sc = att_scaling(d)
    g, q, k, v = dctx.to(dt), q.to(dt), k.to(dt), v.to(dt)
    out = {name: torch.zeros(t.shape[0], hd, dtype=(dt if name[0] == "d" else F64)) for name, t in
           (("dq", q), ("dk", k), ("dv", k), ("b_dq", q), ("b_dk", k), ("b_dv", k))}
    flat = lambda t: t.transpose(0, 1).reshape(-1, hd)
    for r in range(n):
        t0, t1 = int(offs[r]), int(offs[r + 1])
        L = t1 - t0
        rows = slice(r, r + 1) if cls_only else slice(t0, t1)
        qi, gi = _heads(q[rows], heads, d), _heads(g[rows], heads, d)
        nq = qi.shape[1]
        kk, vv = _heads(k[t0:t1], heads, d), _heads(v[t0:t1], heads, d)
        p = probs[r].to(dt)
        dpp = gi[:, :, None, :] * vv[:, None, :, :]                        # [heads, nq, L, d]
        dp = _sum(dpp, 3)
        dot = _sum(p * dp, 2)[..., None]
        ds = p * (dp - dot)
        out["dq"][rows] = flat(_sum(ds[..., None] * kk[:, None, :, :], 2) * sc)
        out["dk"][t0:t1] = flat(_sum(ds[..., None] * qi[:, :, None, :], 1) * sc)
        out["dv"][t0:t1] = flat(_sum(p[..., None] * gi[:, :, None, :], 1))
        if dt == F64:
            bdp = (d + 2) * U * dpp.abs().sum(3)
            bdot = (p * bdp).sum(2, keepdim=True) + (L + 2) * U * (p * dp.abs()).sum(2, keepdim=True)
            bds = p * (bdp + bdot + 2 * U * (dp.abs() + dot.abs()))
            out["b_dq"][rows] = C_ATT_BWD * flat(sc * ((bds[..., None] * kk.abs()[:, None]).sum(2) + (L + 3) * U * (ds.abs()[..., None] * kk.abs()[:, None]).sum(2)))
            out["b_dk"][t0:t1] = C_ATT_BWD * flat(sc * ((bds[..., None] * qi.abs()[:, :, None]).sum(1) + (nq + 3) * U * (ds.abs()[..., None] * qi.abs()[:, :, None]).sum(1)))
            out["b_dv"][t0:t1] = C_ATT_BWD * flat((nq + 2) * U * (p[..., None] * gi.abs()[:, :, None]).sum(1))
    return out


def probs_from_buffer(buf, offs, seq, heads, cls_only):
    """the [L, L] (cls_only: [1, L]) blocks of a probs buffer [n, heads, seq, seq]; what lies outside them is unspecified"""
    n = len(offs) - 1
    b = buf.reshape(n, heads, seq, seq)
    out = []
    for r in range(n):
        L = int(offs[r + 1]) - int(offs[r])
        out.append(b[r, :, :(1 if cls_only else L), :L].clone())
    return out


# ---- source gather -------------------------------------------------------------------------------------------------------
def gather_fwd_ref(ids, src, v0, fallback, sw, sb):
    """x[t] = id < v0 ? sw * src[id] + sb : fallback[id - v0].  -> (value float64, bound): fallback rows and source rows without a
    rescaler are copies (bound 0: equality), rescaled rows one multiply-add (fma_bound)"""
    ids = ids.long()
    is_fb = ids >= v0
    s = src.to(F64)[ids.clamp(max=v0 - 1)]
    bnd = torch.zeros_like(s)
    if sw is not None:
        bnd = fma_bound(sw.to(F64) * s, sb.to(F64).expand_as(s))
        s = sw.to(F64) * s + sb.to(F64)
    fb = fallback.to(F64)[(ids - v0).clamp(min=0)]
    return torch.where(is_fb[:, None], fb, s), torch.where(is_fb[:, None], torch.zeros_like(bnd), bnd)


def gather_bwd_ref(ids, src, v0, n_fallback, dx, dfb0):
    """prod = dx * src[id] (one rounding: torch fp32), keep = dx (copy) on source rows, zeros on fallback rows; dfallback[id - v0]
    += dx over the n rows with that id in no fixed order: (n + 3) U (|dfb0| + sum |dx|).  -> dict(prod, keep: fp32, exact;
    dfallback, b_dfallback: float64)"""
    ids = ids.long()
    is_fb = (ids >= v0)[:, None]
    s = src.to(F32)[ids.clamp(max=v0 - 1)]
    zero = torch.zeros_like(dx)
    dfb, b = scatter_add_ref(dfb0, (ids - v0)[ids >= v0], dx[ids >= v0]) if bool(is_fb.any()) else (dfb0.to(F64), 3 * U * dfb0.to(F64).abs())
    return dict(prod=torch.where(is_fb, zero, dx * s), keep=torch.where(is_fb, zero, dx), dfallback=dfb, b_dfallback=b)


# ---- buffers -------------------------------------------------------------------------------------------------------------
class Frame(Framed):
    """gemm_check.Framed, also for 16-bit outputs: their canary is CANARY16 in every element of the slack"""

    def __init__(self, rows, cols, ld, dtype, fill, shift=0, values=None):
        if fill == "canary" and dtype != torch.float32:
            super().__init__(rows, cols, ld, dtype, 0.0, shift=shift)
            self.buf = torch.full((self.buf.numel(),), CANARY16, dtype=torch.int16).view(dtype)
            if values is not None:
                self.view(self.buf).copy_(values)
        else:
            super().__init__(rows, cols, ld, dtype, fill, shift=shift, values=values)

    def overwritten(self, buf):
        if self.dtype == torch.float32:
            return super().overwritten(buf)
        bits = buf.detach().cpu().contiguous().view(torch.int16).clone()
        assert bits.numel() == self.buf.numel()
        self.view(bits).fill_(CANARY16)
        rel = torch.nonzero(bits != CANARY16).flatten() - self.offset
        if self.rows is None:
            return [(0, int(i)) for i in rel]
        return [(int(i) // self.ld, int(i) % self.ld) for i in rel]


def check_slack(frame, buf, what):
    """the canary outside the view only (an output whose inside is partly unspecified: probs)"""
    where = frame.overwritten(buf)
    if where:
        raise CanaryBroken(f"{what}: {len(where)} element(s) outside the [{frame.rows}, {frame.cols}] output (ld {frame.ld}) were overwritten, "
                           f"first at (row, column) {where[:4]}", where)
