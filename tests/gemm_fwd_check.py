"""Element-by-element check of ONE GEMM launch of the forward with any epilogue (zett_op_fwd_gemm, include/zett_hip.h) against float64
on the SAME values (no GPU in here): the sibling of tests/gemm_check.py and tests/rowops_check.py, whose machinery it uses as it is —
Framed / Frame, check, exact, check_canary, lo_bound, sum_bound, fma_bound, U, products and the record.

The reference is float64 torch on the CPU from exactly the values the kernel is given (16-bit inputs widened):

    z = a . w^T                        fold consumer: z = rstd_m (z - mean_m c_n)
    v = act(z + bias_n)
    r = residual[ri(m), n]             ri = res_index or identity; fp32, or residual_lo widened
                                       with res_stats: r = ((r - mean_ri) rstd_ri) gamma_n + beta_n
    v = v + r;  v = scale_n v + shift_n
    out_f32 / out_f32_b (columns >= split_col) = v;  out_lo = T(v);  dst[dst_rows[m]] = OT(v)
    stats_part[s][m] = (sum v, sum v^2) over columns 128 s ... 128 s + 127

Bounds, per element, by the rules of tests/train_ops_check.py (`expect`):

  * the accumulation: gemm_check.bound's (k + 2) U |a| . |w|^T;
  * one U per further fp32 operation, on magnitudes: the bias add U |bias|-sized inside the (k + 2) as gemm_check has it; the fold
    consumer's three operations (t = -mean rstd, x = fma(t, c, bias), fma(acc, rstd, x)) 3 U (|rstd| (|acc| + |mean| |c|) + |bias|) —
    the cancellation in z - mean c is priced on |z| + |mean| |c|; a LayerNorm'd residual's three (the difference, the product, the
    multiply-add) 3 U ((|r| + |mean|) |rstd| |gamma| + |beta|) — the cancellation in r - mean on |r| + |mean|; the residual add
    U (|act(z)| + |r|); the Rescaler fma_bound(scale v, shift) plus |scale| times what v arrives with;
  * behind a GELU the allowance of z passes through GELU_LIPSCHITZ and ACT_ABS is added, as in gemm_check;
  * a 16-bit value is lo_bound of the fp32 bound;
  * a partial is an fp32 sum in a fixed order: (d + 2) U sum |terms| with d the longest chain of additions (`part_depth`, read from the
    kernel), checked against the float64 sums of THE KERNEL'S OWN OUTPUT ROW, so nothing of the GEMM's allowance enters: F32_LN's own
    fp32 row, within the sum bound alone.  For LN16 / LO_LN only the 16-bit copy leaves the kernel: the partials are then compared with
    the sums of that copy and their bound CARRIES ITS ROUNDING — each fp32 value lies within half a 16-bit ulp of the stored one:
    sum ulp / 2 for the sum, sum (|x| ulp + ulp^2 / 4) for the sum of squares.

Relations between two outputs of one fp32 value are exact: out_lo == T(out_f32) bit for bit (BOTH, F32_LN); a destination launch equals
the same launch into out_f32 converted on the host, and rows the map skips (or that no row maps to) keep the canary.

The slice rel-L2 rule of gemm_check (2e-6 per row and column, the small-norm hold behind a GELU with its 2 % cap, one-element slices
exempt) applies to the fp32 outputs as it stands.

Constants: C_FWD_GEMM_VALUE multiplies value_bound, C_FWD_GEMM_PART the partials' sum bound.  The rule is the project's: each is the
smallest of {1, 2, 4, 8} with which the largest err / bound observed on the device over every case of
tests/test_gemm_fwd_direct_gpu.py is at most 0.5 (for a 16-bit output: the share of the error beyond half an ulp, over the fp32
bound).  profiles/gemm_fwd_check.md holds the observed ratios (written to the file named by ZETT_GEMM_FWD_CHECK_RECORD).

`emulate` is the fp32 arithmetic the bounds are sized against: K in chunks of 4 (gemm_check.emulate_acc), the epilogue in fp32 in the
kernel's documented operation order (multiply-adds fused: computed in float64 and rounded once), the partials in the kernel's tree.
"""
from __future__ import annotations

import os
from types import SimpleNamespace

import torch

from tests import gemm_check as gc
from tests import train_ops_check as tc
from tests.gemm_check import ACT_ABS, CANARY_BITS, GELU_LIPSCHITZ, SLICE_REL, SMALL_NORM, SMALL_SHARE, GemmMismatch, products      # noqa: F401
from tests.train_ops_check import (CANARY16, F32, F64, CanaryBroken, Frame, Framed, OpMismatch, U, check, check_canary, exact,      # noqa: F401
                                   fma_bound, lo_bound, sum_bound, ulp_lo)

C_FWD_GEMM_VALUE = 1.0
C_FWD_GEMM_PART = 1.0

RECORD_ENV = "ZETT_GEMM_FWD_CHECK_RECORD"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DST_DT = {0: torch.float32, 1: torch.float16, 2: torch.bfloat16}          # zett_dtype
RANGE_ACTIVATION, RANGE_OUTPUT, RANGE_DEST = 2, 4, 16
MMAX, NMAX, RMAX = 513, 640, 600          # the operand pool: every case takes leading rows / columns of it

# gemm4d's epilogue instantiations (G4D_EPI_* of csrc/gemm4d.hip.h)
GENERIC, LO, F32E, F32_SCALE, BOTH, F32_LN, LO_FOLD, LO_LN, F32_SCALE_FOLD, LN16 = range(10)
MODE_NAMES = ("GENERIC", "LO", "F32", "F32_SCALE", "BOTH", "F32_LN", "LO_FOLD", "LO_LN", "F32_SCALE_FOLD", "LN16")


def write_record(path):
    """the fwd_gemm entries of the shared record (train_ops_check.RECORD): figures for profiles/gemm_fwd_check.md"""
    keep = {k: v for k, v in tc.RECORD.items() if str(k[0]).startswith("fwd_gemm")}
    saved = dict(tc.RECORD)
    try:
        tc.RECORD.clear()
        tc.RECORD.update(keep)
        tc.write_record(path)
    finally:
        tc.RECORD.clear()
        tc.RECORD.update(saved)


def record_path():
    return os.environ.get(RECORD_ENV)


# ---- the dispatch, restated (csrc/gemm_launch.hip.h gemm_variant_for, csrc/gemm4d.hip.h gemm4d_epi_mode / gemm4d_dst_mode) -------------
def epi_mode_expected(c):
    """gemm4d_epi_mode, line for line, on a case (ld_* as the case states them)"""
    n, two = c.n, c.kind != "f32"
    no_split = c.split_col <= 0 or c.split_col >= n
    has_scale = c.scale is not None
    if c.stats_part and c.residual_lo is not None:
        ok = (two and c.out_lo and not c.out_f32 and c.residual is None and c.act == 0 and not has_scale and no_split and n % 128 == 0 and c.ld_lo % 8 == 0 and
              c.ld_res_lo % 8 == 0)
        return LN16 if ok else -1
    if c.stats_part:
        common = c.out_lo and c.residual is not None and not has_scale and no_split and n % 128 == 0 and c.ld_lo % 4 == 0 and c.ld_res % 4 == 0
        if common and c.out_f32 and c.act == 0 and c.ld_f32 % 4 == 0:
            return F32_LN
        if common and not c.out_f32 and c.act == 1 and c.res_stats is None and c.res_index is None:
            return LO_LN
        return -1
    if c.fold_stats is not None:
        if c.out_lo and not c.out_f32 and c.residual is None and not has_scale and no_split and n % 8 == 0 and c.ld_lo % 8 == 0:
            return LO_FOLD
        if c.out_f32 and not c.out_lo and c.residual is None and has_scale and c.act == 0 and no_split and n % 4 == 0 and c.ld_f32 % 4 == 0:
            return F32_SCALE_FOLD
        return -1
    if not no_split:
        return GENERIC
    if c.res_stats is not None and (c.act != 0 or c.residual is None):
        return GENERIC
    if c.out_lo and not c.out_f32 and c.residual is None and not has_scale and n % 8 == 0 and c.ld_lo % 8 == 0:
        return LO
    if c.out_f32 and c.out_lo and c.residual is None and not has_scale and c.act == 0 and n % 4 == 0 and c.ld_f32 % 4 == 0 and c.ld_lo % 4 == 0:
        return BOTH
    if c.out_f32 and not c.out_lo and n % 4 == 0 and c.ld_f32 % 4 == 0 and (c.residual is None or c.ld_res % 4 == 0):
        if has_scale and c.residual is None and c.act == 0:
            return F32_SCALE
        if not has_scale and (c.act == 0 or (c.act == 1 and c.residual is not None)):
            return F32E
    return GENERIC


def half_ok_expected(c, mode):
    """gemm4d_half_ok"""
    if mode <= GENERIC:
        return False
    if mode == F32E:
        return c.act == 0 or (c.act == 1 and c.residual is not None)
    return True


def variant_expected(c):
    """gemm_variant_for, line for line -> the variant the launch takes"""
    m, n, k, is_f32 = c.m, c.n, c.k, c.kind == "f32"
    has_scale = c.scale is not None
    v = c.gemm_variant
    if v == 0:
        v = 2 if (m > 128 and n > 128) else 1
        if v != 1 and n % 256 == 0 and not has_scale and c.residual is None:
            t256, t384 = ((m + 255) // 256) * (n // 256), ((m + 383) // 384) * (n // 256)
            if 1.7 * ((t384 + 255) // 256) < ((t256 + 255) // 256):
                v = 3
    if v == 3 and (n % 256 != 0 or ((m + 383) // 384) * 384 > c.a_rows_readable or has_scale or c.residual is not None or c.range_final):
        v = 2
    if c.gemm_variant == 0 and v == 2 and not is_f32 and k >= c.gemm4d_min_k:
        v = 7
    if v in (7, 8) and is_f32:
        v = 2
    no_split = c.split_col <= 0 or c.split_col >= n
    wide_ok = (n % 8 == 0 and (not c.out_lo or c.ld_lo % 8 == 0) and c.ld_f32 % 4 == 0 and (c.residual is None or c.ld_res % 4 == 0) and
               (no_split or c.split_col % 8 == 0))
    if v != 1 and not wide_ok:
        v = 1
    if c.residual is not None and has_scale:
        v = 1
    if c.stats_part or c.fold_stats is not None:
        v = 7
    return v


def path_expected(c):
    """-> (variant, mode or -1, tile: 'full' / 'half' / 'cut' / None): what zett_op_fwd_gemm reports, and the tiles gemm4d covers the
    rows with (launch_gemm4d: row0 from gemm_tail_split; gemm4d_row_split cuts every launch of at most 256 tiles at row 0)"""
    v = variant_expected(c)
    if v not in (7, 8):
        return v, -1, None
    if c.dst:
        mode = epi_mode_expected(c.replace(out_f32=True, ld_f32=4, dst=False)) if (c.ld_dst % 4 == 0) else -1
        mode = mode if mode in (F32_SCALE, F32_SCALE_FOLD) else -1
    elif v == 8 and not c.stats_part and c.fold_stats is None:
        mode = GENERIC
    else:
        mode = epi_mode_expected(c)
    ts, m = c.gemm_tail_split, c.m
    tiles = ((m + 255) // 256) * ((c.n + 255) // 256)
    assert tiles < 256, "the cases are smaller than one round of 256 tiles"
    split = {0: m, 1: 0, 2: min(((m // 2 + 255) // 256) * 256, m), 3: 0}[ts]      # (1: gemm4d_row_split, T < 256 tiles -> row0 = 0: half tiles throughout)
    if split < m and not half_ok_expected(c, mode):
        split = m
    return v, mode, ("full" if split >= m else "half" if split == 0 else "cut")


# ---- operands -----------------------------------------------------------------------------------------------------------------
_POOL = {}


def pool(kind, k):
    """a [MMAX, k] with every row scaled by its own factor in [0.5, 2], w [NMAX, k] ~ N(0, 1) 1.5 / sqrt(k) (z has a standard deviation of at
    most 3: the GELUs' range), both rounded to the operand type; the float64 products; per-column vectors with distinct values; a
    residual [RMAX, NMAX] in fp32 and rounded; (mean, rstd) per row that are NOT any row's true statistics; index maps.  Made once per
    (type, k); a case takes leading rows and columns."""
    if (kind, k) in _POOL:
        return _POOL[kind, k]
    if len(_POOL) > 2:
        _POOL.clear()
    g = torch.Generator().manual_seed(1009 * k + 17 * list(DT).index(kind))
    dt = DT[kind]
    row_scale = torch.linspace(0.5, 2.0, MMAX)[torch.randperm(MMAX, generator=g)]
    a = (torch.randn(MMAX, k, generator=g) * row_scale[:, None]).to(dt)
    w = (torch.randn(NMAX, k, generator=g) * (1.5 / k ** 0.5)).to(dt)
    col = torch.arange(NMAX, dtype=F32)
    p = SimpleNamespace(kind=kind, k=k, a=a, w=w, prod=products(a, w))
    p.bias = 0.5 * torch.randn(NMAX, generator=g) + 0.001 * col
    p.gamma = 0.75 + 0.5 * torch.rand(NMAX, generator=g) + 0.0005 * col
    p.beta = 0.3 * torch.randn(NMAX, generator=g) + 0.0007 * col
    p.fold_c = 0.5 * torch.randn(NMAX, generator=g) + 0.0009 * col
    p.scale = 0.5 + torch.rand(NMAX, generator=g) + 0.0003 * col
    p.shift = 0.4 * torch.randn(NMAX, generator=g) - 0.0011 * col
    p.residual = torch.randn(RMAX, NMAX, generator=g) * torch.linspace(0.5, 1.5, RMAX)[torch.randperm(RMAX, generator=g)][:, None]
    p.residual_lo = p.residual.to(dt) if kind != "f32" else None
    mean = torch.linspace(-0.5, 0.5, RMAX)[torch.randperm(RMAX, generator=g)]
    rstd = torch.linspace(0.5, 1.5, RMAX)[torch.randperm(RMAX, generator=g)]
    p.res_stats = torch.stack([mean, rstd], 1).contiguous()
    mean = torch.linspace(-0.5, 0.5, MMAX)[torch.randperm(MMAX, generator=g)]
    rstd = torch.linspace(0.5, 1.5, MMAX)[torch.randperm(MMAX, generator=g)]
    p.fold_stats = torch.stack([mean, rstd], 1).contiguous()
    # a non-monotone map with repeats into the RMAX residual rows: row m adds row (389 m + 7) % RMAX, every fifth row repeats its neighbour's
    idx = (389 * torch.arange(MMAX) + 7) % RMAX
    idx[4::5] = idx[3::5][:idx[4::5].numel()]
    p.res_index = idx.to(torch.int32)
    _POOL[kind, k] = p
    return p


def dst_rows_for(m, n_dst):
    """a permutation of the launch's rows into n_dst >= m destination rows, every seventh row skipped (-1): row i -> (i * 211 + 5) % n_dst
    with n_dst coprime to 211"""
    rows = (torch.arange(m, dtype=torch.int64) * 211 + 5) % n_dst
    assert rows.unique().numel() == m
    rows[3::7] = -1
    return rows


class Case(SimpleNamespace):
    def replace(self, **kw):
        d = dict(self.__dict__)
        d.update(kw)
        return Case(**d)


def make_case(kind, m, n, k, *, act=0, bias=True, residual=None, res_stats=False, res_index=False, fold=False, scale=False, out_f32=False, out_lo=False,
              stats_part=False, split_col=0, dst=False, dst_dtype=0, dst_map=True, range_final=0, pad=0, gemm_variant=0, gemm4d_min_k=64, gemm_tail_split=0,
              gemm_tile_order=0, gemm_group=0, a_slack=False):
    """One launch on the pool's leading m rows / n columns.  residual: None, 'f32' or 'lo'.  pad: extra elements of every output / residual
    leading dimension (a multiple of 8 keeps the wide paths).  gemm4d_min_k defaults to 64 here: the small K of these cases reach
    gemm4d as the forward's K >= 512 do.  a_slack: A is followed by readable rows up to ceil(m / 384) * 384 (variant 3)."""
    p = pool(kind, k)
    c = Case(kind=kind, m=m, n=n, k=k, act=act, pool=p, a=p.a[:m], w=p.w[:n], prod=(p.prod[0][:m, :n], p.prod[1][:m, :n]),
             bias=p.bias[:n] if bias else None, residual=None, residual_lo=None, res_stats=None, res_gamma=None, res_beta=None, res_index=None,
             fold_stats=None, fold_c=None, scale=None, shift=None, out_f32=out_f32, out_lo=out_lo, stats_part=stats_part, split_col=split_col,
             dst=dst, dst_dtype=dst_dtype, dst_rows=None, n_dst=m, range_final=range_final,
             gemm_variant=gemm_variant, gemm4d_min_k=gemm4d_min_k, gemm_tail_split=gemm_tail_split, gemm_tile_order=gemm_tile_order, gemm_group=gemm_group)
    n_res = RMAX if res_index else m
    if residual == "f32":
        c.residual = p.residual[:n_res, :n]
    elif residual == "lo":
        c.residual_lo = p.residual_lo[:n_res, :n]
    if res_stats:
        c.res_stats, c.res_gamma, c.res_beta = p.res_stats[:n_res], p.gamma[:n], p.beta[:n]
    if res_index:
        c.res_index = p.res_index[:m]
    if fold:
        c.fold_stats, c.fold_c = p.fold_stats[:m], p.fold_c[:n]
    if scale:
        c.scale, c.shift = p.scale[:n], p.shift[:n]
    no_split = split_col <= 0 or split_col >= n
    width = n if no_split else split_col
    c.ld_f32 = (max(width, n - width) + pad) if (out_f32 or not no_split) else 0
    c.ld_lo = width + pad if out_lo else 0
    c.ld_res = n + pad if c.residual is not None else 0
    c.ld_res_lo = n + pad if c.residual_lo is not None else 0
    c.ld_part = m + 3 if stats_part else 0
    c.ld_dst = n + 8 if dst else 0          # a leading dimension larger than n
    if dst and dst_map:
        c.n_dst = m + 9 if (m + 9) % 211 else m + 10
        c.dst_rows = dst_rows_for(m, c.n_dst)
    c.a_rows_readable = ((m + 383) // 384) * 384 if a_slack else m
    return c


# ---- reference, bounds, emulation ------------------------------------------------------------------------------------------------
def _res_rows(c, dt):
    """the residual rows the launch adds, [m, n] in dt, and (mean, rstd) [m] of them (or None)"""
    src = c.residual if c.residual is not None else c.residual_lo
    ri = c.res_index.long() if c.res_index is not None else torch.arange(c.m)
    st = None if c.res_stats is None else c.res_stats.to(dt)[ri]
    return src.to(dt)[ri], st


def expect(c):
    """-> dict(v [m, n] float64, b_v: its fp32 bound times C_FWD_GEMM_VALUE)"""
    acc, mag = c.prod
    b_acc = (c.k + 2) * U
    zero = torch.zeros((), dtype=F64)
    bias = c.bias.to(F64) if c.bias is not None else zero
    if c.fold_stats is not None:
        mean, rstd, cc = c.fold_stats[:, 0:1].to(F64), c.fold_stats[:, 1:2].to(F64), c.fold_c.to(F64)
        z = rstd * (acc - mean * cc) + bias
        b = rstd.abs() * b_acc * mag + 3 * U * (rstd.abs() * (acc.abs() + mean.abs() * cc.abs()) + bias.abs())
    else:
        z = acc + bias
        b = gc.bound(dict(mag=mag + bias.abs(), residual=None), c.k, 0)          # (k + 2) U (|a| . |w|^T + |bias|)
    v = gc._gelu(z, c.act)
    if c.act != 0:
        b = GELU_LIPSCHITZ * b + ACT_ABS
    if c.residual is not None or c.residual_lo is not None:
        r, st = _res_rows(c, F64)
        if st is not None:
            mean, rstd, gm, bt = st[:, 0:1], st[:, 1:2], c.res_gamma.to(F64), c.res_beta.to(F64)
            b = b + 3 * U * ((r.abs() + mean.abs()) * rstd.abs() * gm.abs() + bt.abs())
            r = ((r - mean) * rstd) * gm + bt
        b = b + U * (v.abs() + r.abs())
        v = v + r
    if c.scale is not None:
        sc, sh = c.scale.to(F64), c.shift.to(F64)
        b = sc.abs() * b + fma_bound(sc * v, sh)
        v = sc * v + sh
    return dict(v=v, b_v=C_FWD_GEMM_VALUE * b)


def _fma32(a, b, c):
    """a * b + c rounded once (fp32 in, fp32 out): the product of two fp32 values is exact in float64"""
    return (a.double() * b.double() + c.double()).float()


def _gelu32(z, act):
    """gelu_tanh_f / gelu_erf_f in fp32 as written in csrc/gemm.hip.h (torch's exp / erf where the device has its intrinsics)"""
    if act == 0:
        return z
    if act == 1:
        x3 = (z * z) * z
        u2 = 1.5957691216057308 * _fma32(torch.tensor(0.044715), x3, z)
        t = 1.0 - 2.0 * (1.0 / (1.0 + torch.exp2(u2 * 1.4426950408889634)))
        return (0.5 * z) * (1.0 + t)
    return tc.gelu(z, 2)


def part_depth(mode):
    """-> (d_sum, d_squares): the longest chain of fp32 additions behind a partial (csrc/gemm4d.hip.h, the drain of the streamlined
    epilogues).  F32_LN / LO_LN, four columns per lane ("per-row (sum, sum of squares) over the wave's 128 columns: a reduce-scatter over the
    32 lanes"): S = (a + b) + (c + d) is 2, Q = fma(a, a, fma(b, b, fma(c, c, d d))) is 3, then the exchanges xor 16, 8, 4, 2, 1: 5 each.
    LN16, eight columns per lane ("a reduce-scatter over the 16 lanes of a row"): S = ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)) is 3,
    Q a chain of seven multiply-adds is 7, then xor 8, 4, 2, 1: 4 each."""
    return (7, 11) if mode == LN16 else (7, 8)


def _parts32(v32, mode):
    """(sum, sum of squares) per 128-column slice in the kernel's tree -> [S, m, 2] fp32"""
    m, n = v32.shape
    cpl = 8 if mode == LN16 else 4
    x = v32.reshape(m, n // 128, 128 // cpl, cpl)
    if cpl == 4:
        s = (x[..., 0] + x[..., 1]) + (x[..., 2] + x[..., 3])
    else:
        s = ((x[..., 0] + x[..., 1]) + (x[..., 2] + x[..., 3])) + ((x[..., 4] + x[..., 5]) + (x[..., 6] + x[..., 7]))
    q = x[..., cpl - 1] * x[..., cpl - 1]
    for i in range(cpl - 2, -1, -1):
        q = _fma32(x[..., i], x[..., i], q)
    lanes = 128 // cpl
    while lanes > 1:          # lane l adds lane l ^ (lanes / 2): xor 16 (8), ..., 1
        lanes //= 2
        s, q = s[..., :lanes] + s[..., lanes:], q[..., :lanes] + q[..., lanes:]
    return torch.stack([s[..., 0], q[..., 0]], -1).permute(1, 0, 2).contiguous()


def emulate(c, mode=None, chunk=4):
    """the launch in emulated fp32 -> dict(v32 [m, n], and the outputs the case asks for: out_f32, out_f32_b, out_lo, parts [S, m, 2],
    dst [n_dst, n] with the canary where nothing is written)"""
    acc = gc.emulate_acc(c.a, c.w, chunk)
    bias = c.bias.float() if c.bias is not None else torch.zeros(c.n)
    if c.fold_stats is not None:
        mean, rstd = c.fold_stats[:, 0:1].float(), c.fold_stats[:, 1:2].float()
        t = -mean * rstd
        v = _fma32(acc, rstd.expand_as(acc), _fma32(t.expand_as(acc), c.fold_c.float().expand_as(acc), bias.expand_as(acc)))
    else:
        v = acc + bias
    v = _gelu32(v, c.act)
    if c.residual is not None or c.residual_lo is not None:
        r, st = _res_rows(c, F32)
        if st is not None:
            r = _fma32((r - st[:, 0:1]) * st[:, 1:2], c.res_gamma.float().expand_as(r), c.res_beta.float().expand_as(r))
        v = v + r
    if c.scale is not None:
        v = _fma32(c.scale.float().expand_as(v), v, c.shift.float().expand_as(v))
    return outputs_of(c, v, mode)


def outputs_of(c, v32, mode=None):
    """what a launch that computed the fp32 values v32 leaves in its outputs"""
    out = dict(v32=v32)
    no_split = c.split_col <= 0 or c.split_col >= c.n
    width = c.n if no_split else c.split_col
    if c.out_f32:
        out["out_f32"] = v32[:, :width].clone()
    if not no_split:
        out["out_f32_b"] = v32[:, width:].clone()
    if c.out_lo:
        out["out_lo"] = v32[:, :width].to(DT[c.kind])
    if c.stats_part:
        out["parts"] = _parts32(v32, mode if mode is not None else epi_mode_expected(c))
    if c.dst:
        out["dst"] = dst_image(c, v32)
    return out


def canary_like(rows, cols, dtype):
    if dtype == torch.float32:
        return torch.full((rows, cols), CANARY_BITS, dtype=torch.int32).view(torch.float32)
    return torch.full((rows, cols), CANARY16, dtype=torch.int16).view(dtype)


def dst_image(c, v32):
    """[n_dst, n] of the destination type: row m of v32 converted (round to nearest even) at row dst_rows[m], the canary elsewhere"""
    odt = DST_DT[c.dst_dtype]
    img = canary_like(c.n_dst, c.n, odt)
    rows = c.dst_rows if c.dst_rows is not None else torch.arange(c.m)
    keep = rows >= 0
    img[rows[keep]] = v32[keep].to(odt)
    return img


# ---- buffers ---------------------------------------------------------------------------------------------------------------------
def output_frames(c):
    """the canary-framed outputs of a case: name -> Frame"""
    no_split = c.split_col <= 0 or c.split_col >= c.n
    width = c.n if no_split else c.split_col
    f = {}
    if c.out_f32:
        f["out_f32"] = Frame(c.m, width, c.ld_f32, F32, "canary")
    if not no_split:
        f["out_f32_b"] = Frame(c.m, c.n - width, c.ld_f32, F32, "canary")
    if c.out_lo:
        f["out_lo"] = Frame(c.m, width, c.ld_lo, DT[c.kind], "canary")
    if c.stats_part:
        f["parts"] = Frame(c.n // 128, 2 * c.m, 2 * c.ld_part, F32, "canary")
    if c.dst:
        f["dst"] = Frame(c.n_dst, c.n, c.ld_dst, DST_DT[c.dst_dtype], "canary")
    return f


def place(frames, outs):
    """(host test) the emulation's outputs written into copies of the frames' buffers, as a launch would leave them -> name -> buffer"""
    bufs = {}
    for name, fr in frames.items():
        buf = fr.buf.clone()
        val = outs[name]
        fr.view(buf).copy_(val.reshape(val.shape[0], -1) if name == "parts" else val)
        bufs[name] = buf
    return bufs


# ---- the checks --------------------------------------------------------------------------------------------------------------------
def _slices(got, y, act, what):
    """gemm_check's slice rule on an fp32 output: rel-L2 <= SLICE_REL of every row and column (see the module docstring there)"""
    g, y = got.detach().cpu().to(F64), y.to(F64)
    fin = torch.isfinite(g)
    diff = torch.where(fin, g - y, torch.zeros_like(y))
    over, top = [], 0.0
    for dim, name, size in ((1, "row", y.shape[1]), (0, "column", y.shape[0])):
        norm = y.norm(dim=dim)
        keep = torch.ones_like(norm, dtype=torch.bool)
        if act != 0:
            keep &= norm >= SMALL_NORM
        if size == 1:
            keep &= False
        elif act != 0:
            share = 1.0 - float(keep.double().mean())
            assert share <= SMALL_SHARE, f"{what}: {share:.1%} of the {name}s have a reference norm below {SMALL_NORM}: the case is scaled wrongly"
        rel = torch.where(keep, diff.norm(dim=dim) / norm.clamp_min(1e-300), torch.zeros_like(norm))
        top = max(top, float(rel.max()) if rel.numel() else 0.0)
        over.append(torch.nonzero(rel > SLICE_REL).flatten().tolist())
        if over[-1]:
            worst = max(over[-1], key=lambda i: float(rel[i]))
            msg = f"{what}: {len(over[-1])} {name}(s) over rel-L2 {SLICE_REL:.0e}: worst {name} {worst} at {float(rel[worst]):.3e} (first {over[-1][:8]})"
            bad = torch.zeros(y.shape, dtype=torch.bool)
            raise GemmMismatch(msg, bad, over[0], over[1] if len(over) > 1 else [], worst if dim == 1 else 0, worst if dim == 0 else 0)
    return top


def _note_slices(key, rel):
    """the largest slice rel-L2 of an fp32 output, filed under '<layout> slices' (no err / bound of its own)"""
    if key is not None:
        tc._note((key[0], key[1] + " slices"), 0.0, rel)


def _note_lo_share(key, got, ref, b32, dtype):
    """rowops_check.note_lo_share: for the constants, a 16-bit output counts with the share of its error beyond half an ulp, over the
    fp32 bound"""
    if key is None or dtype not in (torch.float16, torch.bfloat16):
        return
    err = (got.detach().cpu().to(F64) - ref).abs() - 0.5 * ulp_lo(ref, dtype)
    share = torch.where(err > 0, err / b32.clamp_min(1e-300), torch.zeros_like(err))
    tc._note((key[0], key[1] + " beyond ulp/2"), float(share.max()) if share.numel() else 0.0, 0.0)


def parts_bound(x, mode, lo):
    """x [m, n] float64: the kernel's own output row.  -> (ref [S, m, 2], bound [S, m, 2]) by the module docstring's rule: (d + 2) U sum |terms|
    times C_FWD_GEMM_PART, plus — `lo` a 16-bit type: x is the rounded copy — half an ulp per element propagated into both sums"""
    m, n = x.shape
    xs = x.reshape(m, n // 128, 128)
    d_s, d_q = part_depth(mode)
    ref = torch.stack([xs.sum(2), (xs * xs).sum(2)], -1)
    bnd = C_FWD_GEMM_PART * torch.stack([(d_s + 2) * U * xs.abs().sum(2), (d_q + 2) * U * (xs * xs).sum(2)], -1)
    if lo in (torch.float16, torch.bfloat16):
        h = 0.5 * ulp_lo(xs, lo)
        # (the sums of the UNROUNDED values are what the kernel adds: their terms are within h of x's, so is the magnitude the sum bound is on)
        bnd = bnd * (1.0 + 2.0 ** -6) + torch.stack([h.sum(2), (2 * xs.abs() * h + h * h).sum(2)], -1)
    return ref.permute(1, 0, 2).contiguous(), bnd.permute(1, 0, 2).contiguous()


def check_launch(c, exp, frames, bufs, what, mode=None, key=None, f32_twin=None):
    """Every output of one launch.  frames / bufs: output_frames(c) and the buffers as the launch left them (host tensors).  mode: the
    gemm4d epilogue the launch reported (names the partials' tree; default: the restated rule).  f32_twin: for a destination launch, the
    [m, n] fp32 values the same launch wrote into out_f32.  key: the record's layout name (op 'fwd_gemm ...' is added here)."""
    mode = epi_mode_expected(c) if mode is None else mode
    no_split = c.split_col <= 0 or c.split_col >= c.n
    width = c.n if no_split else c.split_col
    v, b = (exp["v"], exp["b_v"]) if exp is not None else (None, None)          # (a destination launch has its fp32 twin for a reference)
    k2 = None if key is None else ("fwd_gemm " + key[0], key[1])
    got = {}
    for name, fr in frames.items():
        if name == "dst":
            continue
        check_canary(fr, bufs[name], f"{what} {name}")
        got[name] = fr.view(bufs[name].detach().cpu()).clone()
    if "out_f32" in got:
        check(got["out_f32"], v[:, :width], b[:, :width], f"{what} out_f32", key=k2)
        _note_slices(k2, _slices(got["out_f32"], v[:, :width], c.act, f"{what} out_f32"))
    if "out_f32_b" in got:
        check(got["out_f32_b"], v[:, width:], b[:, width:], f"{what} out_f32_b", key=k2)
        _note_slices(k2, _slices(got["out_f32_b"], v[:, width:], c.act, f"{what} out_f32_b"))
    if "out_lo" in got:
        dt = DT[c.kind]
        if "out_f32" in got:
            exact(got["out_lo"], got["out_f32"].to(dt), f"{what} out_lo == T(out_f32)")
        if dt == torch.float32:
            check(got["out_lo"], v[:, :width], b[:, :width], f"{what} out_lo", key=k2)
        else:
            check(got["out_lo"], v[:, :width], lo_bound(v[:, :width], b[:, :width], dt), f"{what} out_lo")
            _note_lo_share(k2, got["out_lo"], v[:, :width], b[:, :width], dt)
    if "parts" in got:
        own = got["out_f32"] if "out_f32" in got else got["out_lo"]
        ref, bnd = parts_bound(own.to(F64), mode, None if "out_f32" in got else DT[c.kind])
        kp = None if k2 is None else (k2[0], k2[1] + " partials")
        try:
            check(got["parts"].reshape(c.n // 128, c.m, 2).reshape(c.n // 128, 2 * c.m), ref.reshape(c.n // 128, 2 * c.m), bnd.reshape(c.n // 128, 2 * c.m),
                  f"{what} stats_part", key=kp)
        except OpMismatch as e:          # name the slice, the row and which of the two sums
            raise OpMismatch(str(e) + f" [slice {e.row} (columns {128 * e.row} ..), row {e.col // 2}, {'sum of squares' if e.col % 2 else 'sum'}]",
                             e.bad, e.rows, e.cols, e.row, e.col) from None
    if c.dst:
        check_dst(c, frames["dst"], bufs["dst"], f32_twin, what)


def check_dst(c, frame, buf, f32_twin, what):
    """a destination launch: the canary outside [n_dst, n] intact; row dst_rows[m] equals OT(the fp32 twin's row m) bit for bit; every
    destination row no launch row maps to — the skipped ones included — still holds the canary"""
    where = frame.overwritten(buf)
    if where:
        raise CanaryBroken(f"{what} dst: {len(where)} element(s) outside the [{frame.rows}, {frame.cols}] destination (ld {frame.ld}) were overwritten, "
                           f"first at (row, column) {where[:4]}", where)
    got = frame.view(buf.detach().cpu()).clone()
    want = dst_image(c, f32_twin)
    try:
        exact(got, want, f"{what} dst == OT(out_f32 of the same launch)")
    except OpMismatch as e:
        rows = c.dst_rows if c.dst_rows is not None else torch.arange(c.m)
        src = torch.nonzero(rows == e.row).flatten().tolist()
        raise OpMismatch(str(e) + (f" [destination row {e.row} = launch row {src[0]}]" if src else f" [destination row {e.row}: no launch row maps to it, it must keep the canary]"),
                         e.bad, e.rows, e.cols, e.row, e.col) from None
