"""References and bounds of the Rescaler fit (zett_amd/csrc/train_init.hip: zett_op_col_moments, zett_op_rescaler_fit), no GPU in
here: the sibling of tests/rowops_check.py, on the checks, the buffers, the unit U and the record of tests/train_ops_check.py.

References are float64 on the SAME stored values: `moments_ref` (count, mean, M2 = sum (x - mean)^2, population std), `scale_to_ref`
— Rescaler.scale_to exactly as written in zett/utils.py:165-175 — and `init_rescaler_ref`, the sequence of Hypernet.init_rescaler
(zett/model/__init__.py:348-385).  `emulate_moments` / `emulate_fit` restate the kernels' arithmetic (a Welford recurrence in fp64
over chunks of CHUNK rows, the chunks merged in order with Chan's update, the fit in fp64 rounded once to fp32);
tests/test_rescaler_check_host.py holds the emulation below a quarter of every bound.  `emulate_naive` is the one-pass
E[x^2] - mean^2 in fp32 that the bounds are there to catch.

The bounds, per column, by the rules of tests/train_ops_check.py (U = 2^-23; sum_bound(n, mag) = (n + 2) U mag for a sum of n fp32
terms in any order; fma_bound), with n the rows, d = x - mean, all on the float64 intermediates:

    mean = (sum x) / n, a sum of n terms and a division:              bm   = sum_bound(n, sum |x|) / n
    M2 = sum d^2 about a mean that is off by at most bm: moving the centre of a sum of squared deviations by t adds exactly n t^2
         (the first-order term 2 t sum d vanishes: sum d = 0), so the mean's error enters with n bm^2; each term then carries the
         rounding of d (2 U d^2) and of the square (U d^2), and the sum its n additions:
                                                                       bq   = n bm^2 + (n + 5) U M2
         (There is no allowance for a RUNNING mean stored in fp32, whose rounding — an ulp of the mean, different from row to row —
         would enter every deviation at first order: a recurrence in fp32 is over this bound already on two rows whose difference is
         small against their mean, which is why the kernel keeps its recurrence in fp64.)
    std = sqrt(M2 / n): with v = M2 / n off by at most bv = bq / n, |sqrt(v + e) - sqrt(v)| <= min(sqrt |e|, |e| / sqrt v) for
         every |e| <= bv that keeps v + e >= 0; three roundings (division, root, conversion):
                                                                       bstd = min(sqrt bv, bv / std) + 3 U std
    w = ts / (sx + 1e-8), ts and sx off by at most bts and bsx:        bw   = (bts + |w| bsx) / (sx + 1e-8 - bsx) + 2 U |w|
         (infinite where bsx >= sx + 1e-8: a column whose std is not told apart from 0 has no bounded w; bts = 0 for a scalar target)
    b = tm - w mx, a multiply-add on operands that carry bounds:       bb   = btm + |w| bmx + |mx| bw + U (|w mx| + |tm|)

times C_COL_MOMENTS (mean, M2, std) and C_RESCALER_FIT (w, b).  The rule for the constants is the project's: the largest err / bound
seen on the device over every case of tests/test_rescaler_direct_gpu.py and tests/test_rescaler_init_gpu.py is at most 0.5.  The
observed ratios go to the file named by ZETT_RESCALER_CHECK_RECORD (profiles/rescaler_check.md).

The M2 bound is second order in the mean's bound bm — which grows with n — on purpose: a first-order allowance 2 bm sum |d| would
let E[x^2] - mean^2 pass on a column of mean 3 and std 0.01, whose variance that formula loses to cancellation
(tests/test_rescaler_check_host.py::test_naive_formula_exceeds_the_std_bound: it is 3.3 times over the std bound there).
"""
from __future__ import annotations

import os

import numpy as np
import torch

from tests import train_ops_check as tc
from tests.train_ops_check import F32, F64, U, Framed, check, check_canary, exact, fma_bound, sum_bound      # noqa: F401 (re-exported for the tests)
from zett_amd import _lib

C_COL_MOMENTS = 1.0
C_RESCALER_FIT = 1.0

RECORD_ENV = "ZETT_RESCALER_CHECK_RECORD"
CHUNK = _lib.COL_MOMENTS_CHUNK          # rows of one partial (ZETT_COL_MOMENTS_CHUNK)
EPSILON = 1e-8                          # zett/utils.py EPSILON
DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def write_record(path):
    """the rescaler entries of the shared record (train_ops_check.RECORD): figures for profiles/rescaler_check.md"""
    keep = {k: v for k, v in tc.RECORD.items() if str(k[0]).startswith(("col_moments", "rescaler_fit", "init_rescaler"))}
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


# ---- references ------------------------------------------------------------------------------------------------------------------
def moments_ref(x):
    """float64 moments of the stored values of x [n, c] (n >= 1) -> dict(count, mean, m2, std)"""
    x = x.to(F64)
    n = x.shape[0]
    mean = x.sum(0) / n
    m2 = ((x - mean) ** 2).sum(0)
    return dict(count=torch.full_like(mean, float(n)), mean=mean, m2=m2, std=torch.sqrt(m2 / n))


def moments_bound(x, ref):
    """-> dict(mean, m2, std): the module docstring's bm, bq, bstd, times C_COL_MOMENTS"""
    x = x.to(F64)
    n = x.shape[0]
    bm = sum_bound(n, x.abs().sum(0)) / n
    bq = n * bm * bm + (n + 5) * U * ref["m2"]
    bv = bq / n
    std = ref["std"]
    bstd = torch.minimum(torch.sqrt(bv), torch.where(std > 0, bv / std.clamp_min(1e-300), torch.full_like(bv, float("inf")))) + 3 * U * std
    return dict(mean=C_COL_MOMENTS * bm, m2=C_COL_MOMENTS * bq, std=C_COL_MOMENTS * bstd)


def scale_to_ref(x, target=None, target_stds=None, target_means=None):
    """Rescaler.scale_to of zett/utils.py:165-175 line by line, in float64 (std: ddof = 0).  -> (w, b), each [1, c]"""
    x = x.to(F64)
    if target_stds is None:
        target_stds = target.to(F64).std(0, unbiased=False)
    if target_means is None:
        target_means = target.to(F64).mean(0)
    w = (target_stds / (x.std(0, unbiased=False) + EPSILON))[None]
    b = (target_means - (x * w).mean(0))[None]
    return w, b


def fit_bound(xr, xb, tr=None, tb=None, target_std=None, target_mean=None):
    """xr / xb: moments_ref / moments_bound of x; tr / tb: those of the target, or the two scalars.  -> (bw, bb), [c] each, times
    C_RESCALER_FIT (the moments' share keeps C_COL_MOMENTS)"""
    sx, mx, bsx, bmx = xr["std"], xr["mean"], xb["std"], xb["mean"]
    if tr is not None:
        ts, tm, bts, btm = tr["std"], tr["mean"], tb["std"], tb["mean"]
    else:
        ts, tm = torch.full_like(sx, float(target_std)), torch.full_like(sx, float(target_mean))
        bts, btm = torch.zeros_like(sx), torch.zeros_like(sx)
    w = ts / (sx + EPSILON)
    room = sx + EPSILON - bsx
    bw = torch.where(room > 0, (bts + w.abs() * bsx) / room.clamp_min(1e-300), torch.full_like(w, float("inf"))) + 2 * U * w.abs()
    carried = torch.where(mx == 0, torch.zeros_like(bw), mx.abs() * bw)
    bb = btm + w.abs() * bmx + carried + fma_bound(w * mx, tm)
    return C_RESCALER_FIT * bw, C_RESCALER_FIT * bb


def init_rescaler_ref(source, pred_in, pred_out, target_in, target_out, init_range):
    """The sequence of Hypernet.init_rescaler in float64: in_scaler from the source matrix against std = init_range and mean 0;
    scaler / out_scaler from the predictions the identity-scaler forward gave (pred_in, pred_out: what the engine fitted on) against
    the target matrices.  -> dict name -> (w, b)"""
    c = source.shape[1]
    out = {"in_scaler": scale_to_ref(source, target_stds=torch.full((c,), float(init_range), dtype=F64), target_means=torch.zeros(c, dtype=F64)),
           "scaler": scale_to_ref(pred_in, target_in)}
    if target_out is not None:
        out["out_scaler"] = scale_to_ref(pred_out, target_out)
    return out


def init_rescaler_bound(source, pred_in, pred_out, target_in, target_out, init_range):
    """the bounds of init_rescaler_ref's entries -> dict name -> (bw, bb)"""
    def mb(x):
        r = moments_ref(x)
        return r, moments_bound(x, r)
    out = {"in_scaler": fit_bound(*mb(source), target_std=init_range, target_mean=0.0), "scaler": fit_bound(*mb(pred_in), *mb(target_in))}
    if target_out is not None:
        out["out_scaler"] = fit_bound(*mb(pred_out), *mb(target_out))
    return out


# ---- emulations ------------------------------------------------------------------------------------------------------------------
def emulate_chunk(x64):
    """the Welford recurrence of one chunk as the kernel runs it, fp64 (numpy rounds the product where the kernel's fma does not:
    2^-53, far below anything checked here): x64 float64 [n, c] -> (mean, m2)"""
    mean, m2 = np.zeros(x64.shape[1]), np.zeros(x64.shape[1])
    for k in range(x64.shape[0]):
        d = x64[k] - mean
        mean = d * (1.0 / (k + 1)) + mean
        m2 = d * (x64[k] - mean) + m2
    return mean, m2


def emulate_moments(calls, chunk=CHUNK):
    """`calls`: the matrices fed one call after the other (the first without accumulate).  -> float64 dict(count, mean, m2, std)"""
    c = calls[0].shape[1]
    n, mean, m2 = 0.0, np.zeros(c), np.zeros(c)
    for x in calls:
        x64 = x.to(F64).numpy()
        for r0 in range(0, x64.shape[0], chunk):
            part = x64[r0:r0 + chunk]
            mb, qb = emulate_chunk(part)
            nb = float(part.shape[0])
            if n == 0.0:
                n, mean, m2 = nb, mb, qb
            else:
                tot, d = n + nb, mb - mean
                r = nb / tot
                mean = mean + d * r
                m2 = m2 + qb + d * d * (n * r)
                n = tot
    t = lambda v: torch.from_numpy(np.asarray(v, dtype=np.float64))      # noqa: E731
    return dict(count=torch.full((c,), n, dtype=F64), mean=t(mean), m2=t(m2), std=t(np.sqrt(np.maximum(m2, 0.0) / n)) if n else t(np.zeros(c)))


def emulate_naive(x):
    """one pass, fp32, sums taken in row order: mean = sum x / n, var = sum x^2 / n - mean^2.  -> float64 dict(mean, std)"""
    x32 = x.to(F32).numpy()
    n = np.float32(x32.shape[0])
    s1 = np.cumsum(x32, axis=0, dtype=np.float32)[-1]          # (numpy's cumsum adds in the array's type, row after row)
    s2 = np.cumsum(x32 * x32, axis=0, dtype=np.float32)[-1]
    mean = s1 / n
    var = s2 / n - mean * mean
    return dict(mean=torch.from_numpy(mean.astype(np.float64)), std=torch.from_numpy(np.sqrt(np.maximum(var, np.float32(0.0))).astype(np.float64)))


def emulate_fit(xs, ts=None, target_std=None, target_mean=None):
    """the fit kernel: fp64 on the states, w and b rounded once to fp32.  -> (w, b) float32 [c]"""
    sx, mx = xs["std"], xs["mean"]
    t_std = ts["std"] if ts is not None else torch.full_like(sx, float(target_std))
    t_mean = ts["mean"] if ts is not None else torch.full_like(sx, float(target_mean))
    w = t_std / (sx + EPSILON)
    return w.to(F32), (t_mean - w * mx).to(F32)


# ---- cases -------------------------------------------------------------------------------------------------------------------------
ROWS = (1, 2, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1)
COLS = (1, 7, 8, 9, 255, 256, 257)
COL0 = (0, 3, 8)
KINDS = ("f32", "f16", "bf16")


def pairwise_cases():
    """(rows, cols, col0, kind, ld): every (rows, cols) pair once; col0 and the element type run over Z3 with (i + j, i + 2 j), an
    invertible map, so every pair of values of any two of the four parameters occurs.  ld alternates between a multiple of 8
    elements (rows keep a 16-byte alignment) and an odd surplus (they do not)."""
    out = []
    for i, rows in enumerate(ROWS):
        for j, cols in enumerate(COLS):
            col0, kind = COL0[(i + j) % 3], KINDS[(i + 2 * j) % 3]
            width = col0 + cols
            ld = (width + 1 + 7) // 8 * 8 if (i * len(COLS) + j) % 2 == 0 else width + 3
            out.append((rows, cols, col0, kind, ld))
    out.append((4097, 520, 0, "bf16", 520))
    return out


_VALUES = {}


def case_values(rows, width, kind, seed=0):
    """the [rows, width] matrix of a case in its element type: per column a scale in [0.005, 2] and an offset in [-1, 1], so that means
    matter.  Computed once per (shape, type, seed), shared, never modified."""
    key = (rows, width, kind, seed)
    if key not in _VALUES:
        g = torch.Generator().manual_seed(1000003 * rows + 7919 * width + 31 * seed + KINDS.index(kind))
        scale = 0.005 * 400.0 ** torch.rand(width, generator=g, dtype=F64)
        offset = 2.0 * torch.rand(width, generator=g, dtype=F64) - 1.0
        _VALUES[key] = (torch.randn(rows, width, generator=g, dtype=F64) * scale + offset).to(DT[kind])
    return _VALUES[key]


SPECIAL_ROWS = 4096


def special_values(kind):
    """[4096, 4]: column 0 of mean 3 and std 0.01 (the sensitivity column), column 1 constant, column 2 ordinary, column 3 — f16 only —
    values next to the largest finite f16, 65504 (spacing 32)."""
    key = ("special", kind)
    if key not in _VALUES:
        g = torch.Generator().manual_seed(20240607 + KINDS.index(kind))
        x = torch.randn(SPECIAL_ROWS, 4, generator=g, dtype=F64)
        x[:, 0] = 3.0 + 0.01 * x[:, 0]
        x[:, 1] = 1.2421875
        x[:, 3] = 65504.0 - 32.0 * torch.randint(0, 8, (SPECIAL_ROWS,), generator=g).to(F64) if kind == "f16" else 100.0 * x[:, 3]
        _VALUES[key] = x.to(DT[kind])
    return _VALUES[key]


def check_moments(what, got, x, key=None):
    """got: dict(count, mean, m2, std) float64 [c] of a device state over the rows of x.  -> the largest err / bound"""
    ref = moments_ref(x)
    bnd = moments_bound(x, ref)
    assert torch.equal(got["count"], ref["count"]), (what, got["count"][:4], ref["count"][:4])
    worst = 0.0
    for name in ("mean", "m2", "std"):
        worst = max(worst, check(got[name], ref[name], bnd[name], f"{what} {name}", key=None if key is None else (key[0], f"{key[1]} {name}"))[0])
    return worst


def state_dict_of(state):
    """a [c, 3] float64 state (count, mean, M2) -> dict(count, mean, m2, std)"""
    s = state.detach().cpu().to(F64)
    return dict(count=s[:, 0].clone(), mean=s[:, 1].clone(), m2=s[:, 2].clone(), std=torch.sqrt(s[:, 2].clamp_min(0.0) / s[:, 0]))
