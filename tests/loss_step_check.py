"""Element-by-element check of the loss kernels (zett_amd/csrc/train_loss.hip) and of the distance losses and the optimizer step
(zett_amd/csrc/train_step.hip) against float64 on the SAME values (no GPU in here): the sibling of tests/train_ops_check.py, whose
checks (`check`, `exact`, `check_canary`, `check_slack`), buffers (`Frame`), unit U and record mechanism it uses as they are.

Every reference is plain torch on the CPU from exactly the values the kernel is given: fp32 inputs as they are, 16-bit inputs
widened, scalars a kernel reads from a `record` as the fp32 values in it.  Each takes `dt`: float64 is the reference, float32 the
EMULATION the bounds are sized against — the same formulas in fp32 with every long sum taken IN THE ORDER THE KERNEL DOCUMENTS
(`_ce_stats32`, `lane_sum`, `sumsq32` restate it).  tests/test_loss_step_check_host.py asserts that the emulation stays below a
quarter of every bound that holds a long sum, and below half of every bound that is a handful of roundings (a word of a record,
an element of G, dpred or the AdamW outputs): U is the round-off twice over, so a RIGHT kernel whose few operations all round the
same way reaches exactly half of "one U per operation", and a quarter cannot be promised there.

The bounds, per element, by the rules at the top of tests/train_ops_check.py, and what those do not cover:

  * an fp32 sum in a documented fixed order: (d + 2) U sum |terms|, d the longest chain of additions an element passes through;
    d is stated at `ce_depth` (ce_rows_kernel), `dist_depth` (dist_rows_kernel) and `sumsq_depth` (sumsq_kernel) with the lines
    it was read from;
  * a float64 sum of fp32 inputs rounded once to fp32 (ce_finalize, dist_finalize, norm_finalize): U |x| for the rounding, one U
    more per further fp32 operation, and n 2^-52 sum |terms| for the float64 sum itself (`once`);
  * __expf / logf: exp(x) carries (A_EXP + |x|) U exp(x) (the |x| for the rounded argument), log s carries A_LOG U |log s|; the
    bounds of lse, row_loss and G are these propagated through the formulas (`ce_rows_bound`) times C_CE_LSE, C_CE_LOSS, C_CE_G.
    The emulation uses torch's exp / log: what the device intrinsics add is what the constants are for;
  * AdamW and the distance losses: one U per operation through the written formula on float64 intermediates, in magnitudes
    (b1 m + (1 - b1) g' may cancel), times C_ADAMW / C_DIST.
The rule for the five constants is the project's: the smallest of {1, 2, 4, 8} that leaves the largest err / bound observed on the
device over every case of tests/test_loss_step_direct_gpu.py at or below 0.5; profiles/loss_step_check.md holds the figures.

Exact (`exact`): argmax, n_correct, n_counted, skip, the step count, single_token_mask, every "is zero" promise (pad columns, rows
of weight 0, cleared gradients), ce_addend (two IEEE additions in the documented order, contraction off in the kernel), ce_scale
(two IEEE multiplications and a conversion), ce_cast, and every buffer a call must leave alone.

The case tables of the GPU test are built here, without a GPU; the host test restates the dispatch rules and asserts that the
tables reach every branch.
"""
from __future__ import annotations

import itertools

import torch

from tests import train_ops_check as tc
from tests.train_ops_check import (CANARY16, CANARY_BITS, LO, RECORD, U, CanaryBroken, Frame, OpMismatch, check, check_canary,      # noqa: F401 (re-exported)
                                   check_slack, exact, fma_bound, lo_bound, sum_bound, write_record)

F64, F32 = torch.float64, torch.float32
RECORD_ENV = "ZETT_LOSS_STEP_CHECK_RECORD"        # read like train_ops_check.RECORD_ENV; the record itself is train_ops_check.RECORD
TINY = 2.0 ** -148                               # two steps of the fp32 subnormals: the U of a result down there (a step is its round-off twice over, two operations end there)
DT = {"f32": F32, "f16": torch.float16, "bf16": torch.bfloat16}
DT_CODE = {"f32": 0, "f16": 1, "bf16": 2}        # zett_dtype
MSE, RMSE, HUBER = 0, 1, 2                       # zett_distance
MEAN, LEXICAL = 0, 1                             # zett_loss_mode
DECAY, FROZEN = 1, 2                             # zett_adamw_flags
CE_AUTO, CE_ONCE, CE_TWICE = 0, 1, 2
CE_ONCE_MAX = 32768
MT_CHUNK, MT_GROUP, MT_GRID = 65536, 64, 2048

C_CE_LSE = 1.0
C_CE_LOSS = 1.0
C_CE_G = 1.0
C_ADAMW = 1.0
C_DIST = 1.0
A_EXP, A_LOG = 2.0, 2.0

# the slice limits of the wrapper tests (tests/test_lm_loss_gpu.py FWD_LIMIT, tests/test_training_gpu.py)
REL_LOSS, REL_DIST_GRAD, REL_ADAMW = 1e-5, 1e-5, 5e-5


def f32(x):
    """the fp32 value of a python scalar, as a python float"""
    return float(torch.tensor(x, dtype=F32))


def once(value, n=0, mag=None, ops=1):
    """a float64 result rounded to fp32 (`ops` fp32 roundings in all), its float64 sum over n terms of magnitude sum `mag`"""
    value = torch.as_tensor(value, dtype=F64)
    return ops * U * value.abs() + (0.0 if mag is None else n * 2.0 ** -52 * torch.as_tensor(mag, dtype=F64)) + TINY


class Slim(Frame):
    """train_ops_check.Frame with `slack` rows of ld elements around the view instead of 256: the rows of ce_rows are up to 32 772
    columns wide, and eight such rows are already 64 tiles of slack"""

    def __init__(self, rows, cols, ld, dtype, fill, slack=8, shift=0, values=None):
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        assert ld >= cols and shift >= 0 and slack >= 1
        self.offset = slack * ld + shift
        total = self.offset + (rows + slack) * ld
        if fill == "canary":
            self.buf = (torch.full((total,), CANARY_BITS, dtype=torch.int32).view(F32) if dtype == F32 else torch.full((total,), CANARY16, dtype=torch.int16).view(dtype))
        else:
            self.buf = torch.full((total,), float(fill), dtype=dtype)
        if values is not None:
            self.view(self.buf).copy_(values)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def check_outside(frame, after, what):
    """an INPUT the call may write inside its view (logits overwritten by G): everything outside the view keeps its bits"""
    a, b = _bits(after).clone(), _bits(frame.buf).clone()
    frame.view(a).fill_(0)
    frame.view(b).fill_(0)
    rel = torch.nonzero(a != b).flatten() - frame.offset
    if rel.numel():
        where = [(0, int(i)) if frame.rows is None else (int(i) // frame.ld, int(i) % frame.ld) for i in rel]
        raise CanaryBroken(f"{what}: {len(where)} element(s) outside the [{frame.rows}, {frame.cols}] view (ld {frame.ld}) changed, first at (row, column) {where[:4]}", where)


def unchanged(after, before, what):
    """a buffer a call must leave alone: the whole allocation keeps its bits (NaN slack included)"""
    a, b = _bits(after).flatten(), _bits(before).flatten()
    bad = torch.nonzero(a != b).flatten()
    if bad.numel():
        raise CanaryBroken(f"{what}: {bad.numel()} element(s) of a buffer the call must not write changed, first at element {int(bad[0])}", [(0, int(i)) for i in bad[:4]])


# ---- ce_rows ---------------------------------------------------------------------------------------------------------------------
K_LOWEST = float(torch.finfo(torch.float32).min)      # the kernel's kLowest


def ce_nv(v_padded, path=CE_AUTO):
    """zett_op_ce_rows' dispatch (train_loss.hip:333-343): -> NV, the float4 per lane of the read-once path (0: the two-read path)"""
    if path == CE_TWICE or (path == CE_AUTO and v_padded > CE_ONCE_MAX):
        return 0
    per_lane = (v_padded // 4 + 1023) // 1024
    return 1 if per_lane <= 1 else 2 if per_lane <= 2 else 4 if per_lane <= 4 else 8


def ce_lane_vectors(v_padded):
    """the vectors a lane absorbs that can hold a column (both paths: vector i * 1024 + lane, i in column order)"""
    return (v_padded // 4 + 1023) // 1024


def ce_depth(v_padded):
    """-> (d, R) of ce_rows_kernel.  d, the longest chain of fp32 additions behind the row's sum of exponentials: per absorbed
    vector the pairwise sum of four (2) and the addition to the lane's sum (1) (absorb, train_loss.hip:71), six levels of the wave
    butterfly and four of the sixteen wave results (block_combine, :77-96): 3 n + 10 for n vectors per lane.  R, the rescalings
    s * exp(m - m') a term passes through: one per absorbed vector (:68) and one per level (combine, :52): n + 10."""
    n = ce_lane_vectors(v_padded)
    return 3 * n + 10, n + 10


def _ce_stats32(z, v):
    """(max, sum of exp(z - max)) of every row in fp32 in the kernel's documented order: per lane an online pass over its vectors in
    column order (absorb), then the butterfly over the 64 lanes of a wave and over the 16 waves (block_combine / combine)"""
    rows, vp = z.shape
    n = ce_lane_vectors(vp)
    zz = torch.full((rows, n * 4096), -float("inf"), dtype=F32)
    zz[:, :v] = z[:, :v]
    zz = zz.view(rows, n, 1024, 4)
    m, s = torch.full((rows, 1024), K_LOWEST, dtype=F32), torch.zeros(rows, 1024, dtype=F32)
    for i in range(n):
        q = zz[:, i]
        mn = torch.maximum(m, q.max(-1).values)
        s = s * torch.exp(m - mn)
        ex = torch.exp(q - mn[..., None])
        s = s + ((ex[..., 0] + ex[..., 1]) + (ex[..., 2] + ex[..., 3]))
        m = mn

    def comb(m, s, perm):
        mo, so = m[:, perm], s[:, perm]
        big = torch.maximum(m, mo)
        return big, torch.where(m == big, s, s * torch.exp(m - big)) + torch.where(mo == big, so, so * torch.exp(mo - big))

    lane = torch.arange(1024)
    for off in (32, 16, 8, 4, 2, 1):
        m, s = comb(m, s, lane ^ off)
    m, s = m[:, ::64].contiguous(), s[:, ::64].contiguous()
    wave = torch.arange(16)
    for off in (8, 4, 2, 1):
        m, s = comb(m, s, wave ^ off)
    return m[:, 0], s[:, 0]


def first_argmax(x):
    """the lowest column holding the row's maximum"""
    cols = torch.arange(x.shape[1])
    return torch.where(x == x.max(1, keepdim=True).values, cols, x.shape[1]).min(1).values.to(torch.int32)


def ce_rows_ref(z, labels, weight, v, dt=F64):
    """z [rows, v_padded] fp32, of which only the columns < v exist.  -> dict(lse, loss, argmax, G [rows, v_padded], and the
    intermediates the bound needs).  A label outside [0, v) is an all-zero one-hot; a row of weight 0 (either sign) has loss +0 and
    G all +0: the header says "all zero" / "row_loss 0", and the kernel writes the literal 0.f there, so +0 BITS are asked for."""
    rows, vp = z.shape
    x = z[:, :v].to(dt)
    if dt == F64:
        m = x.max(1).values
        s = torch.exp(x - m[:, None]).sum(1)
    else:
        m, s = _ce_stats32(z, v)
    lse = m + torch.log(s)
    w = torch.ones(rows, dtype=dt) if weight is None else weight.to(dt)
    lab = labels.long()
    hit = (lab >= 0) & (lab < v)
    zl = torch.where(hit, x.gather(1, lab.clamp(0, v - 1)[:, None])[:, 0], torch.zeros(rows, dtype=dt))
    live = w != 0
    loss = torch.where(live, w * (lse - zl), torch.zeros(rows, dtype=dt))
    p = torch.exp(x - lse[:, None])
    oh = (torch.arange(v)[None, :] == lab[:, None]).to(dt)
    G = torch.zeros(rows, vp, dtype=dt)
    G[:, :v] = torch.where(live[:, None], w[:, None] * (p - oh), torch.zeros_like(p))
    return dict(lse=lse, loss=loss, argmax=first_argmax(z[:, :v]), G=G, x=x, m=m, s=s, w=w, zl=zl, p=p, oh=oh, live=live)


def ce_rows_bound(ref, v_padded):
    """From the float64 intermediates, with M the row maximum, e_j = exp(x_j - M), s = sum e_j, (d, R) = ce_depth:
        a term as it arrives in s: its own exp, R rescalings by an exp (each with the product's rounding), d additions:
                 bs = U sum_j e_j ((A_EXP + |x_j - M|) + R (A_EXP + 1) + (d + 2))
        lse = M + log s:                   bl = bs / s + A_LOG U |log s| + U |lse|
        row_loss = w (lse - z_label):      |w| (bl + U |lse - z_label|) + U |row_loss|
        p_j = exp(x_j - lse):              bp_j = p_j ((A_EXP + |x_j - lse|) U + bl)
        G_j = w (p_j - onehot_j):          |w| (bp_j + U |p_j - onehot_j|) + U |G_j|
    times C_CE_LSE, C_CE_LOSS, C_CE_G.  -> dict(lse, loss, G): G is the bound of the fp32 value (a 16-bit G: lo_bound of it)"""
    d, R = ce_depth(v_padded)
    x, m, s, w, p, lse = (ref[k].to(F64) for k in ("x", "m", "s", "w", "p", "lse"))
    dx = (x - m[:, None]).abs()
    bs = U * (torch.exp(-dx) * ((A_EXP + dx) + R * (A_EXP + 1) + (d + 2))).sum(1)
    bl = bs / s + A_LOG * U * torch.log(s).abs() + U * lse.abs()
    b_loss = w.abs() * (bl + U * (lse - ref["zl"].to(F64)).abs()) + U * ref["loss"].to(F64).abs() + TINY
    bp = p * ((A_EXP + (x - lse[:, None]).abs()) * U + bl[:, None])
    bG = torch.zeros_like(ref["G"], dtype=F64)
    v = x.shape[1]
    bG[:, :v] = torch.where(ref["live"][:, None], w.abs()[:, None] * (bp + U * (p - ref["oh"].to(F64)).abs()) + U * ref["G"][:, :v].to(F64).abs() + TINY, torch.zeros_like(p))
    return dict(lse=C_CE_LSE * bl, loss=C_CE_LOSS * torch.where(ref["live"], b_loss, torch.zeros_like(b_loss)), G=C_CE_G * bG)


CE_WIDTHS = (4, 4092, 4096, 4100, 8192, 8196, 16384, 16388, 32768, 32772)
CE_G_FORMS = (None, "f32", "inplace", "bf16", "f16")
CE_WEIGHTS = (1.0, 0.0, -0.0, 1e-40, 2.5)          # (1e-40: an fp32 subnormal)
CE_LABELS = ("0", "v-1", "v", "vp-1", "-100", "-1", "2^31-1", "lane_last", "next_lane_first")


def ce_edge_columns(v, v_padded):
    """-> (the last column of a lane's last vector, the first column of the next lane's vector), both real columns where the row
    has them"""
    nvec = v_padded // 4
    q = max(0, min((max(nvec // 1024, 1) - 1) * 1024 + 5, nvec - 2))          # lane 5's last vector at every width of CE_WIDTHS (nvec % 1024 <= 5 or nvec < 1024)
    return min(4 * q + 3, v - 1), min(4 * q + 4, v - 1)


def ce_label(name, v, v_padded):
    last, nxt = ce_edge_columns(v, v_padded)
    return {"0": 0, "v-1": v - 1, "v": v, "vp-1": v_padded - 1, "-100": -100, "-1": -1, "2^31-1": 2 ** 31 - 1, "lane_last": last, "next_lane_first": nxt}[name]


def ce_cases():
    """every width x v in {v_padded, v_padded - 1, v_padded - 3}: 3 to 5 rows, ld_z / ld_g tight and + 4, the five forms of g, the pad
    columns NaN (even widths of the table) or +inf, weights NULL in every third case"""
    out = []
    for i, (vp, dv) in enumerate(itertools.product(CE_WIDTHS, (0, 1, 3))):
        g = CE_G_FORMS[i % 5]
        d_z = 4 * (i % 2)
        out.append(dict(i=i, vp=vp, v=vp - dv, rows=3 + i % 3, d_z=d_z, d_g=d_z if g == "inplace" else 4 * ((i // 2) % 2), g=g, pad="nan" if (i // 3) % 2 == 0 else "inf",
                        weights=i % 3 != 0))
    return out


def ce_inputs(case):
    """-> (z [rows, vp] with its pad columns filled, labels int32 [rows], weight fp32 [rows] or None).  Every row has ONE maximum,
    1.0 above the next value, in an edge column (or at its label)."""
    i, vp, v, rows = case["i"], case["vp"], case["v"], case["rows"]
    g = torch.Generator().manual_seed(1000 + i)
    z = torch.randn(rows, vp, generator=g) * 2
    labels = torch.tensor([ce_label(CE_LABELS[(5 * i + r) % len(CE_LABELS)], v, vp) for r in range(rows)], dtype=torch.int64)
    last, nxt = ce_edge_columns(v, vp)
    for r in range(rows):
        lab = int(labels[r])
        peak = (0, v - 1, last, nxt, lab if 0 <= lab < v else v // 2)[(i + r) % 5]
        z[r, peak] = z[r, :v].max() + 1.0
    z[:, v:] = float("nan") if case["pad"] == "nan" else float("inf")
    weight = torch.tensor([CE_WEIGHTS[(i + r) % 5] for r in range(rows)], dtype=F32) if case["weights"] else None
    return z, labels.to(torch.int32), weight


CE_SPECIAL = dict(vp=8196, v=8195, rows=10)
CE_TIES = ((8, 9), (12, 12 + 4096), (4 * 3 + 1, 4 * 40 + 2), (4 * 5, 4 * (64 * 3 + 5) + 3), (0, 8194))     # in one float4, in one lane's vectors i and i + 1, two lanes of a wave, two waves, first and last real column


def ce_special():
    """ten rows of 8195 columns (NV = 4): the five ties of CE_TIES (bit-identical maxima of 20.0), a constant row, a row whose
    maximum is in column v - 1 with 1e30 in the pad column v, a row with the -100000 mask fill on a fifth of its columns, a row
    of magnitude 1e4, a row whose only unmasked column is its label.  -> (z, labels, expected argmax)"""
    vp, v, rows = CE_SPECIAL["vp"], CE_SPECIAL["v"], CE_SPECIAL["rows"]
    g = torch.Generator().manual_seed(77)
    z = (torch.randn(rows, vp, generator=g) * 2).clamp(-9, 9)
    z[:, v:] = float("nan")
    want = []
    for r, (a, b) in enumerate(CE_TIES):
        z[r, a] = z[r, b] = 20.0
        want.append(a)
    z[5, :v] = 0.5
    want.append(0)
    z[6, v - 1], z[6, v] = 20.0, 1e30
    want.append(v - 1)
    z[7, :v] = torch.where(torch.rand(v, generator=g) < 0.2, torch.full((v,), -100000.0), z[7, :v])
    z[7, 3] = 20.0
    want.append(3)
    z[8, :v] = torch.randn(v, generator=g) * 1e4
    z[8, 77] = z[8, :v].max() + 100.0
    want.append(77)
    z[9, :v] = -100000.0
    z[9, 1234] = 3.0
    want.append(1234)
    labels = torch.tensor([8, 9, -100, 20, v - 1, 0, v - 1, 3, 77, 1234], dtype=torch.int32)
    return z, labels, torch.tensor(want, dtype=torch.int32)


CE_STRIDE = dict(rows=65536 + 70, v=5, vp=8)


def ce_stride():
    rows, v, vp = CE_STRIDE["rows"], CE_STRIDE["v"], CE_STRIDE["vp"]
    g = torch.Generator().manual_seed(5)
    z = torch.randn(rows, vp, generator=g) * 2
    r = torch.arange(rows)
    z[r, r % v] = z[:, :v].max(1).values + 1.0
    z[:, v:] = float("nan")
    labels = ((r * 7) % 8 - 2).to(torch.int32)                        # -2 .. 5: below, inside and at v
    weight = torch.where(r % 11 == 0, torch.zeros(rows), torch.rand(rows, generator=g) + 0.5).to(F32)
    return z, labels, weight


def top_two_gap(z, v):
    """the relative gap between the two largest real values of every row"""
    t = z[:, :v].double().topk(min(2, v), dim=1).values
    return (t[:, 0] - t[:, -1]) / t[:, 0].abs().clamp_min(1e-300) if v > 1 else torch.ones(z.shape[0], dtype=F64)


# ---- the small kernels of the loss ---------------------------------------------------------------------------------------------
def addend_ref(bias, priors, mask, v, v_padded):
    """fp32, in the kernel's order: the mask term, + bias, + priors (two IEEE additions, contraction off): exact"""
    a = torch.zeros(v, dtype=F32)
    if mask is not None:
        a = torch.where(mask != 0, torch.zeros(v), torch.full((v,), -100000.0))
    if bias is not None:
        a = a + bias
    if priors is not None:
        a = a + priors
    return torch.cat([a, torch.zeros(v_padded - v, dtype=F32)])


def ce_finalize_ref(row_loss, weight, labels, argmax):
    """-> (values float64 [3], bounds [3], n_correct, n_counted).  w > 0 counts: a negative weight and both zeros do not (the header:
    "n_counted = rows with w > 0").  sum(w) == 0: loss 0 and 1 / sum(w) = 0."""
    n = row_loss.shape[0]
    w = torch.ones(n, dtype=F64) if weight is None else weight.double()
    sl, sw = row_loss.double().sum(), w.sum()
    counted = w > 0
    nc, nn = int((counted & (argmax == labels)).sum()), int(counted.sum())
    if float(sw) == 0.0:
        return torch.tensor([0.0, 0.0, 0.0], dtype=F64), torch.zeros(3, dtype=F64), nc, nn
    vals = torch.stack([sl / sw, sw, 1.0 / sw])
    ml, mw = row_loss.double().abs().sum(), w.abs().sum()
    rel = n * 2.0 ** -52 * (ml / sl.abs().clamp_min(1e-300) + mw / sw.abs())
    return vals, once(vals) + vals.abs() * rel, nc, nn


def scale_ref(x, record2, upstream, dtype):
    """(dtype)(x * (upstream * record[2])): two fp32 multiplications and a conversion, exact"""
    f = torch.tensor(upstream, dtype=F32) * torch.tensor(record2, dtype=F32)
    return (x * f).to(dtype)


def cast_ref(x, cols_padded, dtype):
    """through float: values are kept, a NaN's payload need not be (the tests feed no NaN)"""
    return torch.cat([x.float().to(dtype), torch.zeros(x.shape[0], cols_padded - x.shape[1], dtype=dtype)], 1)


# ---- the distance losses -------------------------------------------------------------------------------------------------------
HUBER_DELTA = f32(1e-3)
DIST_E = (1, 3, 4, 5, 252, 256, 260, 1023, 1028)
DIST_N = (1, 3, 4, 5, 9)
DIST_SWITCHES = ("none", "pred_shift", "ld_pred", "src_shift1", "src_shift2", "src_shift3", "ld_src", "col0_1", "col0_2", "col0_3", "dpred_shift", "ld_dpred")
DIST_SRC_ROWS = 6
DIST_IDS = (-1, -2 ** 40, DIST_SRC_ROWS, DIST_SRC_ROWS + 7, 2 ** 40, 0, DIST_SRC_ROWS - 1, 2, 3)
DIST_MASKS = (None, "binary", "real", "zero")
DIST_STRIDE = dict(n=8192 + 9, e=8)


def up4(x):
    return (x + 3) // 4 * 4


def not4(x):
    """the smallest leading dimension above x that is no multiple of four"""
    return x + 1 if (x + 1) % 4 else x + 2


def _dist_case(i, j, k, e, kind, sd, sw):
    col0 = int(sw[-1]) if sw.startswith("col0") else 4 * (j % 2)
    c = dict(i=i, e=e, kind=kind, sd=sd, switch=sw, n=DIST_N[(j + k) % 5], ids64=(j + k) % 2 == 1, ids_stride=1 if (j // 2 + k) % 2 == 0 else 3, mask=DIST_MASKS[(j + k) % 4],
             col0=col0, pred_shift=1 if sw == "pred_shift" else 0, ld_pred=not4(e) if sw == "ld_pred" else up4(e) + 4 * (j % 2),
             src_shift=int(sw[-1]) if sw.startswith("src_shift") else 0, dpred_shift=1 if sw == "dpred_shift" else 0,
             ld_dpred=(e + 2 if (e + 2) % 4 else e + 3) if sw == "ld_dpred" else up4(e) + 4 * ((j + 1) % 2))
    c["ld_src"] = not4(col0 + e) if sw == "ld_src" else up4(col0 + e) + 4
    return c


DIST_VECTOR_E = (5, 260, 1023)        # the 4-element accesses with one pass and a scalar end, two passes, four passes and a scalar end


def dist_cases():
    """every e x kind x source dtype; per (e, kind) one of DIST_SWITCHES — each switches vec_ok off ALONE —, n, the id type and stride
    and the mask cycling along the table.  Then, for every kind and source dtype, the 4-element accesses left ON at DIST_VECTOR_E."""
    out = []
    for j, (e, kind) in enumerate(itertools.product(DIST_E, (MSE, RMSE, HUBER))):
        for k, sd in enumerate(("f32", "f16", "bf16")):
            out.append(_dist_case(3 * j + k, j, k, e, kind, sd, DIST_SWITCHES[(j // 3 + 4 * kind) % len(DIST_SWITCHES)]))
    for j, (e, kind) in enumerate(itertools.product(DIST_VECTOR_E, (MSE, RMSE, HUBER))):
        for k, sd in enumerate(("f32", "f16", "bf16")):
            out.append(_dist_case(len(out), j + 1, k, e, kind, sd, "none"))
    return out


def dist_vec_ok(c, grad):
    """dist_args (train_step.hip:320-321) and zett_op_embed_dist_grad (:373), on frames whose unshifted base is 16-byte aligned"""
    es = 4 if c["sd"] == "f32" else 2
    ok = (4 * c["pred_shift"]) % 16 == 0 and c["ld_pred"] % 4 == 0 and (es * c["src_shift"]) % (4 * es) == 0 and c["ld_src"] % 4 == 0 and c["col0"] % 4 == 0
    return ok and (not grad or ((4 * c["dpred_shift"]) % 16 == 0 and c["ld_dpred"] % 4 == 0))


def dist_vec_terms(c):
    """the terms of vec_ok one by one: -> dict(name -> holds)"""
    es = 4 if c["sd"] == "f32" else 2
    return dict(pred=(4 * c["pred_shift"]) % 16 == 0, ld_pred=c["ld_pred"] % 4 == 0, src=(es * c["src_shift"]) % (4 * es) == 0, ld_src=c["ld_src"] % 4 == 0, col0=c["col0"] % 4 == 0,
                dpred=(4 * c["dpred_shift"]) % 16 == 0, ld_dpred=c["ld_dpred"] % 4 == 0)


def clamp_rows(ids, src_rows):
    return ids.long().clamp(0, src_rows - 1)


def dist_inputs(c):
    """-> dict(src [src_rows, ld_src] in the source type, NaN outside the block; ids [n, ids_stride] (unused columns a wild row);
    pred fp32 [n, e]; mask; tgt fp32 [n, e]).  Column 0 of the block is 0 in every source row, so that pred = +-1e-3f there is an
    error of EXACTLY Huber's knee in rows 0 and n - 1; row 1 equals its target (error exactly 0: the RMSE gradient is 0); the
    other errors are 1.5e-3 N(0, 1), inside and outside the knee."""
    n, e, col0 = c["n"], c["e"], c["col0"]
    g = torch.Generator().manual_seed(500 + c["i"])
    dt = DT[c["sd"]]
    src = torch.full((DIST_SRC_ROWS, c["ld_src"]), float("nan"), dtype=dt)
    block = (torch.randn(DIST_SRC_ROWS, e, generator=g) * 0.05).to(dt)
    block[:, 0] = 0
    src[:, col0:col0 + e] = block
    idt = torch.int64 if c["ids64"] else torch.int32
    info = torch.iinfo(idt)
    vals = [max(info.min, min(info.max, DIST_IDS[(c["i"] + r) % len(DIST_IDS)])) for r in range(n)]
    ids = torch.full((n, c["ids_stride"]), 2 ** 45 if c["ids64"] else 10 ** 9, dtype=idt)
    ids[:, 0] = torch.tensor(vals, dtype=idt)
    tgt = block.float()[clamp_rows(ids[:, 0], DIST_SRC_ROWS)]
    pred = tgt + 1.5e-3 * torch.randn(n, e, generator=g)
    pred[0, 0] = HUBER_DELTA
    pred[n - 1, 0] = -HUBER_DELTA if n > 1 else HUBER_DELTA
    if n > 1:
        pred[1] = tgt[1]
    mask = {None: None, "binary": (torch.arange(n) % 2 == 0).float(), "real": torch.where(torch.arange(n) % 2 == 0, 0.5, 2.0).float(), "zero": torch.zeros(n)}[c["mask"]]
    return dict(src=src, ids=ids, pred=pred, mask=mask, tgt=tgt)


def dist_depth(e, vec_ok):
    """the longest chain of additions in dist_rows_kernel (train_step.hip:62-76): per pass over 256 columns the pairwise sum of
    four and the addition to the lane's sum (3), per pass of the 64-column scalar loop one, six levels of wave_sum"""
    tail = (e & ~3) if vec_ok else 0
    return 3 * ((tail + 255) // 256) + (e - tail + 63) // 64 + 6


def lane_sum(t, vec_ok):
    """the row sums of t [n, e]; float32: in dist_rows_kernel's order (the vector passes, the scalar passes, wave_sum's butterfly)"""
    if t.dtype != F32:
        return t.sum(1)
    n, e = t.shape
    tail = (e & ~3) if vec_ok else 0
    acc = torch.zeros(n, 64, dtype=F32)
    if tail:
        it = (tail + 255) // 256
        q = torch.zeros(n, it * 256, dtype=F32)
        q[:, :tail] = t[:, :tail]
        q = q.view(n, it, 64, 4)
        for k in range(it):
            acc = acc + ((q[:, k, :, 0] + q[:, k, :, 1]) + (q[:, k, :, 2] + q[:, k, :, 3]))
    if e - tail:
        it = (e - tail + 63) // 64
        q = torch.zeros(n, it * 64, dtype=F32)
        q[:, :e - tail] = t[:, tail:]
        q = q.view(n, it, 64)
        for k in range(it):
            acc = acc + q[:, k]
    for w in (32, 16, 8, 4, 2, 1):
        acc = acc[:, :w] + acc[:, w:2 * w]
    return acc[:, 0]


def _dist_term(err, kind):
    """-> (term, |d term / d err|)"""
    if kind == HUBER:
        a = err.abs()
        q = a.clamp(max=HUBER_DELTA)
        return 0.5 * q * q + HUBER_DELTA * (a - q), q
    return err * err, 2 * err.abs()


def dist_rows_ref(pred, tgt, mask, kind, vec_ok, dt=F64):
    """-> dict(dist, tnorm, b_dist, b_tnorm).  Bounds (float64 run), with d = dist_depth:
        err = pred - target: U |err|; a term: U (|err| |term'| + 3 |term|); their sum: + (d + 2) U sum terms
        RMSE: the square root halves the relative error, + U; Huber: / 1e-3f / 30: + 2 U; the mask: + U
        tnorm = sqrt(sum t^2): ((d + 3) U sum t^2) through the root, + U            each times C_DIST"""
    err = pred.to(dt) - tgt.to(dt)
    term, slope = _dist_term(err, kind)
    s = lane_sum(term, vec_ok)
    dist = torch.sqrt(s) if kind == RMSE else (s / HUBER_DELTA / 30.0 if kind == HUBER else s)
    if mask is not None:
        dist = dist * mask.to(dt)
    t2 = lane_sum(tgt.to(dt) * tgt.to(dt), vec_ok)
    out = dict(dist=dist, tnorm=torch.sqrt(t2))
    if dt == F64:
        d = dist_depth(pred.shape[1], vec_ok)
        bs = U * (err.abs() * slope + 3 * term).sum(1) + (d + 2) * U * s
        root = torch.sqrt(s)
        b = torch.where(s > 0, 0.5 * bs / root.clamp_min(1e-300), torch.zeros_like(s)) + U * root if kind == RMSE else (bs / HUBER_DELTA / 30.0 + 2 * U * s / HUBER_DELTA / 30.0 if kind == HUBER else bs)
        if mask is not None:
            b = b * mask.double().abs() + U * dist.abs()
        rt = torch.sqrt(t2)
        out["b_dist"] = C_DIST * b + TINY
        out["b_tnorm"] = C_DIST * (torch.where(t2 > 0, 0.5 * (d + 3) * U * t2 / rt.clamp_min(1e-300), torch.zeros_like(t2)) + U * rt) + TINY
    return out


def dist_finalize_ref(row_dist, row_tnorm, mask, mode):
    """-> (values float64 [4], bounds [4]): { loss, 1 / denom, sum(mask) / n, 0 }, float64 sums rounded once"""
    n = row_dist.shape[0]
    sd, st = row_dist.double().sum(), row_tnorm.double().sum()
    sm = mask.double().sum() if mask is not None else torch.tensor(float(n), dtype=F64)
    denom = (sm + 1e-8) * (st / n) if mode == LEXICAL else torch.tensor(float(n), dtype=F64)
    vals = torch.stack([sd / denom, 1.0 / denom, sm / n, torch.tensor(0.0, dtype=F64)])
    b = once(vals) + n * 2.0 ** -52 * torch.stack([row_dist.double().abs().sum() / denom.abs(), 1.0 / denom.abs(), sm.abs() / n, torch.tensor(0.0, dtype=F64)])
    b[3] = 0.0
    return vals, b


def dist_grad_ref(pred, tgt, mask, row_dist, kind, record1, upstream, dt=F64):
    """dpred = f * grad(err), f = upstream * record[1] * mask (Huber: / 1e-3f / 30; RMSE: * mask / row_dist, 0 where mask or row_dist
    is 0), grad = 2 err / err / clamp(err, +-1e-3f).  Six roundings at the most (the base, the mask, two for the row factor, err,
    the product): 6 U |dpred| times C_DIST.  -> (value, bound)"""
    n = pred.shape[0]
    err = pred.to(dt) - tgt.to(dt)
    m = torch.ones(n, dtype=dt) if mask is None else mask.to(dt)
    f = (torch.tensor(upstream, dtype=F32).to(dt) * torch.tensor(record1, dtype=F32).to(dt)) * m
    if kind == HUBER:
        f = f / HUBER_DELTA / 30.0
    if kind == RMSE:
        dist = row_dist.to(dt)
        ok = (m != 0) & (dist != 0)
        f = torch.where(ok, f * (m / torch.where(ok, dist, torch.ones_like(dist))), torch.zeros_like(f))
    grad = err.clamp(-HUBER_DELTA, HUBER_DELTA) if kind == HUBER else (err if kind == RMSE else 2.0 * err)
    val = f[:, None] * grad
    return val, C_DIST * 6 * U * val.double().abs() + TINY


def single_token_mask_ref(ids, width, pad):
    return (ids[:, 1:width] == pad).all(1).float()


# ---- the multi-tensor kernels ------------------------------------------------------------------------------------------------------
MT_LENGTHS = (0, 1, 3, 4, 5, 1023, 1024, 1025, 65535, 65536, 65537, 131077)
MT_EMPTY = (0, 63, 64, 65, 129) + tuple(range(20, 32))
MT_BIG = {6: 65536, 7: 65537, 8: 65537, 9: 131077, 15: 65535, 81: 65537, 96: 131077, 100: 65536, 127: 131077}
MT_ALONE = {10: (1, 0, 0, 0), 11: (0, 1, 0, 0), 12: (0, 0, 1, 0), 13: (0, 0, 0, 1)}        # (p, g, m, v) element offsets: one pointer alone 4-byte aligned
MT_PREFIXES = (0, 1, 63, 64, 65, 130)
MT_STRIDE_N = MT_GRID * MT_CHUNK + MT_CHUNK + 5
MT_PATTERN = 65537


def mt_list():
    """130 tensors: -> list of dict(n, off = (p, g, m, v) element offsets into their allocations, flags, null = frozen with NULL params
    and moments)"""
    small = (1, 3, 4, 5, 1023, 1024, 1025)
    out = []
    for i in range(130):
        n = 0 if i in MT_EMPTY else MT_BIG.get(i, small[i % 7])
        if i in MT_ALONE:
            n = 1025
        flags = (0, DECAY, FROZEN)[i % 3] if i not in MT_ALONE else (0, DECAY)[i % 2]
        off = MT_ALONE.get(i, (i % 4,) * 4)
        out.append(dict(n=n, off=off, flags=flags, null=flags == FROZEN and i % 6 == 5))
    return out


def mt_items(n):
    return (n + MT_CHUNK - 1) // MT_CHUNK


def mt_launches(lengths):
    """the launches of zett_op_grad_norm / zett_op_adamw (train_step.hip:399-416): -> list of (first entry, one past the last entry,
    [entries with elements], work items)"""
    out, first = [], 0
    while first < len(lengths):
        start, group, items = first, [], 0
        while first < len(lengths) and len(group) < MT_GROUP:
            if lengths[first]:
                group.append(first)
                items += mt_items(lengths[first])
            first += 1
        if not group:
            break
        out.append((start, first, group, items))
    return out


def sumsq_depth(aligned):
    """sumsq_kernel (train_step.hip:207-217).  A 16-byte aligned chunk: each of a thread's four sums takes 65 536 / 1024 = 64 terms,
    (s0 + s1) + (s2 + s3) two more, wave_sum six, the pairwise sum of the four waves two: 74.  A chunk that is only 4-byte aligned
    goes through s0 alone: 65 536 / 256 = 256 terms, then the same 2 + 6 + 2: 266."""
    return 74 if aligned else 266


def sumsq32(g, aligned):
    """the sum of squares of one chunk in fp32 in sumsq_kernel's order"""
    n = g.shape[0]
    sq = (g * g).to(F32)
    tail = (n & ~3) if aligned else 0
    acc = torch.zeros(256, 4, dtype=F32)
    if tail:
        it = (tail + 1023) // 1024
        q = torch.zeros(it * 1024, dtype=F32)
        q[:tail] = sq[:tail]
        q = q.view(it, 256, 4)
        for k in range(it):
            acc = acc + q[k]
    if n - tail:
        it = (n - tail + 255) // 256
        q = torch.zeros(it * 256, dtype=F32)
        q[:n - tail] = sq[tail:]
        q = q.view(it, 256)
        s0 = acc[:, 0]
        for k in range(it):
            s0 = s0 + q[k]
        acc = torch.stack([s0, acc[:, 1], acc[:, 2], acc[:, 3]], 1)
    s = ((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])).view(4, 64)
    for w in (32, 16, 8, 4, 2, 1):
        s = s[:, :w] + s[:, w:2 * w]
    return (s[0, 0] + s[1, 0]) + (s[2, 0] + s[3, 0])


def partials_ref(grads, offsets):
    """grads: the tensors of the list in order (fp32, empty ones included), offsets: the element offset of each into its 16-byte
    aligned allocation.  -> (float64 [items], bound [items]): one per started chunk in list order, empty tensors skipped;
    (d + 3) U sum g^2 (the squares round once more)"""
    vals, bnd = [], []
    for g, off in zip(grads, offsets):
        for c in range(mt_items(g.shape[0])):
            s = (g[c * MT_CHUNK:(c + 1) * MT_CHUNK].double() ** 2).sum()
            vals.append(s)
            bnd.append((sumsq_depth(off % 4 == 0) + 3) * U * s + TINY)
    if not vals:
        return torch.zeros(0, dtype=F64), torch.zeros(0, dtype=F64)
    return torch.stack(vals), torch.stack(bnd)


def norm_record_ref(partials, max_norm, b1, b2, step0):
    """from the fp32 partials the second stage is given.  -> dict(norm, coef, c1, c2: (value, bound); skip, step: int)"""
    s = partials.double().sum()
    norm = torch.sqrt(s)
    if not bool(torch.isfinite(norm)):
        step = step0
        out = dict(norm=(norm, None), coef=(torch.tensor(0.0, dtype=F64), torch.tensor(0.0, dtype=F64)), skip=1, step=step)
    else:
        step = step0 + 1
        coef = torch.tensor(1.0, dtype=F64) if float(norm) < max_norm else max_norm / norm
        out = dict(norm=(norm, once(norm, partials.numel(), s)), coef=(coef, torch.tensor(0.0, dtype=F64) if float(norm) < max_norm else once(coef, partials.numel(), 1.0)), skip=0, step=step)
    for name, b in (("c1", b1), ("c2", b2)):
        c = torch.tensor(1.0 - b ** step, dtype=F64)
        out[name] = (c, once(c) + 4 * 2.0 ** -52)
    return out


def adam_hyper(lr, b1, b2, eps, wd):
    """the fp32 values zett_op_adamw passes to its kernel"""
    return dict(lr=f32(lr), b1=f32(b1), b2=f32(b2), omb1=f32(1.0 - b1), omb2=f32(1.0 - b2), eps=f32(eps), wd=f32(wd))


def adamw_ref(p, g, m, v, h, coef, c1, c2, decay, dt=F64):
    """g' = coef g;  m' = b1 m + (1 - b1) g';  v' = b2 v + (1 - b2) g'^2;  p' = p - lr ((m' / c1) / (sqrt(v' / c2) + eps) + wd p), with
    1 / c1 and 1 / c2 formed first, as the kernel does.  coef, c1, c2: the fp32 values of the record.  -> dict(p, m, v) and, in the
    float64 run, b_p, b_m, b_v: one U per operation in magnitudes, times C_ADAMW:
        g' U;  m': the two products (the second carries g') and the sum: 2 U |b1 m| + 3 U |(1 - b1) g'|;  v': 2 U |b2 v| + 5 U (1 - b2) g'^2
        mhat = m' (1 / c1): (bm + 2 U |m'|) / c1;  vhat likewise;  the root halves vhat's relative error, + U;  + eps: + U
        the quotient, wd p, their sum, lr times it, p minus it: one U each on the magnitudes"""
    T = lambda x: torch.tensor(x, dtype=F32).to(dt)
    p, g, m, v = p.to(dt), g.to(dt), m.to(dt), v.to(dt)
    wd = T(h["wd"]) if decay else T(0.0)
    ic1, ic2 = 1.0 / T(c1), 1.0 / T(c2)
    gs = g * T(coef)
    t1, t2 = T(h["b1"]) * m, T(h["omb1"]) * gs
    m2 = t1 + t2
    u1, u2 = T(h["b2"]) * v, T(h["omb2"]) * (gs * gs)
    v2 = u1 + u2
    mhat, vhat = m2 * ic1, v2 * ic2
    root = torch.sqrt(vhat)
    den = root + T(h["eps"])
    ratio = mhat / den
    dec = wd * p
    upd = T(h["lr"]) * (ratio + dec)
    out = dict(p=p - upd, m=m2, v=v2)
    if dt == F64:
        bm = 2 * U * t1.abs() + 3 * U * t2.abs()
        bv = 2 * U * u1.abs() + 5 * U * u2.abs()
        b_mhat = (bm + 2 * U * m2.abs()) * ic1
        b_vhat = (bv + 2 * U * v2.abs()) * ic2
        b_root = torch.where(vhat > 0, 0.5 * b_vhat / root.clamp_min(1e-300), torch.zeros_like(root)) + U * root
        b_den = b_root + U * den
        b_ratio = b_mhat / den + mhat.abs() * b_den / (den * den) + U * ratio.abs()
        mag = ratio.abs() + dec.abs()
        b_upd = T(h["lr"]) * (b_ratio + U * dec.abs() + U * mag) + U * T(h["lr"]) * mag
        out["b_p"] = C_ADAMW * (b_upd + U * (p.abs() + T(h["lr"]) * mag)) + TINY
        out["b_m"], out["b_v"] = C_ADAMW * bm + TINY, C_ADAMW * bv + TINY
    return out


def mt_values(entry, i, which):
    """the parameter, gradient and moments of tensor i of mt_list: parameters at 1.0 in every fifth tensor (LayerNorm-like), a zero
    gradient with non-zero moments in the first quarter of every tensor, v = 0 with g = 0 (the denominator is eps alone) in its
    second eighth"""
    n = entry["n"]
    g = torch.Generator().manual_seed(7000 + 4 * i + which)
    if which == 0:
        return torch.ones(n) if i % 5 == 0 else torch.randn(n, generator=g) * 0.5
    if which == 1:
        x = torch.randn(n, generator=g) * 0.1
        x[:n // 4] = 0.0
        return x
    if which == 2:
        return torch.randn(n, generator=g) * 0.05
    x = torch.rand(n, generator=g) * 0.01
    x[n // 8:n // 4] = 0.0
    return x
