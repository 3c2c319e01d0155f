"""Element-by-element check of the Adafactor step (zett_amd/csrc/train_adafactor.hip, zett_op_adafactor_step) against float64 on
the SAME values (no GPU in here): the sibling of tests/loss_step_check.py, whose checks, buffers and unit U it uses as they are.

`tensor_step` is the step of one tensor from exactly the scalars the device record holds (coef, beta, 1 - beta as fp32 values).
dt = float64 is tests/adafactor_ref.py's definition with the bounds beside it; dt = float32 is the EMULATION the bounds are sized
against: the same formulas in fp32 with every sum taken IN THE ORDER train_adafactor.hip DOCUMENTS (its header table):

  tile row sum of g^2      (x0 + x1) + (x2 + x3) per lane, wave_sum                                   d = 8    `tile_sums`
  tile column sum of g^2   a lane's 16 rows top to bottom, the four waves (w0 + w1) + (w2 + w3)        d = 18   `tile_sums`
  tile sum of g^2          block_sum_pairwise of the 256 column sums                                   d = 26   `tile_sums`
  tile sum of p^2, u^2     a lane's four column sums over 16 rows, (a0 + a1) + (a2 + a3), block sum     d = 26   `tile_lane_sums`
  chunk sums               sumsq_kernel's order (loss_step_check.sumsq_depth)                          d = 74 / 266   `chunk_sums`
  segment sum of v_row     block_sum_pairwise of 256 consecutive entries                               d = 8    `segment_mean`
  second stages            float64 in index order, rounded to fp32 once (loss_step_check.once)

Bounds, by the project's rules ((d + 2) U sum |terms| for a fixed-order sum of depth d, one U more for the rounded squares; one U per
further operation through the written formula; the square roots halve a relative error).  Everything under a root here is a sum
of squares plus 1e-30, so the bounds are kept as RELATIVE errors and multiplied out at the end:

  mean of q over a row / a column     r_q  = (d + 4) U                 (d = 8 / 18: the sum, the squares, the rounding of the mean)
  v' = beta v + (1 - beta) mean       b_v  = 2 U beta v + (3 U + r_q) (1 - beta) mean
  mean(v_row)                         r_m  = max(b_v / v') + 11 U
  r_factor = (v_row / mean)^-1/2      r_r  = (b_v / v' + r_m + U) / 2 + 2 U
  c_factor = v_col^-1/2               r_c  = (b_v / v') / 2 + 2 U
  u = ((coef g) first) second         r_u  = r_r + r_c + 3 U
  flat: q = (coef g)^2 + 1e-30        b_v  = 2 U beta v + 6 U (1 - beta) q;   r_u = (b_v / v') / 2 + 4 U
  RMS(u)                              r_rms = (sum u^2 2 r_u / sum u^2 + (d + 3) U) / 2 + U
  s = max(RMS(p), 1e-3)               r_s  = (d + 3) U / 2 + 2 U
  scale = lr s / max(1, RMS(u))       r_sc = r_s + r_rms + U       (max is 1-Lipschitz: r_rms is kept on both sides of 1)
  p' = p - (scale u + wd p)           b_p  = |scale u| (r_sc + r_u + U) + U |wd p| + U (|scale u| + |wd p|) + U |p'|

times C_AF_V (v_row, v_col, v), C_AF_SCALAR (the record's norm / coef / beta) and C_AF_P (p), by the project's rule: the smallest of
{1, 2, 4, 8} that leaves the largest err / bound observed on the device over every case of tests/test_adafactor_direct_gpu.py at or
below 0.5; profiles/adafactor_check.md holds the figures.

The case tables of the GPU test are built here, without a GPU; tests/test_adafactor_check_host.py restates the dispatch rules and
asserts that the tables reach every branch.
"""
from __future__ import annotations

import torch

from tests import adafactor_ref as ref
from tests import loss_step_check as lc
from tests.train_ops_check import U

F64, F32 = torch.float64, torch.float32
RECORD_ENV = "ZETT_ADAFACTOR_CHECK_RECORD"
TINY = lc.TINY
DECAY, FROZEN = ref.DECAY, ref.FROZEN
TILE_ROWS, TILE_COLS, SEG, GROUP, VEC = 64, 256, 256, 40, 4      # ZETT_ADAFACTOR_TILE_ROWS / _TILE_COLS, kSeg, ZETT_ADAFACTOR_GROUP, float4
MT_CHUNK, MT_GRID = lc.MT_CHUNK, lc.MT_GRID
D_ROW, D_COL, D_TILE, D_SEG = 8, 18, 26, 8

C_AF_V = 1.0
C_AF_P = 1.0
C_AF_SCALAR = 1.0


def f32(x):
    return lc.f32(x)


# ---- the kernel's work decomposition, restated -------------------------------------------------------------------------------------
def is_factored(shape, flags):
    """train_adafactor.hip is_factored: not frozen and min(rows, cols) >= 128 (a 1-D tensor is [1, n])"""
    rows, cols = shape2(shape)
    return not (flags & FROZEN) and min(rows, cols) >= ref.MIN_DIM_TO_FACTOR


def shape2(shape):
    shape = tuple(shape)
    return shape if len(shape) == 2 else (1, shape[0])


def items_of(shape, flags):
    rows, cols = shape2(shape)
    if rows * cols == 0:
        return 0
    if is_factored(shape, flags):
        return -(-rows // TILE_ROWS) * -(-cols // TILE_COLS)
    return -(-rows * cols // MT_CHUNK)


def launches(entries):
    """the launch groups of zett_op_adafactor_step (make_plan): -> list of lists of entry indices, empty tensors left out"""
    out, cur = [], []
    for i, e in enumerate(entries):
        if shape2(e["shape"])[0] * shape2(e["shape"])[1] == 0:
            continue
        cur.append(i)
        if len(cur) == GROUP:
            out.append(cur)
            cur = []
    if cur:
        out.append(cur)
    return out


def tile_vec(shape, p_off, g_off):
    """tile_vec: both pointers 16-byte aligned (element offsets into 16-byte aligned allocations) and cols a multiple of four"""
    return p_off % 4 == 0 and g_off % 4 == 0 and shape2(shape)[1] % 4 == 0


# ---- ordered fp32 sums ---------------------------------------------------------------------------------------------------------------
def _halve(x):
    """wave_sum over the last axis of 64"""
    for w in (32, 16, 8, 4, 2, 1):
        x = x[..., :w] + x[..., w:2 * w]
    return x[..., 0]


def _block_pairwise(x):
    """block_sum_pairwise over the last axis of 256 threads"""
    s = _halve(x.reshape(*x.shape[:-1], 4, 64))
    return (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])


def _tiles(x):
    """[R, C] -> [ntr, 4 waves, 16 rows, ntc, 64 lanes, 4] with zeros past the edges"""
    R, C = x.shape
    ntr, ntc = -(-R // TILE_ROWS), -(-C // TILE_COLS)
    pad = torch.zeros(ntr * TILE_ROWS, ntc * TILE_COLS, dtype=x.dtype)
    pad[:R, :C] = x
    return pad.view(ntr, 4, 16, ntc, 64, 4)


def tile_sums(t):
    """t [R, C] fp32 terms (g^2) -> (rowpart [ntc, R], colpart [ntr, C], tile sums [ntr * ntc]) in af_pass1_kernel's order"""
    R, C = t.shape
    x = _tiles(t)
    ntr, ntc = x.shape[0], x.shape[3]
    q = (x[..., 0] + x[..., 1]) + (x[..., 2] + x[..., 3])
    rowpart = _halve(q).permute(3, 0, 1, 2).reshape(ntc, ntr * TILE_ROWS)[:, :R]
    acc = torch.zeros(ntr, 4, ntc, 64, 4, dtype=t.dtype)
    for k in range(16):
        acc = acc + x[:, :, k]
    col = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])                       # [ntr, ntc, 64, 4]
    colpart = col.reshape(ntr, ntc * TILE_COLS)[:, :C]
    return rowpart, colpart, _block_pairwise(col.reshape(ntr, ntc, 256)).reshape(-1)


def tile_lane_sums(t):
    """t [R, C] fp32 terms (p^2, u^2) -> tile sums [ntr * ntc] in the order of af_pass1_kernel's cp / af_pass2_kernel's acc"""
    x = _tiles(t)
    ntr, ntc = x.shape[0], x.shape[3]
    acc = torch.zeros(ntr, 4, ntc, 64, 4, dtype=t.dtype)
    for k in range(16):
        acc = acc + x[:, :, k]
    a = (acc[..., 0] + acc[..., 1]) + (acc[..., 2] + acc[..., 3])                 # [ntr, 4, ntc, 64]
    return _block_pairwise(a.permute(0, 2, 1, 3).reshape(ntr, ntc, 256)).reshape(-1)


def chunk_sum32(t, vec):
    """one chunk's fp32 terms in chunk_sum's (= sumsq_kernel's) order"""
    n = t.shape[0]
    tail = (n & ~3) if vec else 0
    acc = torch.zeros(256, 4, dtype=F32)
    if tail:
        it = (tail + 1023) // 1024
        q = torch.zeros(it * 1024, dtype=F32)
        q[:tail] = t[:tail]
        q = q.view(it, 256, 4)
        for k in range(it):
            acc = acc + q[k]
    if n - tail:
        it = (n - tail + 255) // 256
        q = torch.zeros(it * 256, dtype=F32)
        q[:n - tail] = t[tail:]
        q = q.view(it, 256)
        s0 = acc[:, 0]
        for k in range(it):
            s0 = s0 + q[k]
        acc = torch.stack([s0, acc[:, 1], acc[:, 2], acc[:, 3]], 1)
    return _block_pairwise(((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])))


def chunk_sums(t, vec):
    """flat fp32 terms -> one sum per started chunk"""
    t = t.reshape(-1)
    return torch.stack([chunk_sum32(t[c:c + MT_CHUNK], vec) for c in range(0, t.shape[0], MT_CHUNK)])


def segment_mean(v):
    """mean of v [L] as af_stats_kernel / af_tensor_kernel take it: fp32 segment sums of 256, their float64 sum, one rounding"""
    L = v.shape[0]
    if v.dtype != F32:
        return v.mean()
    segs = -(-L // SEG)
    pad = torch.zeros(segs * SEG, dtype=F32)
    pad[:L] = v
    return (_block_pairwise(pad.view(segs, SEG)).double().sum() / L).to(F32)


def _sum_items(parts, dt):
    """a second stage: the float64 sum of fp32 partials (the reference run: the partials are float64 already)"""
    return parts.double().sum()


# ---- one tensor ------------------------------------------------------------------------------------------------------------------------
def item_sums(x, shape, flags, off, dt, lanewise=False):
    """sum of x^2 per work item of a tensor.  fp32: in the kernel's order (off: the element offset of the pointer, or the OR of the
    offsets a flat pass tests together); float64: plain sums per item (the values are only ever added up)"""
    if dt == F64:
        return (x.double() ** 2).sum().reshape(1)
    sq = (x * x).to(F32)
    if is_factored(shape, flags):
        return tile_lane_sums(sq) if lanewise else tile_sums(sq)[2]
    return chunk_sums(sq, off % 4 == 0)


def tensor_step(p, g, state, flags, coef, beta, omb, lr, wd, offs=(0, 0, 0), dt=F64):
    """One tensor that is not frozen, from the record's fp32 scalars.  p, g: fp32 tensors of the parameter's shape; state: {"v"} or
    {"v_row", "v_col"} fp32; offs: element offsets (p, g, v) of the pointers into 16-byte aligned allocations (the order of the flat
    sums depends on them).  -> dict(p, state, s, rms_u, scale, sum_p2) and, in the float64 run, b_p and b_state."""
    T = lambda x: torch.tensor(x, dtype=F32).to(dt)
    shape = tuple(p.shape)
    R, C = shape2(shape)
    n = R * C
    pp, gg = p.to(dt).reshape(R, C), g.to(dt).reshape(R, C)
    wd = T(f32(wd)) if flags & DECAY else T(0.0)
    coef_t, beta_t, omb_t = T(coef), T(beta), T(omb)
    c2 = float(torch.tensor(coef, dtype=F32).double()) ** 2
    gp = gg * coef_t
    out = {}
    if is_factored(shape, flags):
        norm_rows = R <= C
        va = (state["v_row"] if norm_rows else state["v_col"]).to(dt)
        vb = (state["v_col"] if norm_rows else state["v_row"]).to(dt)
        if dt == F64:
            g2 = gg * gg
            sa, sb = g2.sum(1), g2.sum(0)
        else:
            rowpart, colpart, _ = tile_sums((gg * gg))
            sa, sb = rowpart.double().sum(0), colpart.double().sum(0)
        mqa, mqb = (c2 * sa.double() / C + ref.EPS).to(dt), (c2 * sb.double() / R + ref.EPS).to(dt)
        ta1, ta2, tb1, tb2 = beta_t * va, omb_t * mqa, beta_t * vb, omb_t * mqb
        va2, vb2 = ta1 + ta2, tb1 + tb2
        mean = segment_mean(va2 if norm_rows else vb2)
        rf = 1.0 / torch.sqrt(va2 / mean if norm_rows else va2)
        cf = 1.0 / torch.sqrt(vb2 if norm_rows else vb2 / mean)
        u = (gp * rf[:, None]) * cf[None, :] if norm_rows else (gp * cf[None, :]) * rf[:, None]
        out["state"] = {"v_row": va2 if norm_rows else vb2, "v_col": vb2 if norm_rows else va2}
        d_sum = D_TILE
        if dt == F64:
            ba = C_AF_V * (2 * U * ta1 + (3 * U + (D_ROW + 4) * U) * ta2) + TINY
            bb = C_AF_V * (2 * U * tb1 + (3 * U + (D_COL + 4) * U) * tb2) + TINY
            ra, rb = ba / va2, bb / vb2
            r_m = float((ra if norm_rows else rb).max()) + (D_SEG + 3) * U
            r_rf = 0.5 * (ra + (r_m + U if norm_rows else 0.0)) + 2 * U
            r_cf = 0.5 * (rb + (0.0 if norm_rows else r_m + U)) + 2 * U
            r_u = r_rf[:, None] + r_cf[None, :] + 3 * U
            out["b_state"] = {"v_row": ba if norm_rows else bb, "v_col": bb if norm_rows else ba}
    else:
        v = state["v"].to(dt).reshape(R, C)
        t1, t2 = beta_t * v, omb_t * (gp * gp + T(ref.EPS))
        v2 = t1 + t2
        u = gp * (1.0 / torch.sqrt(v2))
        out["state"] = {"v": v2.reshape(shape)}
        d_sum = lc.sumsq_depth((offs[1] | offs[2]) % 4 == 0)
        if dt == F64:
            bv = C_AF_V * (2 * U * t1 + 6 * U * t2) + TINY
            r_u = 0.5 * bv / v2 + 4 * U
            out["b_state"] = {"v": bv.reshape(shape)}
    sp = _sum_items(item_sums(pp, shape, flags, offs[0], dt, lanewise=True), dt)
    su = _sum_items(item_sums(u, shape, flags, offs[1] | offs[2], dt, lanewise=True), dt)
    s_raw = torch.sqrt(sp / n).to(dt)
    s = torch.maximum(s_raw, T(ref.EPS_SCALE))
    rms = torch.sqrt(su / n)
    scale = (float(torch.tensor(lr, dtype=F64)) * s.double() / max(1.0, float(rms))).to(dt)
    su_t, wp = scale * u, wd * pp
    p2 = pp - (su_t + wp)
    out.update(p=p2.reshape(shape), u=u.reshape(shape), s=float(s), s_raw=float(s_raw), rms_u=float(rms), scale=float(scale))
    if dt == F64:
        d_p = D_TILE if is_factored(shape, flags) else lc.sumsq_depth(offs[0] % 4 == 0)
        r_s = 0.5 * (d_p + 3) * U + 2 * U
        u2 = u * u
        r_rms = 0.5 * (float((u2 * 2 * r_u).sum() / su) if float(su) > 0 else 0.0) + 0.5 * (d_sum + 3) * U + U
        r_sc = r_s + r_rms + U
        b = su_t.abs() * (r_sc + r_u + U) + U * wp.abs() + U * (su_t.abs() + wp.abs()) + U * p2.abs()
        out["b_p"] = (C_AF_P * b + TINY).reshape(shape)
        out["r_scale"] = r_sc
    return out


def norm_partials(grads, entries, dt=F32):
    """gpart of the whole list in item order (fp32: the kernel's order) — what af_norm_kernel adds up in float64"""
    parts = []
    for g, e in zip(grads, entries):
        R, C = shape2(e["shape"])
        if R * C == 0:
            continue
        sq = (g.to(F32).reshape(R, C) * g.to(F32).reshape(R, C))
        parts.append(tile_sums(sq)[2] if is_factored(e["shape"], e["flags"]) else chunk_sums(sq, e["off"][1] % 4 == 0))
    return torch.cat(parts) if parts else torch.zeros(0, dtype=F32)


def record_ref(grads, max_norm, t0):
    """-> dict(norm, coef, beta, omb: (value, bound); skip, t) from the float64 gradients (lc.norm_record_ref's rules).  The norm's
    first stage is an fp32 sum per item: (d + 3) U / 2 on the root with the largest depth there is, 266."""
    s = sum((g.double() ** 2).sum() for g in grads) if grads else torch.tensor(0.0, dtype=F64)
    norm = torch.sqrt(s)
    pw = float(t0 + 1) ** -ref.DECAY_RATE
    out = dict(beta=(torch.tensor(1.0 - pw, dtype=F64), lc.once(1.0 - pw) + 4 * 2.0 ** -52), omb=(torch.tensor(pw, dtype=F64), lc.once(pw) + 4 * 2.0 ** -52))
    if not bool(torch.isfinite(norm)) or float(norm) > 3e38:
        out.update(norm=(norm, None), coef=(torch.tensor(0.0, dtype=F64), torch.tensor(0.0, dtype=F64)), skip=1, t=t0)
        return out
    r = C_AF_SCALAR * (0.5 * (266 + 3) * U + 2 * U)
    coef = torch.tensor(1.0, dtype=F64) if float(norm) < max_norm else max_norm / norm
    out.update(norm=(norm, r * norm + TINY), coef=(coef, r * coef), skip=0, t=t0 + 1)
    return out


# ---- the case tables ---------------------------------------------------------------------------------------------------------------
FACTOR_EDGE = ((127, 300), (128, 300), (300, 128), (128, 128), (129, 257), (1, 4096), (26, 256))
FLAT_1D = ((1,), (63,), (64,), (65,), (4097,), (MT_CHUNK + 5,))
TILE_EDGE = ((191, 255), (192, 256), (193, 257), (128, 259), (255, 260), (257, 261), (256, 128))      # +-1 around 3 tile heights, 1 tile width, the 256-entry segment, the vector width
FLAT_EDGE = ((3,), (4,), (5,), (1023,), (1024,), (1025,), (2, 130), (130, 2))
SHAPES = FACTOR_EDGE + FLAT_1D + TILE_EDGE + FLAT_EDGE
STRIDE_SHAPE = ((MT_GRID + 1) * TILE_ROWS - 3, TILE_COLS)      # one tile more than the grid's cap of 2 048 workgroups: the item loop strides (tiles and chunks share it)
LABEL_FLAGS = (DECAY, 0, FROZEN)
HYPER = dict(lr=1e-2, wd=0.01)


def entry(shape, flags=DECAY, off=(0, 0, 0), g_scale=0.1, p_scale=0.5, v_scale=1e-2, null=False, g_zero=False, p_zero=False):
    """off: element offsets (p, g, v / v_row / v_col) into the allocations; null: a frozen tensor handed NULL parameter and statistics"""
    return dict(shape=tuple(shape), flags=flags, off=tuple(off), g_scale=g_scale, p_scale=p_scale, v_scale=v_scale, null=null, g_zero=g_zero, p_zero=p_zero)


def single_cases():
    """every shape of SHAPES alone, labels cycling decay / no_decay, then the pointers that break the 16-byte alignment one at a time
    on a factored tensor whose width allows the 16-byte accesses and on a flat one longer than a vector pass"""
    out = [entry(s, flags=(DECAY, 0)[i % 2]) for i, s in enumerate(SHAPES)]
    for shape in ((128, 260), (1025,), (3, 700)):
        for off in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 2, 2), (3, 1, 0)):
            out.append(entry(shape, off=off))
    return out


def mixed_list():
    """every shape of SHAPES once more with frozen / decay / no_decay cycling (frozen ones of factored shape included, some with NULL
    parameters), an empty tensor, offsets cycling, and small vectors up to 2 * GROUP + 5 entries: three launch groups"""
    out = []
    for i, s in enumerate(SHAPES):
        fl = LABEL_FLAGS[i % 3]
        out.append(entry(s, flags=fl, off=(i % 4, (i // 2) % 4, (i // 3) % 4) if i % 5 == 0 else (0, 0, 0), null=fl == FROZEN and i % 2 == 0,
                         g_scale=(1e-3, 1e-1, 1e1)[i % 3]))
    out.insert(7, entry((0,), flags=DECAY))
    out.insert(20, entry((0, 5), flags=0))
    k = 0
    while len(out) < 2 * GROUP + 7:
        out.append(entry((5 + k,), flags=LABEL_FLAGS[k % 3], off=(k % 2, 0, 0)))
        k += 1
    return out


def values(e, i, which, seed=0):
    """the parameter (0), gradient (1) and statistics (2: dict) of entry i"""
    g = torch.Generator().manual_seed(9000 + 8 * i + which + 1000 * seed)
    shape = e["shape"]
    if which == 0:
        return torch.zeros(shape) if e["p_zero"] else torch.randn(shape, generator=g) * e["p_scale"]
    if which == 1:
        return torch.zeros(shape) if e["g_zero"] else torch.randn(shape, generator=g) * e["g_scale"]
    return {k: (torch.rand(s, generator=g) + 0.5) * e["v_scale"] for k, s in ref.state_shapes(shape).items()}
