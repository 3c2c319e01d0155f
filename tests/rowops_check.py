"""Element-by-element check of the forward's row kernels (zett_amd/csrc/rowops.hip.h, called one launch at a time through
zett_op_fwd_*) against float64 on the SAME values (no GPU in here): the sibling of tests/train_ops_check.py, whose machinery it
imports — Framed / Frame, check, exact, check_canary, check_slack, sum_bound, fma_bound, lo_bound, layernorm_ref, layernorm_bound,
attention_ref, U and the record — and whose rules for bounds (its module docstring) it follows: data movement, conversions and single
IEEE operations are bit-exact; a multiply-add is fma_bound; a sum of n terms in any order is sum_bound; a 16-bit value made from fp32
arithmetic is lo_bound; LayerNorm and attention propagate those through their formulas on the float64 intermediates.

Every reference takes `dt`: float64 is the reference, float32 the EMULATION (the same formulas in fp32, every sum strictly left to
right) that tests/test_rowops_check_host.py holds below a quarter of every bound.

New here:

  * buffer order.  A chunk of a plan covers vocabulary rows [row0, row0 + rows) = packed positions [tok0, tok0 + m).  Its hidden-state
    buffers hold POSITION 0 of every row first (buffer row = row - row0) and the other positions behind them in plan order
    (`chunk_row`).  `make_plan` builds a consistent plan around a chunk in the middle of a larger one; `to_buffer` / `from_buffer` move
    rows between the two orders.  References are written in plan order; what a kernel wrote is brought to plan order before the check,
    so a row in the wrong place is a wrong row;
  * the embeddings' LayerNorm in two stages, so that neither hides the other: `sum` against float64 of ((x + type0) + pos), then out_lo
    and stats against layernorm_ref of the kernel's OWN sum — the bits it normalised;
  * the readout: the bias is a sum of H products o w plus bias_b (sum_bound) plus |w| times the LayerNorm bound of o, stored exactly
    (fp32) or within lo_bound of the destination type; rows the map skips keep the canary;
  * attention: train_ops_check.attention_ref with mask = tok_key.  The forward's kernels differ from that arithmetic and
    `attention_expect` extends the bound for it, term by term (see there): the generic loop is an ONLINE softmax (a running maximum, the
    sums rescaled at every step), the fast path computes in base 2 (scaling log2 e folded into one constant, exp2);
  * ln_stats, fold_weight, gather_src as the functions below spell out.

Constants: C_FWD_LN, C_FWD_ATT (generic loop), C_FWD_ATT_FAST, C_LN_STATS multiply the propagated bounds.  The rule is the project's: the
largest err / bound observed on the device over every case of tests/test_rowops_direct_gpu.py is at most 0.5.  All start at 1.0;
profiles/rowops_check.md holds the observed ratios (written to the file named by ZETT_ROWOPS_CHECK_RECORD).
"""
from __future__ import annotations

import os

import torch

from tests import train_ops_check as tc
from tests.train_ops_check import (CANARY16, F32, F64, LO, CanaryBroken, Frame, Framed, OpMismatch, U, attention_ref, check,      # noqa: F401
                                   check_canary, check_slack, exact, fma_bound, layernorm_bound, layernorm_ref, lo_bound, sum_bound)
from tests.gemm_check import CANARY_BITS

C_FWD_LN = 1.0
C_FWD_ATT = 1.0
C_FWD_ATT_FAST = 1.0
C_LN_STATS = 1.0

RECORD_ENV = "ZETT_ROWOPS_CHECK_RECORD"
DT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
LN_KERNELS = ("rows8_32", "rows8_64", "wave", "workgroup")          # zett_ln_kernel
ATT_FAST_KEYS = 8
F16_MAX = 65504.0
RANGE_SOURCE, RANGE_WEIGHT, RANGE_DEST = 1, 8, 16


def write_record(path):
    """the fwd_* entries of the shared record (train_ops_check.RECORD): figures for profiles/rowops_check.md"""
    keep = {k: v for k, v in tc.RECORD.items() if str(k[0]).startswith("fwd_")}
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


# ---- buffer order --------------------------------------------------------------------------------------------------------
def chunk_row(t_rel, row_rel, first, rows):
    """buffer row of packed position tok0 + t_rel of vocabulary row row0 + row_rel (rowops.hip.h chunk_row): position 0 first"""
    return row_rel if first else rows + t_rel - row_rel - 1


def make_plan(lengths, keys=None, uniform=None, row0=0, tok0=0, slots=None, n_slots=5):
    """A plan whose rows [row0, row0 + len(lengths)) are the chunk: `lengths[r]` packed positions each, `keys[r]` their visibility
    (default: all visible), `uniform[r]` (a uniform row has no visible key), `slots[r]` the table slot of every position (-1 = the
    language token; default: drawn from n_slots so that positions of different rows share (slot, position) pairs).  The row0 rows in
    front hold the tok0 positions in front.  -> dict of int32 / uint8 tensors indexed as the kernels index them (row_offset
    [row0 + rows + 1], row_uniform, tok_key, tok_row, tok_slot, tok_pos, tok_pair over ALL positions), and rows, m, row0, tok0,
    offs (chunk-relative offsets), key (the chunk's tok_key), brow (buffer row of every chunk position), n_pairs."""
    rows, m = len(lengths), int(sum(lengths))
    assert all(L >= 1 for L in lengths) and (tok0 == 0 or row0 > 0) and tok0 >= row0
    front = [tok0 // row0] * row0 if row0 else []
    if row0:
        front[-1] += tok0 - sum(front)
    uniform = list(uniform) if uniform is not None else [0] * rows
    keys = [list(k) for k in keys] if keys is not None else [[0 if uniform[r] else 1] * lengths[r] for r in range(rows)]
    g = torch.Generator().manual_seed(1000 + 7 * m + rows)
    if slots is None:
        slots = [torch.randint(0, n_slots, (L,), generator=g).tolist() for L in lengths]
    for r in range(rows):
        assert len(keys[r]) == lengths[r] == len(slots[r]) and (bool(uniform[r]) == (sum(keys[r]) == 0)), (r, keys[r], uniform[r])
    offs = [0]
    for L in front + list(lengths):
        offs.append(offs[-1] + L)
    tok_row, tok_key, tok_slot, tok_pos = [], [], [], []
    for n, L in enumerate(front):
        tok_row += [n] * L; tok_key += [1] * L; tok_slot += [0] * L; tok_pos += list(range(L))
    brow = []
    for r, L in enumerate(lengths):
        t_rel0 = offs[row0 + r] - tok0
        tok_row += [row0 + r] * L; tok_key += keys[r]; tok_slot += slots[r]; tok_pos += list(range(L))
        brow += [chunk_row(t_rel0 + j, r, j == 0, rows) for j in range(L)]
    pair_of, tok_pair = {}, []
    for s, p in zip(tok_slot, tok_pos):
        tok_pair.append(pair_of.setdefault((s, p), len(pair_of)))
    i32 = lambda v: torch.tensor(v, dtype=torch.int32)
    u8 = lambda v: torch.tensor(v, dtype=torch.uint8)
    return dict(row_offset=i32(offs), row_uniform=u8([0] * row0 + [1 if u else 0 for u in uniform]), tok_key=u8(tok_key), tok_row=i32(tok_row),
                tok_slot=i32(tok_slot), tok_pos=i32(tok_pos), tok_pair=i32(tok_pair), rows=rows, m=m, row0=row0, tok0=tok0,
                offs=[o - tok0 for o in offs[row0:]], key=u8(tok_key[tok0:]), brow=torch.tensor(brow, dtype=torch.long), n_pairs=len(pair_of),
                lengths=list(lengths), uniform=uniform)


def to_buffer(x_plan, brow, n_rows=None):
    """rows in plan order -> buffer order (rows no position maps to stay zero)"""
    out = torch.zeros(n_rows or x_plan.shape[0], *x_plan.shape[1:], dtype=x_plan.dtype)
    out[brow] = x_plan
    return out


def from_buffer(x_buf, brow):
    return x_buf[brow]


def note_lo_share(key, got, ref, b32, dtype):
    """A 16-bit output sits within lo_bound = b32 + ulp / 2 (+ ulp), and the rounding alone takes err / bound to almost 1 whatever the
    fp32 arithmetic did.  What the record keeps for the constants is the share of the error the rounding cannot explain, over the fp32
    bound: max (err - ulp / 2) / b32, under the layout '<layout> beyond ulp/2'."""
    if key is None or dtype not in (torch.float16, torch.bfloat16):
        return
    err = (got.detach().cpu().to(F64) - ref).abs() - 0.5 * tc.ulp_lo(ref, dtype)
    share = torch.where(err > 0, err / b32.clamp_min(1e-300), torch.zeros_like(err))
    tc._note((key[0], key[1] + " beyond ulp/2"), float(share.max()) if share.numel() else 0.0, 0.0)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------
def ln_expect(x, gamma, beta, eps, lo=None):
    """-> dict(y, b_y, stats [rows, 2] = (mean, rstd), b_stats, b_lo): layernorm_ref / layernorm_bound on the values given, times
    C_FWD_LN; b_lo = lo_bound of the operand copy in `lo` (float32: b_y)"""
    ref = layernorm_ref(x, gamma, beta, eps)
    b = layernorm_bound(x, gamma, beta, eps, ref)
    out = dict(y=ref["y"], b_y=C_FWD_LN * b["y"], stats=torch.stack([ref["mean"], ref["rstd"]], 1),
               b_stats=C_FWD_LN * torch.stack([b["mean"], b["rstd"]], 1))
    out["b_lo"] = out["b_y"] if lo in (None, torch.float32) else lo_bound(out["y"], out["b_y"], lo)
    return out


def ln_emulate(x, gamma, beta, eps, lo=None):
    """the fp32 emulation of one launch -> dict(out_f32, out_lo, stats)"""
    r = layernorm_ref(x.to(F32), gamma, beta, eps, dt=F32)
    return dict(out_f32=r["y"], out_lo=r["y"] if lo in (None, torch.float32) else r["y"].to(lo), stats=torch.stack([r["mean"], r["rstd"]], 1))


def check_layernorm(what, exp, out_f32=None, out_lo=None, stats=None, key=None):
    """each output that is present against `exp` (ln_expect), rows in the order of exp"""
    if out_f32 is not None:
        check(out_f32, exp["y"], exp["b_y"], what + " out_f32", key=key)
    if out_lo is not None:
        check(out_lo, exp["y"], exp["b_lo"], what + " out_lo", key=key)
        note_lo_share(key, out_lo, exp["y"], exp["b_y"], out_lo.dtype)
    if stats is not None:
        check(stats, exp["stats"], exp["b_stats"], what + " stats", key=key)


def readout_expect(exp, bias_w, bias_b, dest=None):
    """the bias head on the LayerNorm output o = exp['y'] (within exp['b_y']): sum_c o w + bias_b, H products and the addend in any
    order — sum_bound(H + 1) over |o w| and |bias_b| — plus |w| . b_y for the error o arrives with; then the store: exact in fp32, lo_bound
    in a 16-bit destination.  bias_w None: exactly 0.  -> (ref [rows], bound [rows])"""
    rows, h = exp["y"].shape
    if bias_w is None:
        return torch.zeros(rows, dtype=F64), torch.zeros(rows, dtype=F64)
    w, b0 = bias_w.to(F64), float(bias_b.to(F64)[0])
    terms = exp["y"] * w
    ref = terms.sum(1) + b0
    bnd = sum_bound(h + 1, terms.abs().sum(1) + abs(b0)) + (w.abs() * exp["b_y"]).sum(1)
    if dest in (torch.float16, torch.bfloat16):
        bnd = lo_bound(ref, bnd, dest)
    return ref, bnd


def readout_emulate(ln, bias_w, bias_b, dest=None):
    """fp32 emulation of the bias head on ln_emulate's out_f32 -> [rows] in the destination type"""
    rows = ln["out_f32"].shape[0]
    v = torch.zeros(rows, dtype=F32) if bias_w is None else tc._sum(ln["out_f32"] * bias_w.to(F32), 1) + bias_b.to(F32)[0]
    return v.to(dest or torch.float32)


def _canary_mask(vec):
    bits = tc._bits(vec)
    return bits == (CANARY_BITS if vec.element_size() == 4 else torch.tensor(CANARY16, dtype=torch.int16).item())


def check_readout(what, ref, bnd, dest_vec, bias_rows, key=None):
    """dest_vec: the destination vector as the kernel left it (canary where it did not write).  Row r went to element bias_rows[r]
    (None: r; < 0: nowhere).  Every element no row maps to must still hold the canary (CanaryBroken names it); a reference that
    overflows an f16 destination must have become inf of its sign."""
    rows = ref.shape[0]
    dst = list(range(rows)) if bias_rows is None else [int(d) for d in bias_rows]
    written = torch.zeros(dest_vec.shape[0], dtype=torch.bool)
    written[[d for d in dst if d >= 0]] = True
    broken = torch.nonzero(~written & ~_canary_mask(dest_vec)).flatten().tolist()
    if broken:
        raise CanaryBroken(f"{what}: {len(broken)} destination element(s) no row maps to were written, first {broken[:4]}", [(0, i) for i in broken])
    rr = [r for r in range(rows) if dst[r] >= 0]
    if not rr:
        return
    got = dest_vec.detach().cpu()[[dst[r] for r in rr]].to(F64)
    y, b = ref[rr].clone(), bnd[rr]
    if dest_vec.dtype == torch.float16:
        over = y.to(torch.float16).isinf()
        if bool(over.any()):
            ok = got[over] == y[over].to(torch.float16).to(F64)
            if not bool(ok.all()):
                i = [rr[j] for j in torch.nonzero(over).flatten().tolist()][int(torch.nonzero(~ok)[0])]
                raise OpMismatch(f"{what}: row {i} overflows the f16 destination and was not stored as inf", torch.zeros(0, dtype=torch.bool), [i], [], i, 0)
            got, y = got.clone(), y.clone()
            got[over], y[over] = 0.0, 0.0
    try:
        check(got, y, b, what + " bias", key=key)
    except OpMismatch as e:          # (a vector is one row of the check: its column is the readout row)
        i = rr[e.col]
        raise OpMismatch(str(e) + f" [readout row {i} -> destination element {dst[i]}]", e.bad, [i], e.cols, i, 0) from None


# ---- the embeddings' LayerNorm -------------------------------------------------------------------------------------------------
def embed_sum_ref(e, dt=F64):
    """Stage one.  e: tok_slot / tok_pos of the launch's m positions, type0, pos_emb, lang (or None), lang_pos, and table (fp32) or
    table_lo with table_stats, table_gamma, table_beta.  sum = (x + type0) + pos_emb[pos], x = table[slot], or
    fma((table_lo[slot] - mean) rstd, gamma, beta), or lang - (type0 + pos_emb[lang_pos]).
    -> (sum [m, H] in plan order, bound): sum_bound over the terms as written — x, type0, pos: n = 3; the language token lang, type0,
    pos[L], type0, pos: n = 5; the 16-bit table n gamma, beta, type0, pos with n = (table_lo - mean) rstd: n = 4, plus 4 U |n gamma| for
    the two roundings n arrives with, 2 U each: the headroom over the unit round-off that sum_bound's n + 2 gives every term of a short
    sum (the multiply-add, fused or not, is one of the sum's)."""
    slot = e["tok_slot"].long()
    is_lang = (slot < 0)[:, None]
    s = slot.clamp_min(0)
    t0, p = e["type0"].to(dt), e["pos_emb"].to(dt)[e["tok_pos"].long()]
    if e.get("table_lo") is not None:
        st, g, b = e["table_stats"].to(dt)[s], e["table_gamma"].to(dt), e["table_beta"].to(dt)
        n = (e["table_lo"].to(dt)[s] - st[:, 0:1]) * st[:, 1:2]
        x = n * g + b
        bx = 4 * U * (n * g).to(F64).abs()
        mag, terms = (n * g).to(F64).abs() + b.to(F64).abs() + t0.to(F64).abs() + p.to(F64).abs(), 4
    else:
        x = e["table"].to(dt)[s]
        bx = torch.zeros(x.shape, dtype=F64)
        mag, terms = x.to(F64).abs() + t0.to(F64).abs() + p.to(F64).abs(), 3
    if e.get("lang") is not None:
        lang, pl = e["lang"].to(dt), e["pos_emb"].to(dt)[e["lang_pos"]]
        x = torch.where(is_lang, lang - (t0 + pl), x)
        bx = torch.where(is_lang, torch.zeros_like(bx), bx)
        mag_l = lang.to(F64).abs() + 2 * t0.to(F64).abs() + pl.to(F64).abs() + p.to(F64).abs()
        bnd = torch.where(is_lang, sum_bound(5, mag_l), sum_bound(terms, mag)) + bx
    else:
        assert not bool(is_lang.any()), "a language token without the language embedding"
        bnd = sum_bound(terms, mag) + bx
    return (x + t0) + p, bnd


def check_embed(what, e, plan_brow, eps, gamma, beta, sum_buf, out_lo_buf, stats_buf, lo, key=None):
    """The two stages.  sum_buf / out_lo_buf / stats_buf: the kernel's outputs in BUFFER order (each may be None); plan_brow: buffer row
    of every position (identity for pair rows written in place)."""
    if sum_buf is not None:
        ref, bnd = embed_sum_ref(e)
        check(from_buffer(sum_buf.detach().cpu(), plan_brow), ref, bnd, what + " sum (stage one)", key=None if key is None else (key[0] + "_sum", key[1]))
        exp = ln_expect(sum_buf.detach().cpu(), gamma, beta, eps, lo)          # stage two: on the bits the kernel normalised
        check_layernorm(what + " (stage two)", exp, out_lo=out_lo_buf, stats=stats_buf, key=key)


# ---- attention ---------------------------------------------------------------------------------------------------------------
def attention_expect(plan, q, k, v, heads, d, cls_only, fast, lo=None):
    """q (plan order [m, H], or [rows, H] with cls_only), k, v (plan order) -> dict(ctx, bound, bound32: the bound of the fp32 value in
    front of a 16-bit store, fast_rows: per vocabulary row whether the fast path takes it).  attention_ref's bound (two passes, base e, expf) is extended for what the forward's kernels do instead:

      generic loop (online softmax over the L visible keys): the running maximum changes at most L times, each change multiplies
        the sums by corr = expf(old - new); the product of the corrs telescopes to exp(first - max), so their argument errors add up
        to U (max - min score) and two more score bounds 2 B, their own roundings to 2 U each: 2 L U; every step rounds l and acc once
        each and p v once: 3 L U.                                      e_j = 5 L U + U (max - min) + 2 B
      fast path (rows of at most ATT_FAST_KEYS positions, 16-bit operands): the score is dot * sc2, sc2 = fl(scaling * log2 e) — the
        constant's own error (2 U relative) scales s_j - max, and the two products round separately: U (|s_j| + |max|) in units of the
        exponent; exp2 is one more rounding than expf's argument reduction hides: 2 U.  The f16 dot product (v_dot2_f32_f16) adds
        products that are exact in fp32, two at a time, to an fp32 accumulator: inside the (d + 3) U |q| . |k| of the score bound.
                                                                       e_j = U (|s_j| + |max|) + 2 U |s_j - max| + 2 U
    Both enter like eps_j of attention_ref: ctx moves by sum_j p_j |v_j| (e_j + max_j e_j).  The whole is times C_FWD_ATT (generic) or
    C_FWD_ATT_FAST, then lo_bound for a 16-bit ctx."""
    offs, mask = plan["offs"], plan["key"]
    r = attention_ref(q, k, v, mask, offs, heads, d, cls_only)
    sc = tc.att_scaling(d)
    q64, k64, v64 = q.to(F64), k.to(F64), v.to(F64)
    bound = torch.zeros_like(r["b_ctx"])
    fast_rows = []
    for n in range(len(offs) - 1):
        t0, t1 = offs[n], offs[n + 1]
        L = t1 - t0
        is_fast = bool(fast) and lo in (torch.float16, torch.bfloat16) and L <= ATT_FAST_KEYS
        fast_rows.append(is_fast)
        rows = slice(n, n + 1) if cls_only else slice(t0, t1)
        qi, kk, vv = tc._heads(q64[rows], heads, d), tc._heads(k64[t0:t1], heads, d), tc._heads(v64[t0:t1], heads, d)
        m = mask[t0:t1].bool()
        uni = not bool(m.any())
        prod = qi[:, :, None, :] * kk[:, None, :, :]
        s = torch.zeros(prod.shape[:3], dtype=F64) if uni else prod.sum(3) * sc
        vis = torch.ones_like(s, dtype=torch.bool) if uni else m[None, None, :].expand_as(s)
        B = torch.zeros_like(s[..., :1]) if uni else torch.where(vis, (d + 3) * U * sc * prod.abs().sum(3), torch.zeros_like(s)).max(dim=2, keepdim=True).values
        mx = torch.where(vis, s, torch.full_like(s, -float("inf"))).max(dim=2, keepdim=True).values
        mn = torch.where(vis, s, torch.full_like(s, float("inf"))).min(dim=2, keepdim=True).values
        if is_fast:
            e = U * (s.abs() + mx.abs()) + 2 * U * (s - mx).abs() + 2 * U
        else:
            e = (5 * L * U + U * (mx - mn) + 2 * B).expand_as(s)
        e = torch.where(vis, e, torch.zeros_like(e))
        extra = ((r["probs"][n] * (e + e.max(dim=2, keepdim=True).values))[..., None] * vv.abs()[:, None, :, :]).sum(2)
        c = C_FWD_ATT_FAST if is_fast else C_FWD_ATT
        bound[rows] = c * (r["b_ctx"][rows] + extra.transpose(0, 1).reshape(-1, heads * d))
    bound32 = bound
    if lo in (torch.float16, torch.bfloat16):
        bound = lo_bound(r["ctx"], bound, lo)
    return dict(ctx=r["ctx"], bound=bound, bound32=bound32, fast_rows=fast_rows)


def attention_emulate(plan, q, k, v, heads, d, cls_only, lo=None):
    c = attention_ref(q.to(F32), k.to(F32), v.to(F32), plan["key"], plan["offs"], heads, d, cls_only, dt=F32)["ctx"]
    return c if lo in (None, torch.float32) else c.to(lo)


def check_attention(what, plan, exp, ctx_plan, cls_only, key=None):
    """ctx_plan: the kernel's ctx brought to plan order ([rows, H] with cls_only).  Fast and generic rows are checked (and recorded)
    separately, each against its own constant."""
    offs = plan["offs"]
    for path in (True, False):
        idx = []
        for n, f in enumerate(exp["fast_rows"]):
            if f == path:
                idx += [n] if cls_only else list(range(offs[n], offs[n + 1]))
        if not idx:
            continue
        k2 = None if key is None else ("fwd_attention_fast" if path else "fwd_attention_generic", key)
        try:
            check(ctx_plan.detach().cpu()[idx], exp["ctx"][idx], exp["bound"][idx], f"{what} ctx ({'fast' if path else 'generic'} rows)", key=k2)
            note_lo_share(k2, ctx_plan.detach().cpu()[idx], exp["ctx"][idx], exp["bound32"][idx], ctx_plan.dtype)
        except OpMismatch as e:          # name the row of the whole ctx, not of the subset
            bad = torch.zeros(exp["ctx"].shape, dtype=torch.bool)
            bad[idx] = e.bad
            raise OpMismatch(str(e) + f" [ctx row {idx[e.row]} in plan order]", bad, [idx[i] for i in e.rows], e.cols, idx[e.row], e.col) from None


# ---- ln_stats ----------------------------------------------------------------------------------------------------------------
def ln_stats_ref(parts, h, eps, dt=F64):
    """parts [P, rows, 2] = (sum, sum of squares) per 128 columns -> stats [rows, 2] = (mean, rstd), var = max(q / h - mean^2, 0)"""
    p = parts.to(dt)
    mean = tc._sum(p[..., 0], 0) / h
    var = (tc._sum(p[..., 1], 0) / h - mean * mean).clamp_min(0.0)
    return torch.stack([mean, 1.0 / torch.sqrt(var + tc.f32_value(eps))], 1)


def ln_stats_bound(parts, h, eps, ref):
    """mean: a sum of P partials and the division: bm = sum_bound(P, sum |s_p|) / h.
    var = max(q / h - mean^2, 0): q / h within bq = sum_bound(P, sum q_p) / h; mean^2 moves by 2 |mean| bm + bm^2 and rounds once; the
    subtraction rounds once on operands that may each be far larger than their difference — THE CANCELLATION: the bound is absolute, in
    units of q / h and mean^2, not of var:   bv = bq + 2 |mean| bm + bm^2 + 2 U (q / h + mean^2);  the clamp is 1-Lipschitz.
    rstd = (var + eps)^-1/2 is not linearised (bv may exceed var + eps): the larger of the distances to the values at var - bv (not
    below 0) and var + bv, plus three roundings (the sum, the square root, the reciprocal).  Times C_LN_STATS."""
    p = parts.to(F64)
    P = p.shape[0]
    mean, rstd = ref[:, 0].to(F64), ref[:, 1].to(F64)
    qh = p[..., 1].sum(0) / h
    bm = sum_bound(P, p[..., 0].abs().sum(0)) / h
    bq = sum_bound(P, p[..., 1].abs().sum(0)) / h
    bv = bq + 2 * mean.abs() * bm + bm * bm + 2 * U * (qh.abs() + mean * mean)
    var = (qh - mean * mean).clamp_min(0.0)
    e = tc.f32_value(eps)
    hi, lo = 1.0 / torch.sqrt((var - bv).clamp_min(0.0) + e), 1.0 / torch.sqrt(var + bv + e)
    br = torch.maximum(hi - rstd, rstd - lo) + 3 * U * hi
    return C_LN_STATS * torch.stack([bm, br], 1)


def clamp_rstd(eps):
    """1 / sqrt(0 + eps) as the kernel computes it: fp32 addition, square root and division, each correctly rounded"""
    e = torch.tensor(eps, dtype=F32)
    return (torch.tensor(1.0, dtype=F32) / torch.sqrt(torch.tensor(0.0, dtype=F32) + e)).reshape(1)


def check_ln_stats(what, parts, h, eps, stats, clamp_rows=(), key=None):
    ref = ln_stats_ref(parts, h, eps)
    check(stats, ref, ln_stats_bound(parts, h, eps, ref), what + " stats", key=key)
    for r in clamp_rows:
        exact(stats.detach().cpu()[r, 1].reshape(1), clamp_rstd(eps), f"{what} rstd of row {r} (variance clamped to 0)")


# ---- fold_weight ---------------------------------------------------------------------------------------------------------------
def fold_ref(w, gamma, beta, bias, lo, dt=F64):
    """-> dict(w_fold (exact: one fp32 multiply, then the conversion), c, b_c = sum_bound(K) over the rounded values, b, b_b = sum_bound
    (K + 1) over |w beta| and |bias|)"""
    k = w.shape[1]
    wf = (w.to(F32) * gamma.to(F32)).to(lo)
    terms = w.to(dt) * beta.to(dt)
    return dict(w_fold=wf, c=tc._sum(wf.to(dt), 1), b_c=sum_bound(k, wf.to(F64).abs().sum(1)), b=bias.to(dt) + tc._sum(terms, 1),
                b_b=sum_bound(k + 1, terms.to(F64).abs().sum(1) + bias.to(F64).abs()))


def check_fold(what, ref, w_fold, c_out, b_out, rows=None, key=None):
    """rows: the rows whose sums are checked (a row with an out-of-range product has an infinite column sum: only its bits are)"""
    exact(w_fold.detach().cpu(), ref["w_fold"], what + " w_fold", key=key)
    rr = list(range(ref["c"].shape[0])) if rows is None else list(rows)
    check(c_out.detach().cpu()[rr], ref["c"][rr], ref["b_c"][rr], what + " c", key=key)
    check(b_out.detach().cpu()[rr], ref["b"][rr], ref["b_b"][rr], what + " b'", key=key)


# ---- gather_src ----------------------------------------------------------------------------------------------------------------
def gather_expect(ids, src, v0, fallback, sw, sb, out_dtype):
    """train_ops_check.gather_fwd_ref on the ids of the launch: copies (and their conversion) exact, rescaled rows fma_bound, then lo_bound
    in a 16-bit output.  -> dict(value float64, bound (0 = equality of the converted value), out_of_range: a value beyond the f16 limit or NaN)"""
    val, bnd = tc.gather_fwd_ref(ids, src, v0, fallback, sw, sb)
    oor = ~(val.abs() <= F16_MAX)
    return dict(value=val, bound=bnd, out_of_range=oor, dtype=out_dtype)


def gather_emulate(ids, src, v0, fallback, sw, sb, out_dtype):
    ids = ids.long()
    s = src.to(F32)[ids.clamp(max=v0 - 1)]
    if sw is not None:
        s = sw.to(F32) * s + sb.to(F32)
    return torch.where((ids >= v0)[:, None], fallback.to(F32)[(ids - v0).clamp(min=0)], s).to(out_dtype)


def check_gather(what, exp, out, range_word, prec, key=None):
    got, val, bnd = out.detach().cpu(), exp["value"], exp["bound"]
    want_word = RANGE_SOURCE if (prec == "f16" and bool(exp["out_of_range"].any())) else 0
    assert int(range_word) == want_word, f"{what}: range word {int(range_word)}, expected {want_word}"
    if not bool((bnd > 0).any()):
        exact(got, val.to(F32).to(exp["dtype"]), what + " out (copy / conversion)", key=key)
        return
    fin = torch.isfinite(val.to(F32).to(exp["dtype"]).to(F64))
    if not bool(fin.all()):          # beyond the output type: the bits of the conversion, then out of the bounded check
        exact(torch.where(fin, torch.zeros_like(got), got), torch.where(fin, torch.zeros_like(got), val.to(F32).to(exp["dtype"])), what + " out (overflow)")
        got, val = torch.where(fin, got, torch.zeros_like(got)), torch.where(fin, val, torch.zeros_like(val))
    b = bnd if exp["dtype"] == torch.float32 else lo_bound(val, bnd, exp["dtype"])
    check(got, val, b, what + " out", key=key)
