"""tests/rowops_check.py checked without a GPU: the fp32 emulation of every reference stays below a quarter of its bound on the case
shapes of tests/test_rowops_direct_gpu.py (a value rounded to 16 bits spends up to half an ulp of its lo_bound on that rounding
alone: it is held to the bound itself, and the fp32 value in front of the rounding to the quarter); the check FAILS on subtly wrong results (each defect below is applied to a correct
emulated result and must raise OpMismatch or CanaryBroken naming the right row and column); the plan helpers agree with a brute-force
construction; and every zett_op_fwd_* entry point refuses bad arguments before anything is launched.
"""
import ctypes as C

import pytest
import torch

from tests import rowops_check as rc
from tests import test_rowops_direct_gpu as cases
from tests import train_ops_check as tc

F32, F64 = torch.float32, torch.float64
QUARTER = 0.25


def _ratio(got, ref, bnd, what):
    top, _ = tc.check(got, ref, bnd, what)
    assert top <= QUARTER, (what, top)
    return top


# ---- emulation -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", cases.LN_H)
def test_layernorm_emulation_stays_below_a_quarter_of_the_bound(h):
    for case in cases.ln_cases(h):
        if case["prec"] == "f16" and h > 2048:
            continue          # (the same arithmetic as bf16; the wide rows are the slow ones)
        x, gamma, beta = cases.ln_inputs(case)
        lo = rc.DT[case["prec"]]
        exp, emu = rc.ln_expect(x, gamma, beta, cases.EPS_ENC, lo), rc.ln_emulate(x, gamma, beta, cases.EPS_ENC, lo)
        _ratio(emu["out_f32"], exp["y"], exp["b_y"], f"{case} y")
        tc.check(emu["out_lo"], exp["y"], exp["b_lo"], f"{case} y_lo")
        _ratio(emu["stats"], exp["stats"], exp["b_stats"], f"{case} stats")
        g = torch.Generator().manual_seed(1)
        bias_w, bias_b = torch.randn(h, generator=g) / h ** 0.5, torch.tensor([0.25])
        for dest in (None, torch.float16, torch.bfloat16):
            ref, bnd = rc.readout_expect(exp, bias_w, bias_b, dest)
            (_ratio if dest is None else tc.check)(rc.readout_emulate(emu, bias_w, bias_b, dest), ref, bnd, f"{case} bias {dest}")


@pytest.mark.parametrize("h", cases.EMBED_H)
def test_embed_sum_emulation_stays_below_a_quarter_of_the_bound(h):
    for variant, prec in ((0, "f32"), (1, "bf16"), (1, "f16"), (2, "bf16")):
        _, e, _, _ = cases.embed_case(h, prec, variant, 77 + variant)
        ref, bnd = rc.embed_sum_ref(e)
        _ratio(rc.embed_sum_ref(e, dt=F32)[0], ref, bnd, f"embed sum h={h} variant {variant} {prec}")


@pytest.mark.parametrize("h,hd", cases.ATT_SHAPES)
def test_attention_emulation_stays_below_a_quarter_of_the_bound(h, hd):
    for s, rs in enumerate(cases.ATT_ROWSETS):
        prec = cases.PRECS[(s + h // 64) % 3]
        cls_only = (s + hd // 8) % 2
        plan = cases.att_plan(rs, 0, 0)
        _, _, qp, kp, vp = cases.att_values(plan, rs, h, rc.DT[prec], False, cls_only, 5 + s)
        for fast in (True, False):
            exp = rc.attention_expect(plan, qp, kp, vp, h // hd, hd, bool(cls_only), fast, rc.DT[prec])
            _ratio(rc.attention_emulate(plan, qp, kp, vp, h // hd, hd, bool(cls_only)), exp["ctx"], exp["bound32"], f"attention {h} {hd} {prec} set {s}")
            tc.check(rc.attention_emulate(plan, qp, kp, vp, h // hd, hd, bool(cls_only), rc.DT[prec]), exp["ctx"], exp["bound"], f"attention {h} {hd} {prec} set {s} (16-bit)")


def test_small_kernels_emulation_stays_below_a_quarter_of_the_bound():
    for parts in cases.STATS_PARTS:
        for rows in cases.STATS_ROWS:
            p = cases.stats_parts(parts, rows, parts + rows)
            ref = rc.ln_stats_ref(p, 128 * parts, cases.EPS_ENC)
            emu = rc.ln_stats_ref(p, 128 * parts, cases.EPS_ENC, dt=F32)
            _ratio(emu, ref, rc.ln_stats_bound(p, 128 * parts, cases.EPS_ENC, ref), f"ln_stats {parts} {rows}")
            tc.exact(emu[0, 1].reshape(1), rc.clamp_rstd(cases.EPS_ENC), "the clamp row")
    g = torch.Generator().manual_seed(2)
    for k in cases.FOLD_K:
        w, gamma, beta, bias = torch.randn(3, k, generator=g), torch.randn(k, generator=g), torch.randn(k, generator=g), torch.randn(3, generator=g)
        for lo in (torch.bfloat16, torch.float16):
            ref, emu = rc.fold_ref(w, gamma, beta, bias, lo), rc.fold_ref(w, gamma, beta, bias, lo, dt=F32)
            _ratio(emu["c"], ref["c"], ref["b_c"], f"fold c {k}")
            _ratio(emu["b"], ref["b"], ref["b_b"], f"fold b {k}")
    ids = torch.tensor(cases.GATHER_IDS, dtype=torch.int32)
    for e_in in cases.GATHER_E:
        src, fb = torch.randn(cases.GATHER_V0, e_in, generator=g), torch.randn(cases.GATHER_FB, e_in, generator=g)
        sw, sb = 1.0 + 0.1 * torch.randn(e_in, generator=g), 0.1 * torch.randn(e_in, generator=g)
        for prec in cases.PRECS:
            exp = rc.gather_expect(ids, src, cases.GATHER_V0, fb, sw, sb, rc.DT[prec])
            rc.check_gather(f"gather {e_in} {prec}", exp, rc.gather_emulate(ids, src, cases.GATHER_V0, fb, sw, sb, rc.DT[prec]), 0, prec)
            exp = rc.gather_expect(ids, src, cases.GATHER_V0, fb, None, None, rc.DT[prec])
            rc.check_gather(f"gather copy {e_in} {prec}", exp, rc.gather_emulate(ids, src, cases.GATHER_V0, fb, None, None, rc.DT[prec]), 0, prec)


# ---- sensitivity -------------------------------------------------------------------------------------------------------------
def _ln_fixture(h=320, rows=9, lo=torch.bfloat16):
    x, gamma, beta = cases.ln_inputs(dict(h=h, rows=rows, kind=0, seed=3))
    gamma = gamma + 2.0          # (no zero gamma: every column is sensitive)
    return x, gamma, beta, rc.ln_expect(x, gamma, beta, 1e-5, lo), rc.ln_emulate(x, gamma, beta, 1e-5, lo)


def test_layernorm_defects_are_caught():
    x, gamma, beta, exp, emu = _ln_fixture()
    rc.check_layernorm("correct", exp, **emu)
    # one element moved by twice its bound
    bad = emu["out_f32"].to(F64).clone()
    bad[4, 17] = exp["y"][4, 17] + 2 * exp["b_y"][4, 17]
    with pytest.raises(rc.OpMismatch) as ei:
        rc.check_layernorm("moved", exp, out_f32=bad)
    assert (ei.value.row, ei.value.col) == (4, 17) and int(ei.value.bad.sum()) == 1
    # a mean taken over H - 8 columns (row 2)
    h = x.shape[1]
    m8 = x[2, :h - 8].mean()
    d = x[2] - m8
    y = d / torch.sqrt((d * d).mean() + 1e-5) * gamma + beta
    bad = emu["out_f32"].clone()
    bad[2] = y
    with pytest.raises(rc.OpMismatch) as ei:
        rc.check_layernorm("short mean", exp, out_f32=bad)
    assert ei.value.row == 2 and not bool(ei.value.bad[[0, 1, 3, 4, 5, 6, 7, 8]].any())
    bad_st = emu["stats"].clone()
    bad_st[2, 0] = m8
    with pytest.raises(rc.OpMismatch) as ei:
        rc.check_layernorm("short mean", exp, stats=bad_st)
    assert (ei.value.row, ei.value.col) == (2, 0)
    # one lane group's 8 columns taken from the neighbouring row
    bad = emu["out_lo"].clone()
    bad[5, 64:72] = emu["out_lo"][6, 64:72]
    with pytest.raises(rc.OpMismatch) as ei:
        rc.check_layernorm("neighbour", exp, out_lo=bad)
    assert ei.value.row == 5 and 64 <= ei.value.col < 72 and not bool(ei.value.bad[:, :64].any()) and not bool(ei.value.bad[:, 72:].any())
    # a 16-bit value truncated instead of rounded to nearest even: the element that loses most by it
    y32 = emu["out_f32"]
    trunc = (y32.view(torch.int32) & -65536).view(F32)
    loss = ((y32 - trunc).abs().to(F64) / tc.ulp_lo(exp["y"], torch.bfloat16))
    loss[exp["b_y"] > 0.01 * tc.ulp_lo(exp["y"], torch.bfloat16)] = 0
    r, c = divmod(int(loss.argmax()), h)
    assert float(loss[r, c]) > 0.9
    bad = emu["out_lo"].clone()
    bad[r, c] = trunc[r, c].to(torch.bfloat16)
    with pytest.raises(rc.OpMismatch) as ei:
        rc.check_layernorm("truncated", exp, out_lo=bad)
    assert (ei.value.row, ei.value.col) == (r, c)


def test_stores_outside_the_output_are_caught():
    x, gamma, beta, exp, emu = _ln_fixture()
    rows, h = x.shape
    # a store one row past `rows`
    f = tc.Frame(rows, h, h, torch.bfloat16, "canary")
    buf = f.buf.clone()
    f.view(buf).copy_(emu["out_lo"])
    tc.check_canary(f, buf, "intact")
    buf[f.offset + rows * h + 3] = 1.0
    with pytest.raises(rc.CanaryBroken) as ei:
        tc.check_canary(f, buf, "one row past")
    assert ei.value.where == [(rows, 3)]
    # a skipped bias_rows row written
    g = torch.Generator().manual_seed(4)
    bias_w, bias_b = torch.randn(h, generator=g) / h ** 0.5, torch.tensor([0.25])
    ref, bnd = rc.readout_expect(exp, bias_w, bias_b, torch.float16)
    val = rc.readout_emulate(emu, bias_w, bias_b, torch.float16)
    rows_map = torch.tensor([3, -1, 0, 11, -1, 5, 6, 2, 9], dtype=torch.int64)
    dest = tc.Frame(None, 12, 12, torch.float16, "canary")
    vec = dest.view(dest.buf).clone()
    for r, d in enumerate(rows_map.tolist()):
        if d >= 0:
            vec[d] = val[r]
    rc.check_readout("correct", ref, bnd, vec, rows_map)
    bad = vec.clone()
    bad[4] = val[1]          # (row 1 is skipped; had the map been ignored it would have gone somewhere)
    with pytest.raises(rc.CanaryBroken) as ei:
        rc.check_readout("skipped row written", ref, bnd, bad, rows_map)
    assert ei.value.where == [(0, 4)]
    bad = vec.clone()
    bad[3], bad[0] = vec[0], vec[3]          # rows 0 and 2 exchanged in the destination
    with pytest.raises(rc.OpMismatch) as ei:
        rc.check_readout("exchanged", ref, bnd, bad, rows_map)
    assert ei.value.row in (0, 2)


def _att_fixture(cls_only=False):
    rs = cases.ATT_ROWSETS[0]
    plan = cases.att_plan(rs, 2, 6)
    h, hd, lo = 128, 32, torch.bfloat16
    _, _, qp, kp, vp = cases.att_values(plan, dict(lengths=rs["lengths"]), h, lo, False, cls_only, 9)
    exp = rc.attention_expect(plan, qp, kp, vp, h // hd, hd, cls_only, True, lo)
    return plan, (qp, kp, vp), h, hd, lo, exp


def test_attention_defects_are_caught():
    plan, (qp, kp, vp), h, hd, lo, exp = _att_fixture()
    good = rc.attention_emulate(plan, qp, kp, vp, h // hd, hd, False, lo)
    rc.check_attention("correct", plan, exp, good, False)
    offs = plan["offs"]

    def with_keys(row, pos, value):
        p2 = dict(plan)
        key = plan["key"].clone()
        key[offs[row] + pos] = value
        p2["key"] = key
        return rc.attention_emulate(p2, qp, kp, vp, h // hd, hd, False, lo)

    # one visible key left out of one row's softmax (row 6, its key 3), and a masked key let in (row 4, whose position 0 is no key)
    for row, pos, value in ((6, 3, 0), (4, 0, 1), (8, 0, 1)):
        with pytest.raises(rc.OpMismatch) as ei:
            rc.check_attention("key", plan, exp, with_keys(row, pos, value), False)
        assert offs[row] <= ei.value.row < offs[row + 1], (row, ei.value.row)
        touched = ei.value.bad.any(1).nonzero().flatten().tolist()
        assert all(offs[row] <= t < offs[row + 1] for t in touched)
    # two buffer rows exchanged
    buf = rc.to_buffer(good, plan["brow"])
    a, b = 3, plan["rows"] + 5
    bad = buf.clone()
    bad[a], bad[b] = buf[b], buf[a]
    with pytest.raises(rc.OpMismatch) as ei:
        rc.check_attention("exchanged", plan, exp, rc.from_buffer(bad, plan["brow"]), False)
    moved = {int((plan["brow"] == a).nonzero()), int((plan["brow"] == b).nonzero())}
    assert ei.value.row in moved and set(ei.value.bad.any(1).nonzero().flatten().tolist()) == moved
    # position 0 written in plan order instead of first: the buffer IS the plan order
    with pytest.raises(rc.OpMismatch) as ei:
        rc.check_attention("plan order", plan, exp, rc.from_buffer(good, plan["brow"]), False)
    assert bool(ei.value.bad.any())


# ---- plan helpers ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row0,tok0", ((0, 0), (2, 6), (3, 3)))
def test_plan_helpers_match_a_brute_force_construction(row0, tok0):
    for rs in cases.ATT_ROWSETS:
        plan = cases.att_plan(rs, row0, tok0)
        lengths, rows, m = list(rs["lengths"]), len(rs["lengths"]), sum(rs["lengths"])
        assert plan["rows"] == rows and plan["m"] == m and int(plan["row_offset"][row0]) == tok0 and int(plan["row_offset"][-1]) == tok0 + m
        # brute force: position 0 of every row first, in row order; every other position behind them, in plan order
        firsts, others, t = [], [], 0
        for L in lengths:
            firsts.append(t)
            others += list(range(t + 1, t + L))
            t += L
        order = firsts + others          # buffer row -> chunk position
        assert sorted(order) == list(range(m))
        brow = [0] * m
        for b, pos in enumerate(order):
            brow[pos] = b
        assert plan["brow"].tolist() == brow
        for r, L in enumerate(lengths):
            n = row0 + r
            t0, t1 = int(plan["row_offset"][n]), int(plan["row_offset"][n + 1])
            assert t1 - t0 == L and plan["tok_row"][t0:t1].tolist() == [n] * L and plan["tok_pos"][t0:t1].tolist() == list(range(L))
            keys = plan["tok_key"][t0:t1].tolist()
            assert bool(plan["row_uniform"][n]) == (sum(keys) == 0) == (r in rs["uniform"])
            if r in rs["pad0"] and L > 1:
                assert keys[0] == 0 and all(keys[1:])
        # pair slots: equal exactly where (slot, position) are equal, dense from 0
        sp = list(zip(plan["tok_slot"].tolist(), plan["tok_pos"].tolist()))
        pair = plan["tok_pair"].tolist()
        assert sorted(set(pair)) == list(range(plan["n_pairs"])) and len(set(sp)) == plan["n_pairs"]
        assert all((sp[i] == sp[j]) == (pair[i] == pair[j]) for i in range(len(sp)) for j in range(i))
        rows_of = {}
        for t in range(tok0, tok0 + m):
            rows_of.setdefault(pair[t], set()).add(int(plan["tok_row"][t]))
        assert any(len(v) > 1 for v in rows_of.values()) or m < 6, "no pair is shared between rows"
        x = torch.arange(m * 2, dtype=F32).reshape(m, 2)
        assert torch.equal(rc.from_buffer(rc.to_buffer(x, plan["brow"]), plan["brow"]), x)
        assert torch.equal(rc.to_buffer(x, plan["brow"])[:rows], x[firsts])


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_forward_row_entry_points_refuse_bad_arguments_before_touching_the_device():
    """zett_op_fwd_*: arguments are validated before any launch, the return code is ZETT_E_INVALID and zett_last_error says why
    (no GPU needed: nothing is launched)"""
    from zett_amd import _lib
    lib = _lib.load()
    P = C.c_void_p
    buf = (C.c_float * 4096)()
    base = C.addressof(buf)
    a = P((base + 63) & ~63)
    odd = P(a.value + 4)
    null = P(0)
    kid = C.c_int32(0)
    BF, F3, H16 = _lib.PREC_BF16, _lib.PREC_F32, _lib.PREC_F16

    def refused(rc_, *words):
        assert rc_ == _lib.E_INVALID, rc_
        msg = lib.zett_last_error().decode()
        assert all(w in msg for w in words), msg

    ln = lambda prec=BF, inp=a, in_lo=null, ld=64, rows=2, h=64, gamma=a, out=a, bias_w=null, out_bias=null, rows_map=null, dt=-1: lib.zett_op_fwd_layernorm(
        prec, inp, in_lo, ld, rows, h, gamma, a, 1e-5, 1, out, null, null, bias_w, a if bias_w.value else null, out_bias, rows_map, dt, null, C.byref(kid), null)
    refused(ln(h=60, ld=60), "multiple of 8")
    refused(ln(prec=9), "precision")
    refused(ln(inp=null), "null")
    refused(ln(gamma=null), "null")
    refused(ln(inp=odd), "aligned")
    refused(ln(ld=56), "ld_in")
    refused(ln(ld=68), "ld_in")
    refused(ln(prec=F3, inp=null, in_lo=a, out_bias=a), "16-bit")
    refused(ln(in_lo=a), "readout")
    refused(ln(out_bias=a, dt=7), "dtype")
    refused(ln(bias_w=a), "out_bias")
    refused(ln(out_bias=a, rows_map=a), "bias_rows")
    emb = lambda prec=BF, table=a, table_lo=null, tstats=null, slot=a, h=64, trow=null, roff=null, m=2: lib.zett_op_fwd_embed_layernorm(
        prec, table, table_lo, tstats, a if table_lo.value else null, a if table_lo.value else null, slot, a, a, a, null, 0, trow, roff, 0, 1, 0, m, h, a, a, 1e-5, 1,
        a, null, null, C.byref(kid), null)
    refused(emb(h=12), "multiple of 8")
    refused(emb(table=null), "null")
    refused(emb(slot=null), "null")
    refused(emb(prec=F3, table_lo=a, tstats=a), "16-bit")
    refused(emb(table_lo=a), "table_stats")
    refused(emb(trow=a), "row_offset")
    refused(emb(table=odd), "aligned")
    refused(emb(prec=5), "precision")
    att = lambda prec=H16, q=a, ldq=64, ldkv=64, h=64, hd=16, flags=0, roff=a: lib.zett_op_fwd_attention(prec, q, ldq, a, a, ldkv, h, hd, roff, a, a, 0, 1, 0, 0.25, flags,
                                                                                                  null, a, null)
    refused(att(hd=24), "power of two")
    refused(att(hd=4), "power of two")
    refused(att(h=1024, ldq=1024, ldkv=1024, hd=1024), "[8, 512]")
    refused(att(h=96, ldq=96, ldkv=96, hd=64), "divides")
    refused(att(h=60, ldq=64), "multiple of 8")
    refused(att(q=odd), "aligned")
    refused(att(ldq=56), "ldq")
    refused(att(ldkv=68), "ldkv")
    refused(att(roff=null), "null")
    refused(att(flags=8), "flags")
    refused(att(prec=3), "precision")
    gat = lambda prec=BF, src=a, sdt=0, e=64, sw=null, sb=null: lib.zett_op_fwd_gather_src(prec, a, 0, 2, src, sdt, e, 4, a, sw, sb, a, null, null)
    refused(gat(sdt=5), "dtype")
    refused(gat(src=null), "null")
    refused(gat(e=12), "multiple of 8")
    refused(gat(sw=a), "rescaler")
    refused(gat(src=odd), "aligned")
    refused(gat(prec=-1), "precision")
    refused(lib.zett_op_fwd_ln_stats(BF, a, 4, 2, 200, 1e-5, a, null), "128")
    refused(lib.zett_op_fwd_ln_stats(BF, null, 4, 2, 256, 1e-5, a, null), "null")
    refused(lib.zett_op_fwd_ln_stats(BF, a, 1, 2, 256, 1e-5, a, null), "ld_part")
    refused(lib.zett_op_fwd_ln_stats(BF, odd, 4, 2, 256, 1e-5, a, null), "aligned")
    refused(lib.zett_op_fwd_ln_stats(4, a, 4, 2, 256, 1e-5, a, null), "precision")
    fold = lambda prec=BF, w=a, k=64, bias=a: lib.zett_op_fwd_fold_weight(prec, w, 2, k, a, a, bias, a, a, a, null, null)
    refused(fold(prec=F3), "16-bit")
    refused(fold(bias=null), "null")
    refused(fold(k=20), "multiple of 8")
    refused(fold(w=odd), "aligned")
    refused(fold(prec=11), "precision")
    # and nothing to do is not an error
    assert ln(rows=0) == 0 and emb(m=0) == 0 and lib.zett_op_fwd_ln_stats(BF, a, 4, 0, 256, 1e-5, a, null) == 0
