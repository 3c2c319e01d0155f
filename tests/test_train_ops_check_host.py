"""The checker of the training row primitives (tests/train_ops_check.py) passes a right kernel, fails a subtly wrong one AT ITS
ELEMENT, and the case tables of tests/test_train_ops_direct_gpu.py reach every branch they claim to (no GPU).

A right kernel is the fp32 emulation: the reference formulas run in fp32 with every sum taken strictly left to right (data
movement, conversions and single operations: the torch operation itself).  Into that result three mistakes are planted, one at a
time:
  * one element off.  Where the bound is equality or the rounding of a 16-bit type, by 4 ulp of the output's type.  An fp32 result
    of a reduction has a bound that is legitimately wider than 4 ulp of the RESULT (it follows sum |terms|, which cancellation
    makes much larger than the sum): there the element is moved by 4 times its bound, as tests/test_gemm_check_host.py does;
  * one row replaced by the row after it;
  * where the op has one, the zero-pad band filled with the last real row (column, for the transposed outputs).
"""
import pytest
import torch

from tests import test_train_ops_direct_gpu as cases
from tests import train_ops_check as tc

F32, F64 = torch.float32, torch.float64


def _g(seed):
    return torch.Generator().manual_seed(seed)


# ---- specimens: name -> dict(got, ref, bnd (None: bit equality), slice_rel, ulp (plant 4 ulp of the type), pad (first index of the zero band along dim 1)) ----
def _specimens():
    s = {}
    g = _g(1)
    x = torch.rand(65, 5, generator=g) * 2 - 1
    z = (torch.randn(65, 5, generator=g) * 2.5).clamp(-7.99, 7.99)
    for kind, lo in tc.LO.items():
        s[f"transpose_lo {kind}"] = dict(got=tc.transpose_ref(x, 128, lo), ref=tc.transpose_ref(x, 128, lo), bnd=None, pad=65)
        s[f"transpose_lo16 {kind}"] = dict(got=tc.transpose_ref(x.to(lo), 68, lo), ref=tc.transpose_ref(x.to(lo), 68, lo), bnd=None, pad=65)
        s[f"convert_lo {kind}"] = dict(got=tc.convert_ref(x, 8, lo), ref=tc.convert_ref(x, 8, lo), bnd=None, pad=5)
        v, b32 = tc.grad_operands_ref(x, z, 1)
        v32, _ = tc.grad_operands_ref(x, z, 1, dt=F32)
        s[f"grad_operands_lo {kind} dy_lo"] = dict(got=v32.to(lo), ref=v, bnd=tc.lo_bound(v, b32, lo), ulp=True)
        h = tc.gelu(z.double(), 2)
        s[f"gelu_fwd_lo {kind}"] = dict(got=tc.gelu(z, 2).to(lo), ref=h, bnd=tc.lo_bound(h, torch.full_like(h, tc.ACT_ABS), lo), ulp=True)
    s["transpose_f32"] = dict(got=tc.transpose_ref(x, 68, F32), ref=tc.transpose_ref(x, 68, F32), bnd=None, pad=65)
    part, b_part = tc.colpart_ref(*tc.grad_operands_ref(x, z, 1))
    s["grad_operands_lo colsum_part"] = dict(got=tc.colpart_ref(tc.grad_operands_ref(x, z, 1, dt=F32)[0], torch.zeros(65, 5, dtype=F64))[0], ref=part, bnd=b_part)

    a, b, vec, sc = torch.randn(9, 12, generator=g), torch.randn(9, 12, generator=g), torch.randn(12, generator=g), torch.randn(9, generator=g)
    s["add"] = dict(got=a + b, ref=a + b, bnd=None)
    s["mul"] = dict(got=a * b, ref=a * b, bnd=None)
    s["scale_rows"] = dict(got=a * sc[:, None], ref=a * sc[:, None], bnd=None)
    sw = sc.double()[:, None] * vec.double()[None, :]
    s["add_outer"] = dict(got=a + sc[:, None] * vec[None, :], ref=a.double() + sw, bnd=tc.fma_bound(sw, a.double()), slice_rel=tc.REL_SUM, limit=1.0)
    zz, dh = (torch.randn(40, 30, generator=g) * 2.5).clamp(-7.99, 7.99), torch.rand(40, 30, generator=g) * 2 - 1
    for kind in (1, 2):
        s[f"gelu_fwd {kind}"] = dict(got=tc.gelu(zz, kind), ref=tc.gelu(zz.double(), kind), bnd=torch.full((40, 30), tc.ACT_ABS, dtype=F64), limit=0.5)
        ref, bnd = tc.gelu_bwd_ref(zz, dh, kind)
        s[f"gelu_bwd {kind}"] = dict(got=tc.gelu_bwd_ref(zz, dh, kind, dt=F32)[0], ref=ref, bnd=bnd)

    big = torch.randn(max(cases.COLSUM_ROWS), 70, generator=g)
    out0 = torch.randn(70, generator=g)
    ref, bnd = tc.colsum_ref(big, out0)
    s["colsum"] = dict(got=tc.colsum_ref(big, out0, dt=F32)[0], ref=ref, bnd=bnd, slice_rel=tc.REL_SUM, rows=False)
    rows, cols = max(cases.ROWDOT_SHAPES, key=lambda rc: rc[1])
    aa, w, bias = torch.randn(rows, cols, generator=g), torch.randn(cols, generator=g), torch.randn(1, generator=g)
    ref, bnd = tc.rowdot_ref(aa, w, bias)
    s["rowdot"] = dict(got=tc.rowdot_ref(aa, w, bias, dt=F32)[0], ref=ref, bnd=bnd, slice_rel=tc.REL_SUM, rows=False)
    idx = cases.index_rows()
    dst0, upd = torch.randn(cases.IDX_SRC_ROWS, 30, generator=g), torch.randn(cases.IDX_ROWS, 30, generator=g)
    ref, bnd = tc.scatter_add_ref(dst0, idx, upd)
    s["scatter_add_rows"] = dict(got=tc.scatter_add_ref(dst0, idx, upd, dt=F32)[0], ref=ref, bnd=bnd, slice_rel=tc.REL_SUM)
    src = torch.randn(cases.IDX_SRC_ROWS, 30, generator=g)
    s["gather_rows"] = dict(got=src[idx.long()], ref=src[idx.long()], bnd=None)

    ids = cases.gather_ids()
    gsrc = torch.randn(cases.GATHER_V0, 30, generator=g).to(torch.bfloat16)
    fb, gsw, gsb, dx = (torch.randn(n, 30, generator=g) for n in (cases.GATHER_FB, 1, 1, cases.GATHER_T))
    ref, bnd = tc.gather_fwd_ref(ids, gsrc, cases.GATHER_V0, fb, gsw[0], gsb[0])
    emu = torch.where((ids >= cases.GATHER_V0)[:, None], fb[(ids.long() - cases.GATHER_V0).clamp(min=0)], gsw[0] * gsrc.float()[ids.long().clamp(max=cases.GATHER_V0 - 1)] + gsb[0])
    s["gather_fwd"] = dict(got=emu, ref=ref, bnd=bnd, slice_rel=tc.REL_SUM, limit=1.0)
    bw = tc.gather_bwd_ref(ids, gsrc, cases.GATHER_V0, cases.GATHER_FB, dx, fb)
    s["gather_bwd prod"] = dict(got=bw["prod"].clone(), ref=bw["prod"], bnd=None, row=int(torch.nonzero(ids < cases.GATHER_V0 - 0)[0]))
    s["gather_bwd dfallback"] = dict(got=bw["dfallback"].float(), ref=bw["dfallback"], bnd=bw["b_dfallback"], slice_rel=tc.REL_SUM)

    h = max(cases.LN_H)
    xx, gamma, beta, dy, dy2 = cases._ln_inputs(3, h, 1)
    ref = tc.layernorm_ref(xx, gamma, beta, 1e-5)
    bnd = tc.layernorm_bound(xx, gamma, beta, 1e-5, ref)
    emu = tc.layernorm_ref(xx, gamma, beta, 1e-5, dt=F32)
    s["layernorm_fwd y"] = dict(got=emu["y"], ref=ref["y"], bnd=bnd["y"], slice_rel=tc.REL_FWD)
    s["layernorm_fwd rstd"] = dict(got=emu["rstd"], ref=ref["rstd"], bnd=bnd["rstd"], rows=False)
    s["layernorm_fwd y_lo"] = dict(got=emu["y"].to(torch.float16), ref=ref["y"], bnd=tc.lo_bound(ref["y"], bnd["y"], torch.float16), ulp=True, at=(2, 100))
    stats = torch.stack([emu["mean"], emu["rstd"]], 1)
    ref, bnd = tc.layernorm_bwd_ref(dy, dy2, xx, stats, gamma, 2), tc.layernorm_bwd_bound(dy, dy2, xx, stats, gamma, 2)
    emu = tc.layernorm_bwd_ref(dy, dy2, xx, stats, gamma, 2, dt=F32)
    s["layernorm_bwd dx"] = dict(got=emu["dx"], ref=ref["dx"], bnd=bnd["dx"], slice_rel=tc.REL_BWD)
    s["layernorm_bwd partials"] = dict(got=emu["partials"].reshape(4, h), ref=ref["partials"].reshape(4, h), bnd=bnd["partials"].reshape(4, h))

    for name, case in (("dense", dict(form="dense", seq=32, d=128, heads=3, seed=7)), ("packed", dict(form="packed", seq=16, d=256, heads=1, seed=8)),
                       ("cls", dict(form="cls", seq=32, d=128, heads=2, seed=9))):
        lens, offs, q, k, v, dctx, mask = cases._attention_inputs(case)
        cls = case["form"] == "cls"
        ref = tc.attention_ref(q, k, v, mask, offs, case["heads"], case["d"], cls)
        emu = tc.attention_ref(q, k, v, mask, offs, case["heads"], case["d"], cls, dt=F32)
        s[f"attention_fwd ctx {name}"] = dict(got=emu["ctx"], ref=ref["ctx"], bnd=ref["b_ctx"], slice_rel=tc.REL_FWD)
        s[f"attention_fwd probs {name}"] = dict(got=emu["probs"][0].reshape(-1, lens[0]), ref=ref["probs"][0].reshape(-1, lens[0]), bnd=ref["b_probs"][0].reshape(-1, lens[0]))
        s[f"attention_fwd ctx_lo {name}"] = dict(got=emu["ctx"].to(torch.bfloat16), ref=ref["ctx"], bnd=tc.lo_bound(ref["ctx"], ref["b_ctx"], torch.bfloat16), ulp=True)
        bref = tc.attention_bwd_ref(dctx, q, k, v, emu["probs"], offs, case["heads"], case["d"], cls)
        bemu = tc.attention_bwd_ref(dctx, q, k, v, emu["probs"], offs, case["heads"], case["d"], cls, dt=F32)
        for t in ("dq", "dk", "dv"):
            s[f"attention_bwd {t} {name}"] = dict(got=bemu[t], ref=bref[t], bnd=bref["b_" + t], slice_rel=tc.REL_BWD, row=4 if cls and t == "dq" else None)
    return s


_S = {}


def _spec(name):
    if not _S:
        _S.update(_specimens())
    return _S[name]


SPECIMENS = (
    [f"{op} {k}" for k in ("bf16", "f16") for op in ("transpose_lo", "transpose_lo16", "convert_lo", "grad_operands_lo", "gelu_fwd_lo")]
    + ["transpose_f32", "grad_operands_lo colsum_part", "add", "mul", "scale_rows", "add_outer", "gelu_fwd 1", "gelu_fwd 2", "gelu_bwd 1", "gelu_bwd 2", "colsum", "rowdot",
       "scatter_add_rows", "gather_rows", "gather_fwd", "gather_bwd prod", "gather_bwd dfallback", "layernorm_fwd y", "layernorm_fwd rstd", "layernorm_fwd y_lo", "layernorm_bwd dx",
       "layernorm_bwd partials"]
    + [f"attention_{t} {f}" for f in cases.ATT_FORMS for t in ("fwd ctx", "fwd probs", "fwd ctx_lo", "bwd dq", "bwd dk", "bwd dv")])
SPECIMENS = [n.replace("grad_operands_lo bf16", "grad_operands_lo bf16 dy_lo").replace("grad_operands_lo f16", "grad_operands_lo f16 dy_lo") for n in SPECIMENS]


def _verify(spec, got, what):
    if spec["bnd"] is None:
        return tc.exact(got, spec["ref"], what)
    return tc.check(got, spec["ref"], spec["bnd"], what, slice_rel=spec.get("slice_rel"))


def test_the_specimen_list_is_complete():
    assert sorted(SPECIMENS) == sorted(_specimens())


@pytest.mark.parametrize("name", SPECIMENS)
def test_clean_emulation_passes_with_a_margin(name):
    """the sequential fp32 emulation stays below a quarter of every bound at the largest reduction lengths of the GPU cases (h = 8192,
    d = 256, 32 positions, 1000 rows, 1030 columns, 50 hits of one row); a GELU below half of its allowance (one fp32 ulp just
    below |z| = 8 is 0.48e-6 of the 1e-6: two roundings cannot promise less; the inputs stay below 8 for that reason); a single
    multiply-add and a 16-bit output below their bound, which IS the rounding of that arithmetic"""
    spec = _spec(name)
    out = _verify(spec, spec["got"], name)
    if out is not None:
        assert out[0] <= (1.0 if spec.get("ulp") else spec.get("limit", 0.25)), (name, out)          # (a 16-bit output: its own rounding IS the bound)


def _as2d(t):
    return t.reshape(1, -1) if t.dim() < 2 else t.reshape(t.shape[0], -1)


def _flagged(spec, got, what):
    with pytest.raises(tc.OpMismatch) as e:
        _verify(spec, got, what)
    return e.value


def _bump(t, row, col, ulps):
    """move one element away from zero by `ulps` units in the last place of its own type"""
    bits = tc._bits(t).clone().reshape(_as2d(t).shape)
    bits[row, col] += ulps
    return bits.view(t.dtype).reshape(t.shape)


@pytest.mark.parametrize("name", SPECIMENS)
def test_one_element_off_is_found_at_its_place(name):
    spec = _spec(name)
    got = _as2d(spec["got"]).clone()
    ref = _as2d(spec["ref"])
    row, col = spec.get("at", (got.shape[0] // 2, got.shape[1] // 3))          # (at: away from the row of variance 0, whose bound is wide)
    if float(ref[row, col]) == 0:                                  # (a masked probability, a zero band: take the largest element instead)
        flat = int(torch.argmax(ref.double().abs()))
        row, col = flat // got.shape[1], flat % got.shape[1]
    if spec["bnd"] is None or spec.get("ulp"):
        got = _bump(got, row, col, 4)
    else:
        got[row, col] += 4 * float(_as2d(spec["bnd"])[row, col]) + 4 * tc.U * abs(float(got[row, col]))
    e = _flagged(spec, got.reshape(spec["got"].shape), name + ", one element off")
    assert (e.row, e.col) == (row, col) and int(e.bad.sum()) == 1 and name in str(e) and f"(row {row}, column {col})" in str(e)


@pytest.mark.parametrize("name", [n for n in SPECIMENS if n not in ("colsum", "rowdot", "layernorm_fwd rstd")])
def test_a_row_taken_from_its_neighbour_is_found(name):
    spec = _spec(name)
    got = _as2d(spec["got"]).clone()
    row = spec.get("row") if spec.get("row") is not None else min(2, got.shape[0] - 2)
    assert not torch.equal(tc._bits(got[row]), tc._bits(got[row + 1]))
    got[row] = got[row + 1]
    e = _flagged(spec, got.reshape(spec["got"].shape), name + ", a row from its neighbour")
    assert e.row == row and set(torch.nonzero(e.bad.any(1)).flatten().tolist()) == {row}
    assert int(e.bad[row].sum()) >= max(1, got.shape[1] // 2)       # most of the row, not one element of it


@pytest.mark.parametrize("name", [f"{op} {k}" for k in ("bf16", "f16") for op in ("transpose_lo", "transpose_lo16", "convert_lo")] + ["transpose_f32"])
def test_a_pad_band_filled_with_the_last_real_row_is_found(name):
    spec = _spec(name)
    pad = spec["pad"]
    got = spec["got"].clone()
    got[:, pad:] = got[:, pad - 1:pad]
    e = _flagged(spec, got, name + ", pad band filled")
    cols = set(torch.nonzero(e.bad.any(0)).flatten().tolist())
    assert cols and cols <= set(range(pad, got.shape[1])) and e.col >= pad
    assert int(e.bad[:, pad:].sum()) >= (got.shape[1] - pad) * (got.shape[0] - 1)      # the whole band (but for a source value that is 0)


def test_canary_of_a_16_bit_output():
    f = tc.Frame(3, 5, 8, torch.bfloat16, "canary")
    assert bool(torch.isnan(f.buf.float()).all()) and f.overwritten(f.buf) == []
    buf = f.buf.clone()
    f.view(buf).fill_(1.0)
    tc.check_canary(f, buf, "written inside")
    buf[f.offset + 6] = 2.0                                          # row 0, column 6: a canary column
    with pytest.raises(tc.CanaryBroken) as e:
        tc.check_canary(f, buf, "column 6")
    assert e.value.where == [(0, 6)]
    h = tc.Frame(None, 7, 7, torch.float16, "canary")
    assert bool(torch.isnan(h.buf.float()).all())


def test_the_16_bit_rule():
    """lo_bound: half an ulp of the type at the reference, the fp32 allowance, one more ulp only across a rounding boundary"""
    ref = torch.tensor([1.0, 1.0 + 2.0 ** -8, 3.0, 2.0 ** -130], dtype=F64)       # bf16: spacing 2^-7 at 1, 2^-6 at 3
    b = tc.lo_bound(ref, torch.full((4,), 1e-6, dtype=F64), torch.bfloat16)
    assert float(b[0]) == 1e-6 + 2.0 ** -8 and float(b[1]) == 1e-6 + 2.0 ** -8 + 2.0 ** -7 and float(b[2]) == 1e-6 + 2.0 ** -7
    assert float(tc.ulp_lo(ref, torch.bfloat16)[3]) == 2.0 ** -133 and float(tc.ulp_lo(torch.tensor([1e-6], dtype=F64), torch.float16)) == 2.0 ** -24


# ---- the case tables reach every branch --------------------------------------------------------------------------------------
def _transpose_branches(case):
    """The forms transpose_lo_kernel takes for a case, restated from zett_amd/csrc/train_operands.hip:
        load4_edge:  one access where c + 3 < C and ld_in % 4 == 0, the element tail otherwise (same for act_z with ld_z)
        plain:       store4 where c + 3 < C and ld_plain % 4 == 0, scalar otherwise
        transposed:  store4 where r + 3 < Rpad and ld_out % 4 == 0, scalar otherwise (the last group of a band when Rpad % 4 != 0)
        colpart:     a last band that is partly rows, partly padding (R % 64 != 0), and bands that are padding only (r0 >= R)"""
    R, Rpad, Cc = case["R"], case["Rpad"], case["C"]
    ld_in, ld_out, ld_plain, ld_z = Cc + case["d_in"], Rpad + case["d_out"], Cc + case["d_plain"], Cc + case["d_z"]
    out = set()
    for name, ld in (("in", ld_in), ("z", ld_z), ("plain", ld_plain)):
        if ld % 4 == 0 and Cc >= 4:
            out.add(name + " vector")
        if ld % 4 != 0:
            out.add(name + " scalar: ld")
        if ld % 4 == 0 and Cc % 4 != 0:
            out.add(name + " scalar: column tail")
    if ld_out % 4 == 0 and Rpad >= 4:
        out.add("out vector")
    if ld_out % 4 != 0:
        out.add("out scalar: ld")
    if ld_out % 4 == 0 and Rpad % 4 != 0:
        out.add("out scalar: last group of the band")
    if R % 64 != 0 and Rpad > R:
        out.add("colpart: band of rows and padding")
    if (Rpad + 63) // 64 > (R + 63) // 64:
        out.add("band of padding only")
    out.add("act kind %d" % case["kind"])
    out.add("convert: rows of four" if cases.convert_wide(Cc, case["cols_padded"], ld_in, case["cols_padded"]) else "convert: general cast")
    if case["cols_padded"] > Cc:
        out.add("convert: zero columns")
    return out


def test_the_transpose_cases_reach_every_form():
    want = {f"{n} {f}" for n in ("in", "z", "plain") for f in ("vector", "scalar: ld", "scalar: column tail")} | {
        "out vector", "out scalar: ld", "out scalar: last group of the band", "colpart: band of rows and padding", "band of padding only", "act kind 1", "act kind 2",
        "convert: rows of four", "convert: general cast", "convert: zero columns"}
    seen = set()
    for rows in cases.T_ROWS:
        table = cases.transpose_cases(rows)
        assert {c["C"] for c in table} == set(cases.T_COLS) and {c["Rpad"] for c in table} == {rows, (rows + 63) // 64 * 64, rows + 3}
        for c in table:
            seen |= _transpose_branches(c)
    assert seen == want
    for name in ("d_in", "d_out", "d_plain", "d_z"):
        assert {c[name] for rows in cases.T_ROWS for c in cases.transpose_cases(rows)} == {0, 1, 2, 4}
    rows, cols = cases.CONVERT_STRIDE
    assert rows > 65535 and cases.convert_wide(cols, cols, cols, cols)          # min(rows, 65535) workgroups: the loop strides


def test_the_elementwise_cases_reach_both_widths_and_the_second_pass():
    assert {cases.elementwise_wide(*c) for c in cases.EW_SHAPES} == {True, False}
    assert not cases.elementwise_wide(33, 1028, 1) and cases.elementwise_wide(33, 1028, 0) and not cases.elementwise_wide(7, 30, 0)
    cap = 65535 * 256                                               # grid_for: min((n + 255) / 256, 65535) workgroups of 256
    assert cases.EW_STRIDE["wide"] % 4 == 0 and cap < cases.EW_STRIDE["wide"] // 4 < cap + 512
    assert cases.EW_STRIDE["scalar"] % 4 != 0 and cap < cases.EW_STRIDE["scalar"] < cap + 512
    assert {n % 4 for n in cases.GELU_LO_N} == {0, 1, 3}


def test_the_layernorm_cases_reach_every_register_layout():
    """J = ceil(h / 1024) -> 1 / 2 / 4 / 8 (zett_op_layernorm_fwd_f32 / _bwd_f32: j <= 1, <= 2, <= 4, else 8); a partly filled last pass
    is h % 1024 != 0 above 1024 or a J that is not ceil(h / 1024)"""
    assert [cases.ln_j(h) for h in cases.LN_H] == [1, 1, 1, 1, 2, 2, 4, 4, 8, 8]
    assert {cases.ln_j(h) for h in cases.LN_H} == {1, 2, 4, 8}
    assert {h for h in cases.LN_H if h > 1024 and h % 1024} == {1028, 2052, 4100} and cases.ln_j(2052) * 1024 >= 2 * 2052 - 8
    for rows in cases.LN_ROWS:
        parts = cases.ln_nparts(rows)
        assert 1 in parts and rows in parts and rows + 5 in parts and (2 in parts)
    assert cases.LN_STRIDE[0] > 16384 and cases.ln_j(cases.LN_STRIDE[1]) == 1


def test_the_attention_table_holds_every_layout_in_every_form():
    """LMAX from seq (attn_fwd_go: <= 2, 4, 8, 16, else 32), DV from head_dim (<= 64: 1, <= 128: 2, else 4); the backward refuses
    DV = 4 with LMAX = 32"""
    table = cases.attention_cases()
    assert 35 <= len(table) <= 45
    pairs = {(lm, dv) for lm in (2, 4, 8, 16, 32) for dv in (1, 2, 4)}
    for form in cases.ATT_FORMS:
        mine = [c for c in table if c["form"] == form]
        assert {(cases.att_lmax(c["seq"]), cases.att_dv(c["d"])) for c in mine} == pairs
        assert {c["heads"] for c in mine} == {1, 3, 5} and {c["d"] for c in mine} == {8, 64, 72, 128, 136, 256}
        assert {c["wide_ld"] for c in mine} == {False, True} and {c["ctx_lo"] for c in mine} == {None, "bf16", "f16"}
        assert {c["fused"] for c in mine} == ({False} if form == "cls" else {False, True})
        for c in mine:
            lens = cases.attention_lengths(c)
            assert max(lens) == c["seq"] and (form == "dense" or min(lens) == 1) and all(1 <= n <= c["seq"] for n in lens)
    assert {c["seq"] for c in table} == {1, 2, 3, 4, 5, 8, 9, 16, 17, 32}
    assert [cases.att_lmax(s) for s in (1, 2, 3, 4, 5, 8, 9, 16, 17, 32)] == [2, 2, 4, 4, 8, 8, 16, 16, 32, 32]
    assert [cases.att_dv(d) for d in (8, 64, 72, 128, 136, 256)] == [1, 1, 2, 2, 4, 4]
    refused = {(cases.att_lmax(c["seq"]), cases.att_dv(c["d"])) for c in table if cases.att_bwd_refused(c["seq"], c["d"])}
    assert refused == {(32, 4)}
    assert {c["d"] % 64 != 0 for c in table} == {True, False}       # a partly filled 64-column slice: the c < d guards decide


def test_the_index_cases_reach_every_pass_and_edge():
    assert {(c + 255) // 256 for c in cases.IDX_COLS} == {1, 2, 3} and {c % 4 != 0 for c in cases.IDX_COLS} == {True, False}
    idx = cases.index_rows()
    assert set(idx.tolist()) == set(range(cases.IDX_SRC_ROWS)) and int((idx == 5).sum()) >= 50 and idx.numel() == cases.IDX_ROWS
    ids = cases.gather_ids().tolist()
    assert set(cases.GATHER_EDGE_IDS) <= set(ids) and max(ids) == cases.GATHER_V0 + cases.GATHER_FB - 1 and min(ids) == 0
    assert {(c + 255) // 256 for _, c in cases.ROWDOT_SHAPES} == {1, 2, 5} and {r % 4 for r in cases.COLSUM_ROWS} >= {0, 1, 3}
