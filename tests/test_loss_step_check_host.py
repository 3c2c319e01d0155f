"""The checker of the loss and optimizer-step kernels (tests/loss_step_check.py) passes a right kernel, reports a subtly wrong one AT
ITS PLACE, and the case tables of tests/test_loss_step_direct_gpu.py reach every branch they claim to (no GPU).

A right kernel is the fp32 emulation: the reference formulas in fp32, the long sums in the order the kernels document.  It must stay
at or below 0.25 of every bound that holds a long sum (lse, row_loss, row_dist, row_tnorm, the chunk partials) with all constants at
1.  For ce_rows it uses torch's exp / log — what __expf and logf add on the device is what C_CE_LSE, C_CE_LOSS and C_CE_G are for.
Two kinds of bound are held differently, and why:
  * a bound that is a handful of fp32 roundings at one U each (the words of the finalize records: one; an element of G at its label,
    of dpred, of AdamW's p, m, v: two to six): U is the round-off twice over, so a right kernel whose operations all round the same
    way reaches exactly half of such a bound.  0.5 is the ceiling there and what is asserted (LIMIT_FEW); the project's
    tests/test_train_ops_check_host.py holds its multiply-add bounds the same way;
  * a 16-bit G: half an ulp of the type IS the bound (train_ops_check.lo_bound), the emulation is only asserted to pass.
"""
import pytest
import torch

from tests import loss_step_check as lc
from tests import test_loss_step_direct_gpu as cases
from tests import train_ops_check as tc

F32, F64 = torch.float32, torch.float64
LIMIT_FEW = 0.5


def _ratio(got, ref, bnd):
    err = (got.double() - ref.double()).abs()
    assert bool(torch.isfinite(err).all())
    r = torch.where(err == 0, torch.zeros_like(err), err / bnd.double().clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0


def _quarter(got, ref, bnd, c, what, limit=0.25):
    """the emulation against a bound that carries the constant c: at or below `limit` of the bound WITH THE CONSTANT AT 1"""
    r = _ratio(got, ref, bnd) * c
    assert r <= limit, f"{what}: the fp32 emulation is at {r:.3f} of the bound"
    return r


# ---- the emulation stays inside a quarter of every bound -----------------------------------------------------------------------------
def _ce_specimens():
    out = [(f"case {c['i']}", *lc.ce_inputs(c), c["v"]) for c in lc.ce_cases()]
    z, labels, _ = lc.ce_special()
    out.append(("ties and ranges", z, labels, torch.tensor([lc.CE_WEIGHTS[r % 5] for r in range(z.shape[0])], dtype=F32), lc.CE_SPECIAL["v"]))
    z, labels, w = lc.ce_stride()
    out.append(("grid stride", z[:300], labels[:300], w[:300], lc.CE_STRIDE["v"]))
    return out


@pytest.mark.parametrize("spec", _ce_specimens(), ids=lambda s: s[0])
def test_ce_rows_emulation(spec):
    name, z, labels, w, v = spec
    ref, emu = lc.ce_rows_ref(z, labels, w, v), lc.ce_rows_ref(z, labels, w, v, dt=F32)
    bnd = lc.ce_rows_bound(ref, z.shape[1])
    _quarter(emu["lse"], ref["lse"], bnd["lse"], lc.C_CE_LSE, name + " lse")
    _quarter(emu["loss"], ref["loss"], bnd["loss"], lc.C_CE_LOSS, name + " row_loss")
    _quarter(emu["G"], ref["G"], bnd["G"], lc.C_CE_G, name + " G", limit=LIMIT_FEW)
    assert torch.equal(emu["argmax"], ref["argmax"])
    for dt in (torch.bfloat16, torch.float16):
        tc.check(emu["G"].to(dt), ref["G"], tc.lo_bound(ref["G"], bnd["G"], dt), f"{name} G as {dt}")
    dead = ~ref["live"]
    assert bool((emu["G"][dead] == 0).all()) and bool((emu["G"][:, v:] == 0).all()) and not bool(torch.signbit(emu["G"][dead]).any())


@pytest.mark.parametrize("c", lc.dist_cases(), ids=lambda c: f"e{c['e']}-k{c['kind']}-{c['sd']}-{c['switch']}")
def test_distance_emulation(c):
    inp = lc.dist_inputs(c)
    for grad in (False, True):
        vec = lc.dist_vec_ok(c, grad)
        ref, emu = lc.dist_rows_ref(inp["pred"], inp["tgt"], inp["mask"], c["kind"], vec), lc.dist_rows_ref(inp["pred"], inp["tgt"], inp["mask"], c["kind"], vec, dt=F32)
        _quarter(emu["dist"], ref["dist"], ref["b_dist"], lc.C_DIST, "row_dist")
        _quarter(emu["tnorm"], ref["tnorm"], ref["b_tnorm"], lc.C_DIST, "row_tnorm")
    rd = ref["dist"].float()
    val, bnd = lc.dist_grad_ref(inp["pred"], inp["tgt"], inp["mask"], rd, c["kind"], cases.RECORD1, cases.UPSTREAM)
    emu, _ = lc.dist_grad_ref(inp["pred"], inp["tgt"], inp["mask"], rd, c["kind"], cases.RECORD1, cases.UPSTREAM, dt=F32)
    _quarter(emu, val, bnd, lc.C_DIST, "dpred", limit=LIMIT_FEW)
    if c["kind"] == lc.RMSE and c["n"] > 1:
        assert bool((emu[1] == 0).all())                      # the row equal to its target


def test_distance_inputs_hold_the_errors_the_issue_names():
    seen = set()
    for c in lc.dist_cases():
        inp = lc.dist_inputs(c)
        err = inp["pred"].double() - inp["tgt"].double()
        assert float(err[0, 0]) == lc.HUBER_DELTA                                     # exactly the knee, as an fp32 value
        if c["n"] > 1:
            assert float(err[-1, 0]) == -lc.HUBER_DELTA and bool((err[1] == 0).all())
        if c["e"] >= 252 and c["n"] > 2:
            assert bool((err[2].abs() < lc.HUBER_DELTA).any()) and bool((err[2].abs() > lc.HUBER_DELTA).any())
        seen |= {int(x) for x in inp["ids"][:, 0]}
        if c["ids_stride"] > 1:
            assert bool((inp["ids"][:, 1:] >= 10 ** 9).all())                         # a wild row if it were read
        assert bool(torch.isnan(inp["src"][:, :c["col0"]].float()).all()) and bool(torch.isnan(inp["src"][:, c["col0"] + c["e"]:].float()).all())
    assert {-1, -2 ** 40, lc.DIST_SRC_ROWS, lc.DIST_SRC_ROWS + 7, 2 ** 40, 0, lc.DIST_SRC_ROWS - 1} <= seen


@pytest.mark.parametrize("n,aligned", [(65536, True), (65536, False), (65535, True), (1025, True), (1025, False), (5, True), (3, False), (1, True)])
def test_sumsq_emulation(n, aligned):
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 0.1
    ref, bnd = lc.partials_ref([g], [0 if aligned else 1])
    _quarter(lc.sumsq32(g, aligned).reshape(1), ref, bnd, 1.0, f"sumsq n={n} aligned={aligned}")


@pytest.mark.parametrize("step,coef,decay", [(1, 1.0, True), (1000, 0.3125, False), (1000, 1.0, True)])
def test_adamw_emulation(step, coef, decay):
    h = lc.adam_hyper(**cases.HYPER)
    rec = cases._record_in(coef, 0, step, cases.HYPER["b1"], cases.HYPER["b2"])
    worst = 0.0
    for i, en in enumerate(lc.mt_list()[:20]):
        if not en["n"]:
            continue
        p, g, m, v = (lc.mt_values(en, i, w) for w in range(4))
        ref = lc.adamw_ref(p, g, m, v, h, float(rec[1]), float(rec[4]), float(rec[5]), decay)
        emu = lc.adamw_ref(p, g, m, v, h, float(rec[1]), float(rec[4]), float(rec[5]), decay, dt=F32)
        for nm in ("p", "m", "v"):
            worst = max(worst, _quarter(emu[nm], ref[nm], ref["b_" + nm], lc.C_ADAMW, f"adamw tensor {i} {nm}", limit=LIMIT_FEW))
    assert worst > 0


def test_the_finalize_records_round_once():
    """a float64 result rounded to fp32 is the emulation here: at most U / 2, half of the one-rounding bound"""
    g = torch.Generator().manual_seed(3)
    n = 1000
    rl, w = torch.rand(n, generator=g) * 5, torch.tensor([1.0, 0.0, -0.0, -0.5, 2.5])[torch.arange(n) % 5]
    labels = torch.randint(0, 9, (n,), generator=g, dtype=torch.int32)
    vals, bnd, nc, nn = lc.ce_finalize_ref(rl, w, labels, labels.clone())
    _quarter(vals.float(), vals, bnd, 1.0, "ce_finalize", limit=LIMIT_FEW)
    assert nn == int((w > 0).sum()) == nc == 400                                      # 1.0 and 2.5 count; 0, -0.0 and -0.5 do not
    assert lc.ce_finalize_ref(torch.zeros(4), torch.tensor([0.0, -0.0, 0.0, -0.0]), labels[:4], labels[:4])[0].tolist() == [0.0, 0.0, 0.0]
    for mode in (lc.MEAN, lc.LEXICAL):
        for mask in (None, (torch.arange(n) % 3 != 0).float(), torch.zeros(n)):
            vals, bnd = lc.dist_finalize_ref(rl, rl + 0.5, mask, mode)
            assert bool(torch.isfinite(vals).all())
            _quarter(vals.float(), vals, bnd, 1.0, "dist_finalize", limit=LIMIT_FEW)
    want = lc.norm_record_ref(rl, 1.0, 0.9, 0.999, 999)
    for nm in ("norm", "coef", "c1", "c2"):
        _quarter(want[nm][0].float(), want[nm][0], want[nm][1], 1.0, nm, limit=LIMIT_FEW)
    assert want["step"] == 1000 and want["skip"] == 0


def test_exact_references():
    g = torch.Generator().manual_seed(4)
    bias, priors = torch.randn(5, generator=g), torch.randn(5, generator=g)
    mask = torch.tensor([0, 1, 255, 0, 1], dtype=torch.uint8)
    a = lc.addend_ref(bias, priors, mask, 5, 8)
    assert a.shape == (8,) and bool((a[5:] == 0).all()) and float(a[0]) == float((torch.tensor(-100000.0) + bias[0]) + priors[0]) and float(a[1]) == float(bias[1] + priors[1])
    assert bool((lc.scale_ref(torch.randn(9, generator=g), 0.0, 1.7, torch.bfloat16).float() == 0).all())
    ids = torch.tensor([[3, 3, 3], [3, 4, 3], [4, 3, 3]])
    assert lc.single_token_mask_ref(ids, 3, 3).tolist() == [1.0, 0.0, 1.0] and lc.single_token_mask_ref(ids, 1, 3).tolist() == [1.0, 1.0, 1.0]


# ---- planted errors are reported at their place ------------------------------------------------------------------------------------------
def _ce_planted_case():
    c = next(c for c in lc.ce_cases() if c["vp"] == 8196 and c["v"] == 8195)
    z, labels, _ = lc.ce_inputs(c)
    labels = torch.tensor([lc.ce_edge_columns(c["v"], c["vp"])[0]] * c["rows"], dtype=torch.int32)      # the last column of a lane's last vector
    w = torch.tensor([2.5, 0.0, 1.0, 1.0, 1.0][:c["rows"]])
    ref = lc.ce_rows_ref(z, labels, w, c["v"])
    return c, z, labels, w, ref, lc.ce_rows_bound(ref, c["vp"]), lc.ce_rows_ref(z, labels, w, c["v"], dt=F32)


def test_planted_g_element_off_by_a_16_bit_ulp():
    c, z, labels, w, ref, bnd, emu = _ce_planted_case()
    for dt in (torch.bfloat16, torch.float16):
        b = tc.lo_bound(ref["G"], bnd["G"], dt)
        got = emu["G"].to(dt).double()
        tc.check(got, ref["G"], b, "G")
        r, col = 2, 4321
        got[r, col] = ref["G"][r, col] + b[r, col] + tc.ulp_lo(ref["G"][r, col], dt)
        with pytest.raises(lc.OpMismatch) as e:
            tc.check(got, ref["G"], b, "G")
        assert (e.value.row, e.value.col) == (r, col) and int(e.value.bad.sum()) == 1


def test_planted_one_hot_beside_the_label():
    c, z, labels, w, ref, bnd, emu = _ce_planted_case()
    lab = int(labels[0])
    wrong = lc.ce_rows_ref(z, labels + 1, w, c["v"], dt=F32)["G"]
    for dt, b in ((F32, bnd["G"]), (torch.bfloat16, tc.lo_bound(ref["G"], bnd["G"], torch.bfloat16))):
        with pytest.raises(lc.OpMismatch) as e:
            tc.check(wrong.to(dt), ref["G"], b, "G")
        assert e.value.col in (lab, lab + 1) and set(torch.nonzero(e.value.bad.any(0)).flatten().tolist()) == {lab, lab + 1}
        assert set(e.value.bad.any(1).nonzero().flatten().tolist()) == set(range(c["rows"])) - {1}
        assert not bool(e.value.bad[1].any())                                     # (the row of weight 0 has no one-hot)


def test_planted_pad_column_and_zero_weight_row():
    c, z, labels, w, ref, bnd, emu = _ce_planted_case()
    v, vp = c["v"], c["vp"]
    G = emu["G"].clone()
    tc.exact(G[:, v:].contiguous(), torch.zeros(G.shape[0], vp - v), "pad")
    G[2, v] = 1e-30
    with pytest.raises(lc.OpMismatch) as e:
        tc.exact(G[:, v:].contiguous(), torch.zeros(G.shape[0], vp - v), "pad")
    assert (e.value.row, e.value.col) == (2, 0)
    with pytest.raises(lc.OpMismatch):
        tc.check(G, ref["G"], bnd["G"], "G")                                       # the element bound of a pad column is 0 too
    G = emu["G"].clone()
    dead = ~ref["live"]
    assert dead.tolist() == [False, True, False, False, False][:c["rows"]]
    G[1, 17] = -0.0                                                                 # even a zero of the wrong sign
    with pytest.raises(lc.OpMismatch) as e:
        tc.exact(G[dead].contiguous(), torch.zeros(1, vp), "zero row")
    assert (e.value.row, e.value.col) == (0, 17)
    G[1, 17] = 1e-30
    with pytest.raises(lc.OpMismatch) as e:
        tc.check(G, ref["G"], bnd["G"], "G")
    assert (e.value.row, e.value.col) == (1, 17)


def test_planted_last_of_two_tied_maxima():
    z, labels, want = lc.ce_special()
    ref = lc.ce_rows_ref(z, labels, None, lc.CE_SPECIAL["v"])
    assert torch.equal(ref["argmax"], want)
    for r, (a, b) in enumerate(lc.CE_TIES):
        got = want.clone()
        got[r] = b
        with pytest.raises(lc.OpMismatch) as e:
            tc.exact(got, want, "argmax")
        assert e.value.col == r
    got = want.clone()
    got[6] = lc.CE_SPECIAL["v"]                                                    # the larger value in the pad column
    with pytest.raises(lc.OpMismatch):
        tc.exact(got, want, "argmax")


def test_planted_partial_one_slot_late():
    grads = [torch.randn(n, generator=torch.Generator().manual_seed(n)) for n in (5, 131077, 0, 1025)]
    ref, bnd = lc.partials_ref(grads, [0, 0, 0, 1])
    total = 5                                                                     # 1 + 3 + 0 + 1 chunks
    assert ref.shape[0] == total == sum(lc.mt_items(g.shape[0]) for g in grads)
    frame = tc.Frame(None, total + 4, total + 4, F32, "canary")
    buf = frame.buf.clone()
    frame.view(buf)[:total] = ref.float()
    got = frame.view(buf)
    tc.check(got[:total], ref, bnd, "partials")
    canary = torch.full((4,), tc.CANARY_BITS, dtype=torch.int32)
    tc.exact(got[total:].view(torch.int32), canary, "beyond")
    frame.view(buf)[2:total + 1] = ref.float()[1:]                                 # the chunks after the first, each one slot late
    frame.view(buf).view(torch.int32)[1] = tc.CANARY_BITS
    with pytest.raises(lc.OpMismatch) as e:
        tc.check(got[:total], ref, bnd, "partials")
    assert e.value.col == 1
    with pytest.raises(lc.OpMismatch) as e:
        tc.exact(got[total:].view(torch.int32), canary, "beyond")
    assert e.value.col == 0


def test_planted_adamw_errors():
    h = lc.adam_hyper(**cases.HYPER)
    en = lc.mt_list()[3]
    p, g, m, v = (lc.mt_values(en, 3, w) for w in range(4))
    ref = lc.adamw_ref(p, g, m, v, h, 1.0, 0.1, 0.001, False)
    tc.check(lc.adamw_ref(p, g, m, v, h, 1.0, 0.1, 0.001, False, dt=F32)["p"], ref["p"], ref["b_p"], "p")
    with pytest.raises(lc.OpMismatch):
        tc.check(lc.adamw_ref(p, g, m, v, h, 1.0, 0.1, 0.001, True, dt=F32)["p"], ref["p"], ref["b_p"], "p")      # weight decay on a no-decay tensor
    frozen = p.clone()
    frozen[2] = torch.nextafter(frozen[2], torch.tensor(9.0))
    with pytest.raises(lc.OpMismatch) as e:
        tc.exact(frozen, p, "a frozen tensor's parameter")
    assert e.value.col == 2


def test_planted_dpred_at_the_wrong_leading_dimension():
    c = next(c for c in lc.dist_cases() if c["switch"] == "ld_dpred" and c["n"] >= 3 and c["e"] >= 4)
    assert c["ld_pred"] != c["ld_dpred"]
    inp = lc.dist_inputs(c)
    val, _ = lc.dist_grad_ref(inp["pred"], inp["tgt"], inp["mask"], torch.ones(c["n"]), c["kind"], 0.37, 1.7, dt=F32)
    frame = tc.Frame(c["n"], c["e"], c["ld_dpred"], F32, "canary")
    buf = frame.buf.clone()
    for r in range(c["n"]):
        buf[frame.offset + r * c["ld_pred"]:frame.offset + r * c["ld_pred"] + c["e"]] = val[r]
    with pytest.raises((lc.CanaryBroken, AssertionError)) as e:
        tc.check_canary(frame, buf, "dpred")
    if isinstance(e.value, lc.CanaryBroken):
        assert all(col >= c["e"] or row >= c["n"] for row, col in e.value.where)
    right = frame.buf.clone()
    frame.view(right).copy_(val)
    tc.check_canary(frame, right, "dpred")


def test_planted_target_row_without_the_clamp():
    c = next(c for c in lc.dist_cases() if c["n"] == 9 and c["kind"] == lc.MSE)
    inp = lc.dist_inputs(c)
    ids = inp["ids"][:, 0].long()
    out_of_range = ((ids < 0) | (ids >= lc.DIST_SRC_ROWS)).nonzero().flatten().tolist()
    assert out_of_range
    block = inp["src"][:, c["col0"]:c["col0"] + c["e"]].float()
    wrong_tgt = block[ids % lc.DIST_SRC_ROWS]                                      # what an unclamped index that stays inside the table would fetch
    ref = lc.dist_rows_ref(inp["pred"], inp["tgt"], inp["mask"], c["kind"], True)
    wrong = lc.dist_rows_ref(inp["pred"], wrong_tgt, inp["mask"], c["kind"], True, dt=F32)
    with pytest.raises(lc.OpMismatch) as e:
        tc.check(wrong["tnorm"], ref["tnorm"], ref["b_tnorm"], "row_tnorm")
    assert e.value.col in out_of_range and set(e.value.bad.nonzero()[:, 1].tolist()) <= set(out_of_range)


def test_planted_clip_comparison():
    """`norm < max_norm` against `norm <= max_norm`: at norm == max_norm the other branch is max_norm / norm, which is 1.0 too, so the
    two are the same bits there and nothing can tell them apart; what a check CAN see is a clip that is not applied above max_norm"""
    parts = torch.tensor([9.0, 16.0])
    want = lc.norm_record_ref(parts, 5.0, 0.9, 0.999, 0)
    assert float(want["norm"][0]) == 5.0 and float(want["coef"][0]) == 1.0 == 5.0 / 5.0
    above = lc.norm_record_ref(torch.tensor([9.0, 16.0, 1.0]), 5.0, 0.9, 0.999, 0)
    with pytest.raises(lc.OpMismatch):
        tc.check(torch.tensor([1.0]), above["coef"][0].reshape(1), above["coef"][1].reshape(1), "coef")
    with pytest.raises(lc.OpMismatch):
        tc.check(torch.tensor([float(above["coef"][0])], dtype=F32), want["coef"][0].reshape(1), want["coef"][1].reshape(1), "coef")      # (below the threshold: exactly 1)
    for bad in (float("inf"), float("nan")):
        r = lc.norm_record_ref(torch.tensor([1.0, bad]), 5.0, 0.9, 0.999, 4)
        assert r["skip"] == 1 and r["step"] == 4 and float(r["coef"][0]) == 0.0


# ---- the case tables reach every branch -------------------------------------------------------------------------------------------------
def test_ce_tables_reach_every_layout():
    table = lc.ce_cases()
    per_lane = lambda vp: (vp // 4 + 1023) // 1024
    assert {lc.ce_nv(c["vp"]) for c in table} == {1, 2, 4, 8, 0}
    assert {lc.ce_nv(c["vp"], lc.CE_TWICE) for c in table} == {0}
    for nv in (1, 2, 4, 8):                                                       # at, one vector below and one vector past every limit
        limit = nv * 4096
        widths = {c["vp"] for c in table}
        assert limit in widths and per_lane(limit) == nv and lc.ce_nv(limit) == nv
        assert (limit + 4 in widths and per_lane(limit + 4) == nv + 1) or limit == lc.CE_ONCE_MAX
        assert limit - 4 in widths or nv > 1
    assert lc.CE_ONCE_MAX + 4 in {c["vp"] for c in table} and 4 in {c["vp"] for c in table}
    for vp in lc.CE_WIDTHS:
        assert {c["vp"] - c["v"] for c in table if c["vp"] == vp} == {0, 1, 3}
    assert {c["g"] for c in table} == set(lc.CE_G_FORMS) and {(c["g"], c["d_z"]) for c in table} == {(g, dz) for g in lc.CE_G_FORMS for dz in (0, 4)}
    assert {c["d_g"] for c in table if c["g"] in ("f32", "bf16", "f16")} == {0, 4} and all(c["d_g"] == c["d_z"] for c in table if c["g"] == "inplace")
    assert {c["pad"] for c in table} == {"nan", "inf"} and {c["rows"] for c in table} == {3, 4, 5} and {c["weights"] for c in table} == {True, False}
    names, weights = set(), set()
    for c in table:
        z, labels, w = lc.ce_inputs(c)
        names |= {n for n in lc.CE_LABELS if lc.ce_label(n, c["v"], c["vp"]) in labels.tolist()}
        weights |= set() if w is None else {repr(float(x)) for x in w}
        pad = z[:, c["v"]:]
        assert bool(torch.isnan(pad).all()) if c["pad"] == "nan" else bool((pad == float("inf")).all())
        gap = lc.top_two_gap(z, c["v"])
        assert bool(((gap >= 1e-3) | (gap == 0)).all()), (c, gap)
    assert names == set(lc.CE_LABELS) and weights == {repr(float(torch.tensor(x, dtype=F32))) for x in lc.CE_WEIGHTS}
    assert 0 < float(torch.tensor(1e-40, dtype=F32)) < 2.0 ** -126                   # a subnormal weight
    last, nxt = lc.ce_edge_columns(8195, 8196)
    assert last % 4 == 3 and nxt == last + 1 and (last // 4) % 1024 + 1 == (nxt // 4) % 1024      # a lane's vector ends, the next lane's begins
    assert cases.lc.CE_STRIDE["rows"] > 65536


def test_ce_ties_sit_where_two_maxima_can_meet():
    z, labels, want = lc.ce_special()
    v = lc.CE_SPECIAL["v"]
    assert lc.ce_nv(lc.CE_SPECIAL["vp"]) == 4
    lane, vec, wave = (lambda c: (c // 4) % 1024), (lambda c: c // 4 // 1024), (lambda c: ((c // 4) % 1024) // 64)
    (a0, b0), (a1, b1), (a2, b2), (a3, b3), (a4, b4) = lc.CE_TIES
    assert a0 // 4 == b0 // 4                                                       # inside one float4
    assert lane(a1) == lane(b1) and vec(b1) == vec(a1) + 1 and b1 == a1 + 4096     # one lane's vector i and vector i + 1
    assert lane(a2) != lane(b2) and wave(a2) == wave(b2) and vec(a2) == vec(b2)    # two lanes of one wave
    assert wave(a3) != wave(b3) and vec(a3) == vec(b3)                             # two waves
    assert (a4, b4) == (0, v - 1)
    gap = lc.top_two_gap(z, v)
    assert gap[:6].tolist() == [0.0] * 6 and bool((gap[6:] >= 1e-3).all())           # bit-identical ties, else a unique maximum
    for r, (a, b) in enumerate(lc.CE_TIES):
        assert z[r, a].view(torch.int32) == z[r, b].view(torch.int32) and int(want[r]) == a
    assert float(z[6, v]) > float(z[6, :v].max()) and int(want[6]) == v - 1
    assert 0.15 < float((z[7, :v] == -100000.0).double().mean()) < 0.25 and float(z[8, :v].abs().max()) > 1e4
    assert int((z[9, :v] != -100000.0).sum()) == 1 and int(labels[9]) == int(want[9])
    gap = lc.top_two_gap(lc.ce_stride()[0], lc.CE_STRIDE["v"])
    assert bool((gap >= 1e-3).all())


def test_distance_tables_switch_the_vector_path_off_one_term_at_a_time():
    table = lc.dist_cases()
    assert {(c["e"], c["kind"], c["sd"]) for c in table} >= {(e, k, s) for e in lc.DIST_E for k in (0, 1, 2) for s in lc.DT}
    for kind in (0, 1, 2):                                                          # both kernels of every kind and type WITH the 4-element accesses, over one and several passes
        for sd in lc.DT:
            on = {c["e"] for c in table if c["kind"] == kind and c["sd"] == sd and lc.dist_vec_ok(c, True)}
            assert on >= set(lc.DIST_VECTOR_E) and any(e > 256 and e % 4 for e in on) and any(4 < e <= 256 for e in on), (kind, sd, on)
            assert {c["e"] for c in table if c["kind"] == kind and c["sd"] == sd and not lc.dist_vec_ok(c, False)}, (kind, sd)
    term_of = dict(pred_shift="pred", ld_pred="ld_pred", src_shift1="src", src_shift2="src", src_shift3="src", ld_src="ld_src", col0_1="col0", col0_2="col0", col0_3="col0",
                   dpred_shift="dpred", ld_dpred="ld_dpred")
    seen = set()
    for c in table:
        terms = lc.dist_vec_terms(c)
        off = {k for k, ok in terms.items() if not ok}
        assert off == ({term_of[c["switch"]]} if c["switch"] != "none" else set()), (c, terms)      # each ALONE
        rows_ok = all(ok for k, ok in terms.items() if k not in ("dpred", "ld_dpred"))
        assert lc.dist_vec_ok(c, False) == rows_ok and lc.dist_vec_ok(c, True) == (not off)
        assert c["ld_pred"] >= c["e"] and c["ld_dpred"] >= c["e"] and c["col0"] + c["e"] <= c["ld_src"]
        seen.add((c["switch"], c["sd"]))
    assert seen == {(s, t) for s in lc.DIST_SWITCHES for t in lc.DT}
    assert {c["n"] for c in table} == set(lc.DIST_N) and {c["ids64"] for c in table} == {True, False} and {c["ids_stride"] for c in table} == {1, 3}
    assert {(c["ids64"], c["ids_stride"]) for c in table} == {(a, b) for a in (True, False) for b in (1, 3)} and {c["mask"] for c in table} == set(lc.DIST_MASKS)
    assert {lc.dist_depth(e, True) for e in lc.DIST_E} == {7, 9, 10, 12, 19, 21} and lc.dist_depth(1028, False) == 17 + 6


def test_every_grid_cap_is_exceeded_once():
    assert lc.CE_STRIDE["rows"] > 65536                                              # ce_rows: min(rows, 65 536) workgroups
    assert (cases.ADDEND_STRIDE[1] + 255) // 256 > 2048                              # ce_addend
    assert (cases.SCALE_STRIDE + 1023) // 1024 > 2048 and cases.SCALE_STRIDE % 4     # ce_scale (and a ragged end)
    assert (cases.CAST_STRIDE[0] * cases.CAST_STRIDE[2] + 255) // 256 > 2048 * 4     # cast_kernel
    assert (lc.DIST_STRIDE["n"] + 3) // 4 > 2048                                     # dist_rows_kernel, dist_grad_kernel
    assert (cases.MASK_STRIDE + 255) // 256 > 2048                                   # single_token_mask_kernel
    assert lc.mt_items(lc.MT_STRIDE_N) > lc.MT_GRID and lc.MT_STRIDE_N % lc.MT_CHUNK == 5      # sumsq_kernel, adamw_kernel: the item stride
    assert lc.MT_CHUNK - lc.MT_PATTERN == -1                                         # every chunk starts at another phase of the pattern
    assert max(cases.FINALIZE_N) > 256 and {255, 256, 257} <= set(cases.FINALIZE_N)


def test_the_tensor_list_crosses_the_launch_boundary_with_empties():
    entries = lc.mt_list()
    lengths = [en["n"] for en in entries]
    assert len(entries) == 130 and set(lengths) == set(lc.MT_LENGTHS)
    assert all(lengths[i] == 0 for i in (0, 63, 64, 65, 129))
    launches = lc.mt_launches(lengths)
    assert len(launches) == 2 and len(launches[0][2]) == lc.MT_GROUP and launches[0][1] - launches[0][0] > lc.MT_GROUP      # 64 tensors with elements span more than 64 entries
    assert launches[1][0] == launches[0][1] and launches[1][2][-1] < 129
    assert [len(lc.mt_launches(lengths[:k])) for k in lc.MT_PREFIXES] == [0, 0, 1, 1, 1, 2]
    assert sum(launches[0][3:]) + launches[1][3] == sum(lc.mt_items(n) for n in lengths)
    assert {en["flags"] for en in entries} == {0, lc.DECAY, lc.FROZEN} and any(en["null"] for en in entries) and all(en["flags"] == lc.FROZEN for en in entries if en["null"])
    assert {en["off"][1] for en in entries} == {0, 1, 2, 3}
    alone = sorted(en["off"] for en in entries if len(set(en["off"])) > 1)
    assert alone == [(0, 0, 0, 1), (0, 0, 1, 0), (0, 1, 0, 0), (1, 0, 0, 0)]            # each of the four pointers alone off 16 bytes
    assert all(not (en["flags"] & lc.FROZEN) and en["n"] >= 1024 for en in entries if len(set(en["off"])) > 1)
    multi = [en for en in entries if en["n"] > lc.MT_CHUNK and not en["flags"] & lc.FROZEN]
    assert {all(o % 4 == 0 for o in en["off"]) for en in multi} == {True, False}        # several chunks on the vector and on the scalar path
    assert lc.sumsq_depth(True) == 64 + 2 + 6 + 2 and lc.sumsq_depth(False) == 256 + 2 + 6 + 2
