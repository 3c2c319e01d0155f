"""pair_qkv_kernel (zett_amd/csrc/rowops.hip.h) one launch at a time through zett_op_fwd_pair_qkv, ELEMENT BY ELEMENT against float64
on the same values (tests/id_qkv_check.py: the bound is the fp32 bound of the kernel's five operations on the float64 intermediates
plus half an ulp of the output type).  Buffers are framed as in tests/test_rowops_direct_gpu.py: NaN slack around every input, a
canary around the output, so a fetch or a store outside an operand shows; index arrays are always valid.

Shapes: H = 128 (3H = 384 columns: less than one 2048-column block) and H = 704 (2112: one full block and a partial one); 1, 7 and
300 rows; 6 table slots referenced out of order; positions 0..8 (the kernel keeps the first 8 positions' rows of C in LDS and reads
the ninth from memory); f16 and bf16; pair rows (written in place) and buffer rows of a chunk in the middle of a plan (position 0 of
a vocabulary row first; at 300 rows the position-0 block is permuted through cls_slot as well).  From 7 rows on, one row is scaled
beyond the f16 range: f16 stores infinities there and sets ZETT_RANGE_ACTIVATION's bit, bf16 holds the values and sets nothing."""
import ctypes as C

import pytest
import torch

from tests import id_qkv_check as ic
from tests import rowops_check as rc
from tests.test_rowops_direct_gpu import DEV, NULL, _lib, _prec, _stream, done, idx, inp, iptr, ok, outp

gpu = pytest.mark.gpu
F32 = torch.float32
LO = {"f16": torch.float16, "bf16": torch.bfloat16}
SLOTS, N_POS = 6, 9
ROW0, TOK0 = 2, 5
LENGTHS = {1: (1,), 7: (3, 1, 2, 1), 300: tuple(range(1, 10)) * 6 + (9, 8, 7, 6)}
OVERFLOW_ROW = 3

CASES = [dict(h=h, n=n, prec=prec, buffer=buffer) for h in (128, 704) for n in (1, 7, 300) for prec in ("f16", "bf16") for buffer in (False, True)]


def case_id(c):
    return f"h{c['h']}-n{c['n']}-{c['prec']}-{'buffer' if c['buffer'] else 'pair'}"


def make_values(case):
    """CPU tensors of one case.  slot / pos / stats and the reference are in the order of the kernel's row index j; buffer rows
    carry the plan and `brow`, the buffer row of every j."""
    n, cols, lo = case["n"], 3 * case["h"], LO[case["prec"]]
    g = torch.Generator().manual_seed(7000 + 13 * n + case["h"])
    v = dict(u=torch.randn(SLOTS, cols, generator=g).to(lo), c_pos=0.3 * torch.randn(N_POS, cols, generator=g), c_w=torch.randn(cols, generator=g),
             b_q=torch.randn(cols, generator=g))
    stats = torch.stack([0.1 * torch.randn(n, generator=g), 0.5 + torch.rand(n, generator=g)], 1)
    if n >= 7:
        stats[OVERFLOW_ROW, 1] = 3.0e5
    v["stats"] = stats
    order = [(5 * i + 3) % SLOTS for i in range(n)]          # 3 2 1 0 5 4 ...: never ascending
    if not case["buffer"]:
        v["slot"] = torch.tensor(order, dtype=torch.int32)
        v["pos"] = torch.tensor([(7 * i + 8) % N_POS for i in range(n)], dtype=torch.int32)
        return v
    lengths, at, slots = LENGTHS[n], 0, []
    for L in lengths:
        slots.append(order[at:at + L])
        at += L
    plan = rc.make_plan(lengths, row0=ROW0, tok0=TOK0, slots=slots)
    assert plan["m"] == n
    brow = plan["brow"]
    if n == 300:
        perm = torch.randperm(plan["rows"], generator=g)
        v["cls_slot"] = perm.to(torch.int32)
        brow = torch.where(brow < plan["rows"], perm[brow.clamp_max(plan["rows"] - 1)], brow)
    v.update(plan=plan, brow=brow, slot=plan["tok_slot"][TOK0:], pos=plan["tok_pos"][TOK0:])
    return v


@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_pair_qkv(case):
    _, lib = _lib()
    v = make_values(case)
    n, cols, lo = case["n"], 3 * case["h"], LO[case["prec"]]
    ld_out = cols + 8
    u, c_pos, c_w, b_q = inp(v["u"]), inp(v["c_pos"]), inp(v["c_w"]), inp(v["b_q"])
    out = outp(n, cols, lo, ld_out)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    if case["buffer"]:
        plan, brow = v["plan"], v["brow"]
        stats = inp(rc.to_buffer(v["stats"], brow))
        slot, pos, tok_row, row_offset = idx(plan["tok_slot"]), idx(plan["tok_pos"]), idx(plan["tok_row"]), idx(plan["row_offset"])
        cls_slot = idx(v["cls_slot"]) if "cls_slot" in v else None
        args = (TOK0, n, iptr(tok_row), iptr(row_offset), ROW0, plan["rows"], iptr(cls_slot))
    else:
        stats = inp(v["stats"])
        slot, pos = idx(v["slot"]), idx(v["pos"])
        args = (0, n, NULL, NULL, 0, 0, NULL)
    ok(lib.zett_op_fwd_pair_qkv(_prec(case["prec"]), u.p, iptr(slot), iptr(pos), *args, stats.p, c_pos.p, N_POS, c_w.p, b_q.p, cols, out.p, ld_out,
                                iptr(word), _stream()), lib)
    torch.cuda.synchronize()
    # (the canary check also asks for finite values inside: not where this case stores infinities — check_pair_qkv then holds every
    #  other element, an unwritten one included, to its bound)
    got = done(out, f"pair_qkv {case}", partial=case["prec"] == "f16" and n >= 7)
    if case["buffer"]:
        got = rc.from_buffer(got, v["brow"])
    x = ic.pair_qkv_ref(v["u"], v["slot"], v["pos"], v["stats"], v["c_pos"], v["c_w"], v["b_q"])
    over = ic.check_pair_qkv(f"pair_qkv {case}", got, x, lo, key=("fwd_pair_qkv", case["prec"]))
    assert over == (case["prec"] == "f16" and n >= 7)
    assert int(word.cpu()[0]) == (ic.RANGE_ACTIVATION if over else 0)


@gpu
def test_pair_qkv_refusals():
    """every argument is validated before a launch: ZETT_E_INVALID with a text, nothing written"""
    L, lib = _lib()
    v = make_values(dict(h=128, n=7, prec="f16", buffer=False))
    u, c_pos, c_w, b_q, stats = inp(v["u"]), inp(v["c_pos"]), inp(v["c_w"]), inp(v["b_q"]), inp(v["stats"])
    out = outp(7, 384, torch.float16)
    slot, pos = idx(v["slot"]), idx(v["pos"])

    def call(prec=L.PREC_F16, u_=u.p, cols=384, ld=384, n_pos=N_POS, tok_row=NULL, cls=NULL):
        return lib.zett_op_fwd_pair_qkv(prec, u_, iptr(slot), iptr(pos), 0, 7, tok_row, NULL, 0, 0, cls, stats.p, c_pos.p, n_pos, c_w.p, b_q.p, cols, out.p, ld, NULL,
                                        _stream())
    for bad in (call(prec=L.PREC_F32), call(prec=77), call(u_=NULL), call(cols=380), call(ld=376), call(n_pos=0), call(tok_row=iptr(slot)), call(cls=iptr(slot)),
                call(u_=C.c_void_p(u.p.value + 2))):
        assert bad == L.E_INVALID and lib.zett_last_error()
    torch.cuda.synchronize()
    done(out, "refused launches", partial=True)
    assert not bool(torch.isfinite(out.view().float()).any())
