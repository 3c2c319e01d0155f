"""The forward's row kernels (zett_amd/csrc/rowops.hip.h) called one launch at a time through zett_op_fwd_* and checked ELEMENT BY
ELEMENT against float64 on the same values (tests/rowops_check.py), at the layout edges the whole-model tests cannot see: every
LayerNorm kernel and lane count (the re-read loops past 8192 columns included), every branch of the attention's head sum, packed
narrow last groups with lane groups past the last row, rows longer than a lane group with and without pair slots, the online-softmax
loop on 16-bit operands, a non-uniform row whose position 0 is no key, the tails of ln_stats, gather_src's second loop trip and the
readout's row map.  The entry points go through the launchers the forward calls (csrc/rowops_launch.hip.h), so a case here is a
launch the forward would make for the same width and options.

Buffers: every floating-point operand is a view INSIDE a larger allocation of this test (gemm_check.Framed / train_ops_check.Frame):
256 rows of its leading dimension (256 elements for a vector) in front of and behind it.  What that slack is for: the slack of an
input is NaN, so a value fetched from outside the operand poisons the result; the slack of an output — rows past `rows`, columns past
the width — is a canary bit pattern, so a store outside the output breaks it and an element that was not written is not finite.  A
one-tile overrun therefore stays inside this test's memory and SHOWS.  Index arrays are always valid.  Nothing here is meant to fault.

The case tables are module constants without a GPU in them; tests/test_rowops_check_host.py runs the emulation over the same tables.
"""
import ctypes as C

import pytest
import torch

from tests import rowops_check as rc
from tests import train_ops_check as tc

DEV = "cuda:0"
gpu = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
PRECS = ("f32", "bf16", "f16")
NULL = C.c_void_p(0)

# ---- case tables (no GPU) ------------------------------------------------------------------------------------------------
# LayerNorm widths by the kernel a 16-bit launch with ln_rows8 goes to; with ln_rows8 off or in f32 the rows8 widths take the wave kernel.
# rows8: 1 ... 4 vectors of 8 columns per lane on 32 lanes (256 ... 1024), 3 and 4 on 64 (a width with 1 or 2 there takes 32 lanes)
LN_WIDTHS = {"rows8_32": (256, 512, 768, 1024), "rows8_64": (1536, 2048), "wave": (64, 320, 1280), "workgroup": (2112, 8192, 8256)}
LN_H = tuple(h for k in rc.LN_KERNELS for h in LN_WIDTHS[k])
LN_ROWS = (1, 7, 8, 9, 13)
LN_REREAD_H = 8256                       # the smallest width past LN_MAX_VEC * 256 * 4 columns: the re-read loops
LN_OUTPUTS = (("out_f32", "out_lo", "stats"), ("out_lo",), ("out_f32",), ("out_lo", "stats"))
EPS_ENC, EPS_PROJ = 1e-5, 1e-6


def ln_kernel_expected(h, prec, ln_rows8):
    for name, hs in LN_WIDTHS.items():
        if h in hs:
            if name.startswith("rows8") and (prec == "f32" or not ln_rows8):
                return "wave"
            return name
    raise KeyError(h)


def ln_cases(h):
    """every precision x ln_rows8 (both where it matters) of width h; the row counts, the optional outputs and the input kinds cycle along
    the table, and LN_ROWS runs in full at the first width of every kernel"""
    out, i = [], LN_H.index(h)
    full = any(h == hs[0] for hs in LN_WIDTHS.values())
    for prec in PRECS:
        for ln8 in ((1, 0) if (prec != "f32" and ln_kernel_expected(h, prec, 1).startswith("rows8")) else (1,)):
            for rows in (LN_ROWS if (full and prec != "f16") else (LN_ROWS[i % 5],)):
                out.append(dict(h=h, prec=prec, ln8=ln8, rows=rows, outputs=LN_OUTPUTS[i % 4], kind=i % 3, seed=i))
                i += 1
    return out


def ln_inputs(case):
    """x [rows, h], gamma (zeros and negatives), beta.  kind 1: a row mean large against the spread; rows >= 7: the last row has zero variance"""
    g = torch.Generator().manual_seed(50 + case["seed"])
    rows, h = case["rows"], case["h"]
    x = torch.randn(rows, h, generator=g)
    if case["kind"] == 1:
        x = 100.0 + 0.01 * x
    if rows >= 7:
        x[-1] = 0.5
    gamma = torch.randn(h, generator=g)
    gamma[::7] = 0.0
    return x, gamma, 0.1 * torch.randn(h, generator=g)


READOUT_H = (256, 1536, 320, 2112, LN_REREAD_H)
READOUT_DESTS = (None, "f32", "f16", "bf16")          # None: the fp32 store without a map (bias_dtype -1)
EMBED_H = (256, 768, 1536, 64, 1280, 2112, LN_REREAD_H)
EMBED_LENGTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9)
EMBED_TABLE_ROWS = 6

# attention: (H, head_dim)
ATT_SHAPES = ((64, 8), (64, 16), (128, 32), (64, 64), (128, 128), (256, 256), (512, 512),      # every branch of head_sum
              (1024, 64),                                                                    # two full groups
              (320, 64),                                                                     # a partial group that cannot be packed
              (768, 64), (640, 64), (576, 64), (1088, 64),                                   # packed groups of 2, 4, 8, 8 rows per wave
              (768, 256), (640, 128))                                                        # a head that fills the lane group
# row sets: lengths, uniform rows, rows whose position 0 is no key.  9 / 5 / 1 rows: lane groups past the last row, wave counts off 4
ATT_ROWSETS = (dict(lengths=(1, 2, 3, 4, 5, 6, 7, 8, 9), uniform=(2,), pad0=(4, 8), subnormal_k=5, subnormal_q=6),
               dict(lengths=(12, 70, 3, 8, 1), uniform=(), pad0=(0,)),
               dict(lengths=(5,), uniform=(), pad0=()))


def att_plan(rs, row0, tok0):
    keys = []
    for r, L in enumerate(rs["lengths"]):
        k = [1] * L
        if r in rs["uniform"]:
            k = [0] * L
        elif r in rs["pad0"] and L > 1:
            k[0] = 0
        keys.append(k)
    return rc.make_plan(rs["lengths"], keys=keys, uniform=[int(r in rs["uniform"]) for r in range(len(rs["lengths"]))], row0=row0, tok0=tok0)


def att_values(plan, rs, h, lo, by_pair, cls_only, seed):
    """q / k / v in the operand type.  by_pair: one row per (slot, position) pair, so positions that share a pair share their values.
    -> (q_store, kv_store [*, 2h], q_plan, k_plan, v_plan): the stored matrices (buffer order or pair order; q [rows, h] with cls_only)
    and the same values in plan order.  The f16 subnormal rows: every k (or q) of the row is an f16 subnormal, the other operand large."""
    g = torch.Generator().manual_seed(seed)
    m, rows, tok0 = plan["m"], plan["rows"], plan["tok0"]
    n = plan["n_pairs"] if by_pair else m
    q, k, v = (torch.randn(n, h, generator=g) for _ in range(3))
    idx = plan["tok_pair"][tok0:].long() if by_pair else torch.arange(m)
    if not by_pair:          # (pair rows are shared between vocabulary rows: the special rows keep to the unshared layout)
        sub = lambda shape: (torch.randint(1, 1024, shape, generator=g).float() * 2.0 ** -24) * (torch.randint(0, 2, shape, generator=g).float() * 2 - 1)
        for name, big, small in (("subnormal_k", q, k), ("subnormal_q", k, q)):
            if name in rs:
                t0, t1 = plan["offs"][rs[name]], plan["offs"][rs[name] + 1]
                small[t0:t1] = sub((t1 - t0, h))
                big[t0:t1] *= 8192.0
    q, k, v = q.to(lo), k.to(lo), v.to(lo)
    q_plan, k_plan, v_plan = q[idx], k[idx], v[idx]
    if cls_only:
        q_plan = q_plan[[plan["offs"][r] for r in range(rows)]]
        q_store = q_plan
    else:
        q_store = q if by_pair else rc.to_buffer(q_plan, plan["brow"])
    k_store, v_store = (k, v) if by_pair else (rc.to_buffer(k_plan, plan["brow"]), rc.to_buffer(v_plan, plan["brow"]))
    return q_store, torch.cat([k_store, v_store], 1), q_plan, k_plan, v_plan


GATHER_E = (64, 1024, 1088, 2112)
GATHER_V0, GATHER_FB, GATHER_SLOT0 = 11, 4, 3
GATHER_IDS = (5, 0, 9, GATHER_V0 - 1, GATHER_V0, GATHER_V0 + GATHER_FB - 1, 2, GATHER_V0 + 1, 10, 7)          # the first GATHER_SLOT0 are in front of the launch
STATS_PARTS = (1, 7, 8, 9, 16, 33)
STATS_ROWS = (1, 63, 64, 65)
FOLD_K = (64, 256, 320, 2112)
FOLD_N = 3


# ---- plumbing ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = rc.record_path()          # figures for profiles/rowops_check.md
    if path:
        rc.write_record(path)


def _lib():
    from zett_amd import _lib
    return _lib, _lib.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def _prec(kind):
    L, _ = _lib()
    return {"f32": L.PREC_F32, "bf16": L.PREC_BF16, "f16": L.PREC_F16}[kind]


def _dtype_code(kind):
    return {"f32": 0, "f16": 1, "bf16": 2}[kind]


class Op:
    """a Frame on the device: .t the whole allocation, .p the pointer of the view"""

    def __init__(self, frame):
        self.f, self.t = frame, frame.buf.to(DEV)
        self.p = C.c_void_p(self.t.data_ptr() + frame.byte_offset())

    def back(self):
        return self.t.cpu()

    def view(self):
        return self.f.view(self.back())


def inp(values, ld=None, shift=0):
    values = values.contiguous()
    if values.dim() == 1:
        return Op(tc.Frame(None, values.shape[0], values.shape[0], values.dtype, float("nan"), shift=shift, values=values))
    return Op(tc.Frame(values.shape[0], values.shape[1], ld or values.shape[1], values.dtype, float("nan"), shift=shift, values=values))


def outp(rows, cols, dtype, ld=None):
    return Op(tc.Frame(rows, cols, ld or cols, dtype, "canary"))


def idx(t):
    return t.to(DEV)


def iptr(t):
    return NULL if t is None else C.c_void_p(t.data_ptr())


def ok(rc_, lib):
    assert rc_ == 0, lib.zett_last_error().decode()


def done(op, what, partial=False):
    """after the synchronize: the canary intact around the output (and, unless partial, every element inside written) -> the view"""
    buf = op.back()
    (tc.check_slack if partial else tc.check_canary)(op.f, buf, what)
    return op.f.view(buf)


def run_layernorm(lib, prec, h, rows, eps, ln8, gamma, beta, x=None, x_lo=None, ld_in=None, outputs=("out_f32", "out_lo", "stats"), readout=None):
    """one zett_op_fwd_layernorm launch -> (kernel name, dict of the outputs' views, the destination vector or None, range word)"""
    lo = rc.DT[prec]
    src = inp(x, ld_in) if x is not None else None
    src_lo = inp(x_lo, ld_in) if x_lo is not None else None
    g, b = inp(gamma), inp(beta)
    o32 = outp(rows, h, F32) if "out_f32" in outputs else None
    olo = outp(rows, h, lo) if "out_lo" in outputs else None
    st = outp(rows, 2, F32) if "stats" in outputs else None
    bw = bb = dest = rows_map = None
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    code = -1
    if readout is not None:
        bw = inp(readout["bias_w"]) if readout.get("bias_w") is not None else None
        bb = inp(readout["bias_b"].repeat(4)) if readout.get("bias_b") is not None else None
        dd = readout.get("dest")
        code = -1 if dd is None else _dtype_code(dd)
        dest = outp(None, readout["n_dest"], rc.DT[dd or "f32"])
        rows_map = idx(readout["bias_rows"]) if readout.get("bias_rows") is not None else None
    kid = C.c_int32(-7)
    p = lambda o: NULL if o is None else o.p
    ok(lib.zett_op_fwd_layernorm(_prec(prec), p(src), p(src_lo), ld_in or h, rows, h, g.p, b.p, eps, ln8, p(o32), p(olo), p(st), p(bw), p(bb), p(dest),
                                 iptr(rows_map), code, iptr(word), C.byref(kid), _stream()), lib)
    torch.cuda.synchronize()
    what = f"layernorm h={h} rows={rows} {prec} ln8={ln8}"
    got = {name: done(o, f"{what} {name}") for name, o in (("out_f32", o32), ("out_lo", olo), ("stats", st)) if o is not None}
    dvec = done(dest, what + " out_bias", partial=True) if dest is not None else None
    return rc.LN_KERNELS[kid.value], got, dvec, int(word.cpu()[0])


# ---- LayerNorm -----------------------------------------------------------------------------------------------------------
def test_ln_tables_reach_every_kernel():
    """(no GPU) the widths reach all four kernels in the 16-bit modes and both float4 kernels in f32"""
    for prec in ("bf16", "f16"):
        assert {ln_kernel_expected(h, prec, 1) for h in LN_H} == set(rc.LN_KERNELS)
    assert {ln_kernel_expected(h, "f32", 1) for h in LN_H} == {"wave", "workgroup"}
    assert {c["rows"] for h in LN_H for c in ln_cases(h)} == set(LN_ROWS) and LN_REREAD_H in LN_H and LN_REREAD_H > 8192


@gpu
@pytest.mark.parametrize("h", LN_H)
def test_layernorm_plain(h):
    _, lib = _lib()
    for case in ln_cases(h):
        x, gamma, beta = ln_inputs(case)
        prec, rows = case["prec"], case["rows"]
        kernel, got, _, word = run_layernorm(lib, prec, h, rows, EPS_ENC, case["ln8"], gamma, beta, x=x, ld_in=h + 8 * (case["seed"] % 2), outputs=case["outputs"])
        assert kernel == ln_kernel_expected(h, prec, case["ln8"]), (case, kernel)
        assert word == 0
        exp = rc.ln_expect(x, gamma, beta, EPS_ENC, rc.DT[prec])
        rc.check_layernorm(f"layernorm {case}", exp, key=("fwd_layernorm", f"{kernel}/{prec}"), **got)


@gpu
@pytest.mark.parametrize("h", READOUT_H)
def test_layernorm_readout(h):
    """the readout instantiations: rows from in (fp32) or in_lo (exact 16-bit values), the bias head with and without weights, the fp32
    store and the three destination types, the row map null / a permutation / with skipped rows"""
    _, lib = _lib()
    i = READOUT_H.index(h)
    for j, prec in enumerate(PRECS):
        lo = rc.DT[prec]
        for d, dest in enumerate(READOUT_DESTS):
            n = i + j + d
            rows = LN_ROWS[n % 5]
            case = dict(h=h, rows=rows, kind=n % 3, seed=200 + n, prec=prec, dest=dest)
            x, gamma, beta = ln_inputs(case)
            use_lo = prec != "f32" and (n % 2 == 0 or h == LN_REREAD_H)
            x_lo = x.to(lo) if use_lo else None
            g = torch.Generator().manual_seed(300 + n)
            bias_w = None if (d == 1 and j == 0) else torch.randn(h, generator=g) / h ** 0.5
            bias_b = torch.tensor([0.25])
            n_dest = rows + 3
            mode = (n // 2) % 3 if dest is not None else 0          # 0: no map, 1: a permutation into the destination, 2: with skipped rows
            rows_map = None
            if mode:
                rows_map = (torch.randperm(n_dest, generator=g)[:rows]).to(torch.int64)
                if mode == 2:
                    rows_map[::2] = -1
            ro = dict(bias_w=bias_w, bias_b=bias_b, dest=dest, n_dest=n_dest, bias_rows=rows_map)
            outputs = ("out_f32", "out_lo") if dest is not None else LN_OUTPUTS[n % 4]
            kernel, got, dvec, word = run_layernorm(lib, prec, h, rows, EPS_PROJ, 1, gamma, beta, x=None if use_lo else x, x_lo=x_lo, ld_in=h + 8,
                                                    outputs=outputs, readout=ro)
            assert kernel == ln_kernel_expected(h, prec, 1) and word == 0, (case, kernel, word)
            exp = rc.ln_expect(x_lo if use_lo else x, gamma, beta, EPS_PROJ, lo)
            what = f"readout {case} in_lo={use_lo} map={mode}"
            rc.check_layernorm(what, exp, key=("fwd_readout", f"{kernel}/{prec}"), **got)
            ref, bnd = rc.readout_expect(exp, bias_w, bias_b, rc.DT[dest] if dest else None)
            if bias_w is None:
                assert bool((bnd == 0).all())
            rc.check_readout(what, ref, bnd, dvec, rows_map, key=("fwd_readout_bias", f"{kernel}/{prec}/{dest or 'f32 store'}"))


@gpu
def test_layernorm_readout_reports_a_bias_beyond_the_f16_destination():
    """a finite bias past 65504 in an f16 destination: stored as inf, ZETT_RANGE_DEST's bit set — and only then (every other case asserts 0)"""
    _, lib = _lib()
    h, rows = 256, 7
    x, gamma, beta = ln_inputs(dict(h=h, rows=rows, kind=0, seed=400))
    bias_w, bias_b = torch.randn(h, generator=torch.Generator().manual_seed(5)) / 16, torch.tensor([1.0e5])
    ro = dict(bias_w=bias_w, bias_b=bias_b, dest="f16", n_dest=rows, bias_rows=None)
    kernel, got, dvec, word = run_layernorm(lib, "bf16", h, rows, EPS_PROJ, 1, gamma, beta, x=x, outputs=("out_f32",), readout=ro)
    assert word == rc.RANGE_DEST, word
    exp = rc.ln_expect(x, gamma, beta, EPS_PROJ, torch.bfloat16)
    ref, bnd = rc.readout_expect(exp, bias_w, bias_b, torch.float16)
    assert bool(ref.to(torch.float16).isinf().all())
    rc.check_readout("readout overflow", ref, bnd, dvec, None)


def embed_case(h, prec, variant, seed):
    """variant 0: fp32 table, language token, a chunk in the middle of a plan; 1: the 16-bit table (16-bit modes), no language token;
    2: pair rows in place (tok_row null), language token"""
    g = torch.Generator().manual_seed(seed)
    lo = rc.DT[prec]
    lang = variant != 1
    slots = []
    for L in EMBED_LENGTHS:
        s = torch.randint(0, EMBED_TABLE_ROWS, (L,), generator=g).tolist()
        if lang and L >= 2:
            s[-1] = -1
        slots.append(s)
    row0, tok0 = (3, 10) if variant == 0 else (0, 0)
    plan = rc.make_plan(EMBED_LENGTHS, slots=slots, row0=row0, tok0=tok0)
    if lang:          # the language token sits at position lang_pos in every row that has it
        pos = plan["tok_pos"].clone()
        pos[plan["tok_slot"] < 0] = max(EMBED_LENGTHS)
        plan["tok_pos"] = pos
    e = dict(tok_slot=plan["tok_slot"][tok0:], tok_pos=plan["tok_pos"][tok0:], type0=0.1 * torch.randn(h, generator=g),
             pos_emb=0.1 * torch.randn(max(EMBED_LENGTHS) + 2, h, generator=g), lang=torch.randn(h, generator=g) if lang else None, lang_pos=max(EMBED_LENGTHS))
    if variant == 1 and prec != "f32":
        raw = 3.0 + 2.0 * torch.randn(EMBED_TABLE_ROWS, h, generator=g)
        e.update(table_lo=raw.to(lo), table_stats=torch.stack([raw.mean(1), 1.0 / raw.std(1)], 1).contiguous(), table_gamma=torch.randn(h, generator=g),
                 table_beta=0.1 * torch.randn(h, generator=g))
    else:
        e["table"] = torch.randn(EMBED_TABLE_ROWS, h, generator=g)
    gamma = torch.randn(h, generator=g)
    gamma[::5] = 0.0
    return plan, e, gamma, 0.1 * torch.randn(h, generator=g)


def run_embed(lib, prec, h, plan, e, gamma, beta, ln8, in_place, with_sum=True):
    lo, m = rc.DT[prec], plan["m"]
    ops = {k: inp(e[k]) for k in ("table", "table_lo", "table_stats", "table_gamma", "table_beta", "type0", "pos_emb", "lang") if e.get(k) is not None}
    p = lambda k: ops[k].p if k in ops else NULL
    g, b = inp(gamma), inp(beta)
    slot, pos, trow, roff = idx(plan["tok_slot"]), idx(plan["tok_pos"]), idx(plan["tok_row"]), idx(plan["row_offset"])
    olo, st, sm = outp(m, h, lo), outp(m, 2, F32), outp(m, h, F32) if with_sum else None
    kid = C.c_int32(-7)
    ok(lib.zett_op_fwd_embed_layernorm(_prec(prec), p("table"), p("table_lo"), p("table_stats"), p("table_gamma"), p("table_beta"), iptr(slot), iptr(pos),
                                       p("type0"), p("pos_emb"), p("lang"), e["lang_pos"], NULL if in_place else iptr(trow), NULL if in_place else iptr(roff),
                                       plan["row0"], plan["rows"], plan["tok0"], m, h, g.p, b.p, EPS_ENC, ln8, olo.p, st.p, NULL if sm is None else sm.p,
                                       C.byref(kid), _stream()), lib)
    torch.cuda.synchronize()
    what = f"embed layernorm h={h} {prec}"
    return rc.LN_KERNELS[kid.value], done(olo, what + " out_lo"), done(st, what + " stats"), None if sm is None else done(sm, what + " sum")


@gpu
@pytest.mark.parametrize("h", EMBED_H)
def test_layernorm_embed(h):
    """position 0 first over rows of 1 to 9 positions, the language token present and absent, fp32 and 16-bit tables, pair rows in place,
    tok0 and row0 nonzero; two stages (rowops_check.check_embed); one run without `sum` must give the other outputs bit for bit"""
    _, lib = _lib()
    for j, prec in enumerate(PRECS):
        for variant in (0, 1, 2):
            if h == LN_REREAD_H and not (variant == 1 and prec != "f32"):
                continue          # (the re-read width runs the 16-bit table, once per 16-bit mode)
            plan, e, gamma, beta = embed_case(h, prec, variant, 500 + 10 * j + variant)
            in_place = variant == 2
            ln8 = 0 if (variant == 2 and prec == "bf16") else 1
            kernel, olo, st, sm = run_embed(lib, prec, h, plan, e, gamma, beta, ln8, in_place)
            assert kernel == ln_kernel_expected(h, prec, ln8), (h, prec, variant, kernel)
            brow = torch.arange(plan["m"]) if in_place else plan["brow"]
            rc.check_embed(f"embed h={h} {prec} variant {variant}", e, brow, EPS_ENC, gamma, beta, sm, olo, st, rc.DT[prec],
                           key=("fwd_embed_layernorm", f"{kernel}/{prec}"))
            if variant == 0:
                _, olo2, st2, _ = run_embed(lib, prec, h, plan, e, gamma, beta, ln8, in_place, with_sum=False)
                tc.exact(olo2, olo, "embed out_lo without sum")
                tc.exact(st2, st, "embed stats without sum")


# ---- attention -------------------------------------------------------------------------------------------------------------
def run_attention(lib, prec, h, hd, plan, q_store, kv_store, cls_only, fast, pack, by_pair):
    lo = rc.DT[prec]
    ldq = h if cls_only else h + 8
    q, kv = inp(q_store, ldq), inp(kv_store, 2 * h + 8)
    out_rows = plan["rows"] if cls_only else plan["m"]
    ctx = outp(out_rows, h, lo)
    roff, runi, tkey, tpair = idx(plan["row_offset"]), idx(plan["row_uniform"]), idx(plan["tok_key"]), idx(plan["tok_pair"])
    vptr = C.c_void_p(kv.p.value + h * kv.t.element_size())
    flags = (1 if cls_only else 0) | (2 if fast else 0) | (4 if pack else 0)
    ok(lib.zett_op_fwd_attention(_prec(prec), q.p, ldq, kv.p, vptr, 2 * h + 8, h, hd, iptr(roff), iptr(runi), iptr(tkey), plan["row0"], plan["rows"], plan["tok0"],
                                 tc.att_scaling(hd), flags, iptr(tpair) if by_pair else NULL, ctx.p, _stream()), lib)
    torch.cuda.synchronize()
    return done(ctx, f"attention h={h} d={hd} {prec} flags={flags} pair={by_pair}")


@gpu
@pytest.mark.parametrize("h,hd", ATT_SHAPES)
def test_attention(h, hd):
    """fast and generic paths each inside their bound (rows of 1..8 positions, 9, 12 and 70), cls_only 0 and 1, with and without pair
    slots, chunks in the middle of a plan; pack on and off must give the same bits"""
    _, lib = _lib()
    heads = h // hd
    for j, prec in enumerate(PRECS):
        lo = rc.DT[prec]
        for s, rs in enumerate(ATT_ROWSETS):
            plan = att_plan(rs, *((2, 6) if (s + j) % 2 else (0, 0)))
            for cls_only in (0, 1):
                by_pair = s == 1 or ((s + j + cls_only) % 2 == 0 and not (s == 0 and prec == "f16"))          # (the long rows: with pair slots and, below, without; f16's subnormal rows: never shared)
                for pair in ((by_pair, False) if s == 1 and not cls_only else (by_pair,)):
                    q_store, kv_store, qp, kp, vp = att_values(plan, rs, h, lo, pair, cls_only, 700 + 10 * s + j)
                    variants = ((1, 1), (1, 0), (0, 1)) if prec != "f32" else ((0, 1), (0, 0))
                    got = {}
                    for fast, pack in variants:
                        ctx = run_attention(lib, prec, h, hd, plan, q_store, kv_store, cls_only, fast, pack, pair)
                        got[(fast, pack)] = ctx
                        if pack == 0:
                            tc.exact(ctx, got[(fast, 1)], f"attention h={h} d={hd} {prec}: pack off against pack on")
                            continue
                        exp = rc.attention_expect(plan, qp, kp, vp, heads, hd, bool(cls_only), bool(fast), lo)
                        ctx_plan = ctx if cls_only else rc.from_buffer(ctx, plan["brow"])
                        rc.check_attention(f"attention h={h} d={hd} {prec} rows={rs['lengths']} cls={cls_only} fast={fast} pair={pair}", plan, exp, ctx_plan,
                                           bool(cls_only), key=f"{prec}/d{hd}")


# ---- gather_src, ln_stats, fold_weight -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("e_in", GATHER_E)
def test_gather_src(e_in):
    """ids on both sides of v0 (v0 - 1 and v0 among them), slot0 > 0, every source and output type, with and without the rescaler; one
    source value beyond the f16 range sets ZETT_RANGE_SOURCE's bit in f16 mode and in no other"""
    _, lib = _lib()
    g = torch.Generator().manual_seed(900 + e_in)
    ids_all = torch.tensor(GATHER_IDS, dtype=torch.int32)
    ids = ids_all[GATHER_SLOT0:]
    fb = torch.randn(GATHER_FB, e_in, generator=g)
    sw, sb = 1.0 + 0.1 * torch.randn(e_in, generator=g), 0.1 * torch.randn(e_in, generator=g)
    for sdt in ("f32", "f16", "bf16"):
        for big in (False, True):
            src = torch.randn(GATHER_V0, e_in, generator=g)
            if big:
                src[2, e_in - 3] = 1.0e5 if sdt != "f16" else 65504.0          # (row 2 is gathered; an f16 source passes the limit through the rescaler)
            src = src.to(rc.DT[sdt])
            for prec in PRECS:
                for rescale in ((True,) if big else (False, True)):
                    s_op, f_op, o = inp(src), inp(fb), outp(len(ids), e_in, rc.DT[prec])
                    w_op, b_op = (inp(sw * (2.0 if big else 1.0)), inp(sb)) if rescale else (None, None)
                    word = torch.zeros(1, dtype=torch.int32, device=DEV)
                    il = idx(ids_all)
                    ok(lib.zett_op_fwd_gather_src(_prec(prec), iptr(il), GATHER_SLOT0, len(ids), s_op.p, _dtype_code(sdt), e_in, GATHER_V0, f_op.p,
                                                  w_op.p if rescale else NULL, b_op.p if rescale else NULL, o.p, iptr(word), _stream()), lib)
                    torch.cuda.synchronize()
                    what = f"gather_src e_in={e_in} src={sdt} out={prec} rescale={rescale} big={big}"
                    exp = rc.gather_expect(ids, src, GATHER_V0, fb, sw * (2.0 if big else 1.0) if rescale else None, sb if rescale else None, rc.DT[prec])
                    assert bool(exp["out_of_range"].any()) == big, what
                    rc.check_gather(what, exp, done(o, what, partial=big), int(word.cpu()[0]), prec, key=("fwd_gather_src", f"{sdt}->{prec}"))


def stats_parts(parts, rows, seed):
    """partials (sum, sum of squares) of real rows of 128 * parts columns, and row 0 made to cancel below zero: q one part in 2^16 short
    of h mean^2 -> the clamp"""
    g = torch.Generator().manual_seed(seed)
    x = (2.0 + torch.randn(rows, parts, 128, generator=g)).float()
    p = torch.stack([x.sum(2), (x * x).sum(2)], 2).permute(1, 0, 2).contiguous()          # [parts, rows, 2]
    p[:, 0, 0] = 128 * 1.5
    p[:, 0, 1] = 128 * 2.25 * (1.0 - 2.0 ** -16)
    return p


@gpu
@pytest.mark.parametrize("parts", STATS_PARTS)
def test_ln_stats(parts):
    _, lib = _lib()
    for rows in STATS_ROWS:
        p = stats_parts(parts, rows, 40 * parts + rows)
        ld = rows + 5
        po = inp(p.reshape(parts, rows * 2), ld * 2)
        st = outp(rows, 2, F32)
        ok(lib.zett_op_fwd_ln_stats(_prec("bf16"), po.p, ld, rows, 128 * parts, EPS_ENC, st.p, _stream()), lib)
        torch.cuda.synchronize()
        what = f"ln_stats parts={parts} rows={rows}"
        rc.check_ln_stats(what, p, 128 * parts, EPS_ENC, done(st, what), clamp_rows=(0,), key=("fwd_ln_stats", "f32"))


@gpu
@pytest.mark.parametrize("k", FOLD_K)
def test_fold_weight(k):
    _, lib = _lib()
    g = torch.Generator().manual_seed(60 + k)
    for prec in ("bf16", "f16"):
        for big in (False, True) if (prec == "f16" and k == FOLD_K[0]) else (False,):
            w, gamma, beta, bias = torch.randn(FOLD_N, k, generator=g), torch.randn(k, generator=g), torch.randn(k, generator=g), torch.randn(FOLD_N, generator=g)
            gamma[::9] = 0.0
            if big:
                w[1, 5], gamma[5] = 400.0, 300.0
            wo, go, bo, bi = inp(w), inp(gamma), inp(beta), inp(bias)
            wf, co, bp = outp(FOLD_N, k, rc.DT[prec]), outp(None, FOLD_N, F32), outp(None, FOLD_N, F32)
            word = torch.zeros(1, dtype=torch.int32, device=DEV)
            ok(lib.zett_op_fwd_fold_weight(_prec(prec), wo.p, FOLD_N, k, go.p, bo.p, bi.p, wf.p, co.p, bp.p, iptr(word), _stream()), lib)
            torch.cuda.synchronize()
            what = f"fold_weight k={k} {prec} big={big}"
            assert int(word.cpu()[0]) == (rc.RANGE_WEIGHT if big else 0), what
            ref = rc.fold_ref(w, gamma, beta, bias, rc.DT[prec])
            rc.check_fold(what, ref, done(wf, what, partial=big), done(co, what, partial=big), done(bp, what), rows=(0, 2) if big else None,
                          key=("fwd_fold_weight", prec))
