"""zett_op_fwd_gemm — ONE GEMM launch of the forward, through the forward's own variant rule and launchers — checked ELEMENT BY ELEMENT
against float64 on the same values (tests/gemm_fwd_check.py): every epilogue instantiation of gemm4d (the LayerNorm-fold producers and
consumers, LO, BOTH, F32, F32_SCALE, the generic drain), the destination stores, full and 128x256 HALF tiles, the 128x128, gemm8r and
384x256 tiles on the epilogues they carry, at the row / column / K counts where a tile, a 64-row pass, a 128-column slice or an LDS stage
starts and ends.

Buffers: every operand, vector, residual and statistic is a view INSIDE a larger allocation of this test (gemm_check.Framed) whose slack
is NaN — a value fetched from outside poisons the result —; every output sits in a canary frame (train_ops_check.Frame) — a store
outside it, or an element that was not written, shows.  For the 384-row tile, which does not clamp rows, A is followed by readable rows
up to ceil(m / 384) * 384 and a_rows_readable says so.  Index arrays are in range.  Nothing here is meant to fault.

The entry reports the variant and gemm4d's epilogue mode it ran; every case asserts them against the restated rule
(gemm_fwd_check.path_expected).  The case tables are module constants without a GPU in them; tests/test_gemm_fwd_check_host.py proves
what they reach and runs the emulation over them.
"""
import ctypes as C

import pytest
import torch

from tests import gemm_check as gc
from tests import gemm_fwd_check as fc
from tests import train_ops_check as tc

DEV = "cuda:0"
gpu = pytest.mark.gpu
F32 = torch.float32
KINDS16 = ("bf16", "f16")

# ---- case tables (no GPU) ------------------------------------------------------------------------------------------------------
MS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 513)
KS16 = (64, 128, 192, 576)          # one, two, three K steps (two / three LDS stages), nine
KS32 = (32, 96, 544)
N_PRODUCER, N_LO, N_FOUR, N_V3 = (128, 256, 384, 640), (8, 136, 264, 520), (132, 260), (256, 512)

# mode -> (the N of its sweep, its flavours: make_case keywords).  A flavour with split="mid" cuts the columns at 8 * (n // 16).
MODES = {
    "LO": (N_LO, (dict(out_lo=True), dict(out_lo=True, act=1), dict(out_lo=True, act=2, bias=False))),
    "F32": (N_LO + N_FOUR, (dict(out_f32=True), dict(out_f32=True, residual="f32", pad=8), dict(out_f32=True, residual="f32", res_stats=True),
                            dict(out_f32=True, residual="f32", res_stats=True, res_index=True, pad=8), dict(out_f32=True, residual="f32", act=1),
                            dict(out_f32=True, residual="f32", res_index=True))),
    "F32_SCALE": (N_LO + N_FOUR, (dict(out_f32=True, scale=True), dict(out_f32=True, scale=True, range_final=1, pad=8))),
    "BOTH": (N_LO + N_FOUR, (dict(out_f32=True, out_lo=True), dict(out_f32=True, out_lo=True, pad=8))),
    "F32_LN": (N_PRODUCER, (dict(out_f32=True, out_lo=True, stats_part=True, residual="f32"),
                            dict(out_f32=True, out_lo=True, stats_part=True, residual="f32", res_stats=True, pad=8),
                            dict(out_f32=True, out_lo=True, stats_part=True, residual="f32", res_stats=True, res_index=True))),
    "LO_FOLD": (N_LO, (dict(out_lo=True, fold=True), dict(out_lo=True, fold=True, act=1), dict(out_lo=True, fold=True, act=2, pad=8))),
    "LO_LN": (N_PRODUCER, (dict(out_lo=True, stats_part=True, residual="f32", act=1), dict(out_lo=True, stats_part=True, residual="f32", act=1, pad=8))),
    "F32_SCALE_FOLD": (N_LO + N_FOUR, (dict(out_f32=True, fold=True, scale=True), dict(out_f32=True, fold=True, scale=True, range_final=1, pad=8))),
    "LN16": (N_PRODUCER, (dict(out_lo=True, stats_part=True, residual="lo"), dict(out_lo=True, stats_part=True, residual="lo", res_stats=True, pad=8),
                          dict(out_lo=True, stats_part=True, residual="lo", res_stats=True, res_index=True), dict(out_lo=True, stats_part=True, residual="lo", res_index=True))),
    "GENERIC": (N_LO, (dict(out_f32=True, act=2, residual="f32"), dict(out_f32=True, out_lo=True, split="mid"), dict(out_f32=True, act=1, residual="f32", res_stats=True, res_index=True),
                       dict(out_f32=True, out_lo=True, residual="f32", pad=8), dict(out_f32=True, scale=True, act=2), dict(out_f32=True, act=1))),
}
# what the 128x128, gemm8r and (without a residual or a Rescaler) 384x256 tiles carry as well: the same arguments, the same bits
SHARED = (dict(out_lo=True, act=1), dict(out_f32=True), dict(out_f32=True, out_lo=True), dict(out_f32=True, act=2, residual="f32"),
          dict(out_f32=True, residual="f32", res_stats=True, res_index=True, pad=8), dict(out_f32=True, act=1, residual="f32", res_stats=True),
          dict(out_f32=True, out_lo=True, split="mid"), dict(out_f32=True, scale=True), dict(out_lo=True, act=2, residual="f32", res_index=True),
          dict(out_f32=True, out_lo=True, act=2, bias=False))
SHARED_SHAPES = ((300, 264), (513, 520), (300, 256), (513, 512), (257, 136))          # 256 / 512 columns: the 384-row tile's
DST_MODES = ("F32_SCALE", "F32_SCALE_FOLD")
DST_SHAPES = ((1, 8), (65, 136), (129, 132), (257, 264), (300, 260), (513, 520))


def build(kind, m, n, k, flavour, **opts):
    kw = dict(flavour)
    if kw.pop("split", None):
        kw["split_col"] = 8 * (n // 16)
    kw.update(opts)
    return fc.make_case(kind, m, n, k, **kw)


def sweep(mode, kind, k):
    """the (m, n) sweep of a mode: every flavour meets every m and every n; gemm_variant 7 (an option of the handle: every launch that can
    takes gemm4d) so that the small m reach the tile too; full tiles (gemm_tail_split 0)"""
    ns, flavours = MODES[mode]
    return [build(kind, m, n, k, flavours[(i + j) % len(flavours)], gemm_variant=7) for i, m in enumerate(MS) for j, n in enumerate(ns)]


def tail_options(c):
    """the other tail splits a case runs with, bit for bit: 1 (the default: at these sizes half tiles throughout), 2 where the cut lands
    inside (256 or 512), 3 on the first column count of the sweep"""
    return [1] + ([2] if c.m > 256 else []) + ([3] if c.n in (8, 128) else [])


# ---- plumbing ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", autouse=True)
def _record():
    yield
    path = fc.record_path()          # figures for profiles/gemm_fwd_check.md
    if path and tc.RECORD:
        fc.write_record(path)


def _lib():
    from zett_amd import _lib
    return _lib, _lib.load()


class Dev:
    """the device copies of a test function's inputs: NaN-framed, uploaded once per distinct (name, shape, leading dimension)"""

    def __init__(self):
        self.cache = {}
        self.flag = torch.zeros(64, dtype=torch.int32, device=DEV)

    def matrix(self, name, values, ld, pool, rows_alloc=None):
        key = (name, id(pool), tuple(values.shape), ld, rows_alloc)
        if key not in self.cache:
            rows, cols = values.shape
            fr = gc.Framed(rows_alloc or rows, cols, ld, values.dtype, float("nan"))
            fr.view(fr.buf)[:rows] = values
            self.cache[key] = (fr, fr.buf.to(DEV))
        fr, buf = self.cache[key]
        return buf.data_ptr() + fr.byte_offset()

    def vector(self, name, values, pool):
        key = (name, id(pool), tuple(values.shape))
        if key not in self.cache:
            if values.dtype == F32:
                fr = gc.Framed(None, values.shape[0], values.shape[0], F32, float("nan"), values=values)
                self.cache[key] = (fr, fr.buf.to(DEV), fr.byte_offset(), values)
            else:          # index arrays: valid everywhere
                self.cache[key] = (None, values.to(DEV), 0, values)
        _, buf, off, _ = self.cache[key]          # (the entry keeps `values` alive: its id is part of the key)
        return buf.data_ptr() + off


def launch(dev, c, frames=None, planted=None):
    """one call -> (buffers brought back: name -> host tensor, variant, mode, range word).  planted: name -> tensor replacing a per-column
    vector of the case (range-guard tests)."""
    L, lib = _lib()
    p = c.pool
    frames = fc.output_frames(c) if frames is None else frames
    dbuf = {name: fr.buf.to(DEV) for name, fr in frames.items()}
    ptr = lambda name: dbuf[name].data_ptr() + frames[name].byte_offset() if name in frames else None
    d = L.ZettFwdGemmDesc()
    d.size = C.sizeof(L.ZettFwdGemmDesc)
    d.a = dev.matrix("a", c.a, c.k, p, rows_alloc=c.a_rows_readable if c.a_rows_readable > c.m else None)
    d.w = dev.matrix("w", c.w, c.k, p)
    d.lda = d.ldw = c.k
    d.m, d.n, d.k, d.act, d.a_rows_readable = c.m, c.n, c.k, c.act, c.a_rows_readable
    planted = planted or {}
    for name in ("bias", "res_gamma", "res_beta", "fold_c", "scale", "shift", "res_index"):
        v = planted.get(name, getattr(c, name))
        if v is not None:
            setattr(d, name, dev.vector(name if name not in planted else name + " planted", v, p if name not in planted else v))
    if c.residual is not None:
        d.residual, d.ld_res = dev.matrix("residual", c.residual, c.ld_res, p), c.ld_res
    if c.residual_lo is not None:
        d.residual_lo, d.ld_res_lo = dev.matrix("residual_lo", c.residual_lo, c.ld_res_lo, p), c.ld_res_lo
    if c.res_stats is not None:
        d.res_stats = dev.matrix("res_stats", c.res_stats, 2, p)
    if c.fold_stats is not None:
        d.fold_stats = dev.matrix("fold_stats", c.fold_stats, 2, p)
    d.out_f32, d.out_lo, d.out_f32_b, d.stats_part, d.dst = ptr("out_f32"), ptr("out_lo"), ptr("out_f32_b"), ptr("parts"), ptr("dst")
    d.ld_f32, d.ld_lo, d.ld_part, d.split_col = c.ld_f32, c.ld_lo, c.ld_part, c.split_col
    if c.dst:
        d.ld_dst, d.dst_dtype = c.ld_dst, c.dst_dtype
        if c.dst_rows is not None:
            d.dst_rows = dev.vector("dst_rows", c.dst_rows, c.dst_rows)
    dev.flag.zero_()
    d.range_flag, d.range_final = dev.flag.data_ptr(), c.range_final
    d.gemm_variant, d.gemm4d_min_k, d.gemm_tail_split, d.gemm_tile_order, d.gemm_group = c.gemm_variant, c.gemm4d_min_k, c.gemm_tail_split, c.gemm_tile_order, c.gemm_group
    variant, mode = C.c_int32(-9), C.c_int32(-9)
    st = C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)
    rc = lib.zett_op_fwd_gemm({"bf16": L.PREC_BF16, "f32": L.PREC_F32, "f16": L.PREC_F16}[c.kind], C.byref(d), C.byref(variant), C.byref(mode), st)
    if rc != 0:
        raise AssertionError(f"{describe(c)}: return code {rc}: {lib.zett_last_error().decode()}")
    torch.cuda.synchronize()
    return {name: b.cpu() for name, b in dbuf.items()}, variant.value, mode.value, int(dev.flag[0].item())


def describe(c):
    feats = [f for f in ("out_f32", "out_lo", "stats_part", "dst") if getattr(c, f)] + [f for f in ("bias", "residual", "residual_lo", "res_stats", "res_index", "fold_stats", "scale")
                                                                                          if getattr(c, f) is not None]
    return (f"{c.kind} [{c.m}, {c.n}] k={c.k} act={c.act} {'+'.join(feats)} split_col={c.split_col} variant option {c.gemm_variant} tail {c.gemm_tail_split} "
            f"order {c.gemm_tile_order} group {c.gemm_group}")


def run_checked(dev, c, key):
    """launch, assert the reported path and a clean range word, check every output -> (buffers, frames, variant, mode)"""
    frames = fc.output_frames(c)
    bufs, variant, mode, word = launch(dev, c, frames)
    what = describe(c)
    v_exp, m_exp, _ = fc.path_expected(c)
    assert (variant, mode) == (v_exp, m_exp), f"{what}: ran variant {variant} mode {mode}, the rule says {v_exp} / {m_exp}"
    assert word == 0, f"{what}: range word {word} on clean inputs"
    fc.check_launch(c, fc.expect(c), frames, bufs, what, mode=mode if mode >= 0 else None, key=key)
    return bufs, frames, variant, mode


def same_bits(dev, c, ref_bufs, **opts):
    """the case with other options: every output allocation bit for bit what the checked launch left (canary included)"""
    c2 = c.replace(**opts)
    bufs, variant, mode, word = launch(dev, c2)
    v_exp, m_exp, _ = fc.path_expected(c2)
    assert (variant, mode) == (v_exp, m_exp), f"{describe(c2)}: ran variant {variant} mode {mode}, the rule says {v_exp} / {m_exp}"
    assert word == 0, f"{describe(c2)}: range word {word} on clean inputs"
    for name, b in bufs.items():
        a = ref_bufs[name]
        same = torch.equal(tc._bits(a), tc._bits(b))
        if not same:
            where = torch.nonzero(tc._bits(a) != tc._bits(b)).flatten()
            raise AssertionError(f"{describe(c2)}: {name} differs in {where.numel()} element(s) from the same launch with {describe(c)}; first at flat index {int(where[0])}")
    return variant, mode


# ---- every epilogue mode at the tile edges -----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", KS16)
@pytest.mark.parametrize("kind", KINDS16)
@pytest.mark.parametrize("mode", tuple(MODES))
def test_mode_at_every_edge(mode, kind, k):
    """M x N of the mode's sweep on full tiles, every output element by element; then the same launch with the other tail splits — HALF
    tiles throughout, the cut at 256 / 512, HALF tiles only — bit for bit."""
    dev = Dev()
    for c in sweep(mode, kind, k):
        _, v_mode, _ = fc.path_expected(c)
        bufs, _, variant, got_mode = run_checked(dev, c, key=(fc.MODE_NAMES[v_mode] if v_mode >= 0 else "tile 1/2", f"{kind} k={k}"))
        if variant == 7:
            for ts in tail_options(c):
                same_bits(dev, c, bufs, gemm_tail_split=ts)


@gpu
@pytest.mark.parametrize("kind", KINDS16)
@pytest.mark.parametrize("mode", tuple(MODES))
def test_tile_order_and_group(mode, kind):
    """both tile orders and groups of 1 and 8 tiles, on three row tiles x three column tiles: the same bits"""
    ns, flavours = MODES[mode]
    dev = Dev()
    n = {N_PRODUCER: 640, N_LO: 520}.get(ns, 520)
    for f in flavours[:2]:
        c = build(kind, 513, n, 192, f, gemm_variant=7)
        bufs, _, variant, _ = run_checked(dev, c, key=None)
        assert variant == 7
        for order in (0, 1):
            for group in (0, 1, 8):
                for ts in (0, 1):
                    if (order, group, ts) != (0, 0, 0):
                        same_bits(dev, c, bufs, gemm_tile_order=order, gemm_group=group, gemm_tail_split=ts)


# ---- the same arguments on every variant ---------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("k", (64, 576))
@pytest.mark.parametrize("kind", KINDS16 + ("f32",))
def test_variants_give_the_same_bits(kind, k):
    """the epilogues every tile carries, on variants 1, 2, 3 (where the rule lets it run: 256 | n, no residual, no Rescaler, readable
    rows), 7 and 8: variant 1 element by element, the others bit for bit against it"""
    k = k if kind != "f32" else k // 2
    dev = Dev()
    ran = set()
    for m, n in SHARED_SHAPES:
        for f in SHARED:
            c = build(kind, m, n, k, f, gemm_variant=1, a_slack=True)
            bufs, _, variant, _ = run_checked(dev, c, key=("tile 128x128", f"{kind} k={k}"))
            assert variant == 1
            ran.add(variant)
            for v in (2, 3, 7, 8, 0):
                got, _ = same_bits(dev, c, bufs, gemm_variant=v)
                ran.add(got)
    assert ran == ({1, 2, 3} if kind == "f32" else {1, 2, 3, 7, 8}), ran


@gpu
@pytest.mark.parametrize("k", KS32)
def test_fp32_operands_at_the_edges(k):
    """fp32 operands (exact-fp32 MFMA; the 128x128 and gemm8r tiles): the shared epilogues over M x N, the option left to the rule"""
    dev = Dev()
    for i, m in enumerate(MS):
        for j, n in enumerate(N_LO + N_FOUR):
            c = build("f32", m, n, k, SHARED[(i + j) % len(SHARED)])
            run_checked(dev, c, key=("tile 1/2 fp32", f"f32 k={k}"))


@gpu
@pytest.mark.parametrize("kind", KINDS16)
def test_the_384_row_tile(kind):
    """variant 3 on its own, element by element: 256 and 512 columns, row counts around its 128-row wave rows and its 384-row edge; A
    has the readable rows the tile reads, and the launch falls back to variant 2 when a_rows_readable does not cover them"""
    dev = Dev()
    for k in (64, 192):
        for m in (1, 129, 383, 384, 385, 513):
            for j, n in enumerate(N_V3):
                f = (dict(out_lo=True, act=1), dict(out_f32=True, out_lo=True), dict(out_f32=True, act=2))[(m + j) % 3]
                c = build(kind, m, n, k, f, gemm_variant=3, a_slack=True)
                bufs, _, variant, _ = run_checked(dev, c, key=("tile 384x256", f"{kind} k={k}"))
                assert variant == 3
                variant, _ = same_bits(dev, c.replace(a_rows_readable=c.m), bufs)
                assert variant == (2 if m % 384 else 3)


# ---- destination stores ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dst_dtype", (0, 1, 2))
@pytest.mark.parametrize("kind", KINDS16)
@pytest.mark.parametrize("mode", DST_MODES)
def test_destination_stores(mode, kind, dst_dtype):
    """F32_SCALE / F32_SCALE_FOLD storing into a destination of each type: the twin launch into out_f32 is checked element by element, the
    destination must be its conversion bit for bit at the mapped rows (a permutation with skipped rows, ld_dst > n; or no map), the
    canary everywhere else; full and HALF tiles"""
    dev = Dev()
    flavour = MODES[mode][1][0]
    for i, (m, n) in enumerate(DST_SHAPES):
        k = KS16[i % 4]
        twin = build(kind, m, n, k, flavour, gemm_variant=7)
        bufs, frames, variant, got_mode = run_checked(dev, twin, key=None)
        f32 = frames["out_f32"].view(bufs["out_f32"]).clone()
        for ts in (0, 1):
            c = build(kind, m, n, k, dict(flavour, out_f32=False), gemm_variant=7, dst=True, dst_dtype=dst_dtype, dst_map=(i + ts) % 2 == 0, gemm_tail_split=ts)
            v_exp, m_exp, _ = fc.path_expected(c)
            if v_exp != 7:          # n % 8: the rule sends the launch to the 128x128 tile, where the forward stages the rows — the entry refuses
                continue
            frames_d = fc.output_frames(c)
            dbufs, variant, dmode, word = launch(dev, c, frames_d)
            assert (variant, dmode) == (7, m_exp) and dmode == got_mode and word == 0, (describe(c), variant, dmode, word)
            fc.check_launch(c, None, frames_d, dbufs, describe(c), f32_twin=f32)


# ---- the range guard ---------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", KINDS16)
def test_range_guard_reports_exactly_the_documented_bit(kind):
    """one planted value: a 16-bit output above 65504 (ZETT_RANGE_ACTIVATION, f16 only), an infinite fp32 output with range_final
    (ZETT_RANGE_OUTPUT), a finite value from 65520 up into an f16 destination (ZETT_RANGE_DEST); the word is exactly that bit, on every
    tile that carries the guard (the 384-row tile does not)"""
    dev = Dev()
    m, n, k = 300, 264, 128
    f16 = kind == "f16"

    def word(c, **planted):
        return launch(dev, c, planted=planted)[3]

    col = 133
    for variant, ts in ((7, 0), (7, 1), (8, 0), (2, 0), (1, 0)):
        big = fc.pool(kind, k).bias[:n].clone()
        big[col] = 70000.0
        c = build(kind, m, n, k, dict(out_lo=True), gemm_variant=variant, gemm_tail_split=ts)
        assert word(c) == 0 and word(c, bias=big) == (fc.RANGE_ACTIVATION if f16 else 0), (variant, ts)
        c = build(kind, m, n, k, dict(out_f32=True, out_lo=True), gemm_variant=variant, gemm_tail_split=ts)
        assert word(c, bias=big) == (fc.RANGE_ACTIVATION if f16 else 0), (variant, ts)
        inf = fc.pool(kind, k).bias[:n].clone()
        inf[col] = float("inf")
        c = build(kind, m, n, k, dict(out_f32=True, scale=True, range_final=1), gemm_variant=variant, gemm_tail_split=ts)
        assert word(c) == 0 and word(c, bias=inf) == fc.RANGE_OUTPUT, (variant, ts)
        assert word(c.replace(range_final=0), bias=inf) == 0, (variant, ts)
    shift = fc.pool(kind, k).shift[:n].clone()
    shift[col] = 66000.0
    for ts in (0, 1):
        for fold in (False, True):
            for dtype, want in ((1, fc.RANGE_DEST), (2, 0), (0, 0)):
                c = build(kind, m, n, k, dict(scale=True, fold=fold), gemm_variant=7, gemm_tail_split=ts, dst=True, dst_dtype=dtype)
                assert word(c) == 0 and word(c, shift=shift) == want, (ts, fold, dtype)
