"""tests/gemm_fwd_check.py without a GPU: the fp32 emulation of a forward GEMM launch stays well inside every bound and passes every
check; ten planted defects each raise a mismatch that names the element; the case tables of tests/test_gemm_fwd_direct_gpu.py reach
what they claim, by the restated dispatch; zett_op_fwd_gemm refuses what include/zett_hip.h says it refuses (a refused call launches
nothing, and every call here has m = 0 besides: host addresses do)."""
import ctypes as C

import pytest
import torch

from tests import gemm_fwd_check as fc
from tests import test_gemm_fwd_direct_gpu as T
from tests import train_ops_check as tc

F32, F64 = torch.float32, torch.float64


def _emulated(c):
    """emulate -> (outs, frames, bufs as a launch would leave them)"""
    outs = fc.emulate(c)
    frames = fc.output_frames(c)
    return outs, frames, fc.place(frames, outs)


def _ratio(got, ref, bnd):
    err = (got.to(F64) - ref).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / bnd.clamp_min(1e-300)).max())


# ---- the emulation -----------------------------------------------------------------------------------------------------------------
def _host_cases(kind):
    """a cut of the GPU test's tables small enough for a CPU: every mode and flavour, rows 65 and 300, every N of the mode, K of one and
    three steps"""
    if kind == "f32":
        return [T.build("f32", m, n, k, f) for k in (32, 96) for m in (65, 300) for n, f in zip((8, 136, 264, 520, 132, 260, 264, 136, 520), T.SHARED)]
    out = []
    for mode in T.MODES:
        for k in (64, 192):
            out += [c for c in T.sweep(mode, kind, k) if c.m in (65, 300)]
    return out


@pytest.mark.parametrize("kind", ("bf16", "f16", "f32"))
def test_emulation_stays_inside_every_bound_and_passes(kind):
    """the fp32 value below a quarter of its bound (every bound here holds the K-long sum); the partials in the kernel's tree, against the
    emulation's own output row as the check does: below a quarter of the sum bound where the fp32 row leaves (F32_LN), below half where the
    bound is made of the half-ulps of the 16-bit copy (LN16, LO_LN: 128 roundings that a right kernel commits exactly as the emulation does,
    dominated by the row's few largest elements — a handful of roundings, not a long sum); and the whole launch passes check_launch"""
    worst_v = worst_p = worst_p16 = 0.0
    for c in _host_cases(kind):
        exp = fc.expect(c)
        outs, frames, bufs = _emulated(c)
        what = T.describe(c)
        worst_v = max(worst_v, _ratio(outs["v32"], exp["v"], exp["b_v"]))
        if c.stats_part:
            mode = fc.epi_mode_expected(c)
            own = outs["out_f32"] if c.out_f32 else outs["out_lo"]
            ref, bnd = fc.parts_bound(own.to(F64), mode, None if c.out_f32 else fc.DT[kind])
            if c.out_f32:
                worst_p = max(worst_p, _ratio(outs["parts"], ref, bnd))
            else:
                worst_p16 = max(worst_p16, _ratio(outs["parts"], ref, bnd))
        fc.check_launch(c, exp, frames, bufs, what)
    assert worst_v <= 0.25, worst_v
    assert worst_p <= 0.25, worst_p
    assert worst_p16 <= 0.5, worst_p16


def test_destination_images_pass_and_the_emulated_twin_converts_exactly():
    for dtype in (0, 1, 2):
        for dst_map in (True, False):
            c = T.build("f16", 65, 136, 64, dict(scale=True, fold=True), dst=True, dst_dtype=dtype, dst_map=dst_map, gemm_variant=7)
            outs, frames, bufs = _emulated(c)
            fc.check_launch(c, None, frames, bufs, T.describe(c), f32_twin=outs["v32"])


# ---- planted defects ---------------------------------------------------------------------------------------------------------------
def _raises_at(c, outs, rows=None, cols=None, f32_twin=None):
    """outs (a defective launch's outputs) checked as case c -> the OpMismatch; its (row, col) must lie in rows / cols when given"""
    frames = fc.output_frames(c)
    bufs = fc.place(frames, outs)
    with pytest.raises(tc.OpMismatch) as info:
        fc.check_launch(c, fc.expect(c) if not c.dst else None, frames, bufs, "planted", f32_twin=f32_twin)
    e = info.value
    if rows is not None:
        assert e.row in rows, (e.row, str(e))
    if cols is not None:
        assert e.col in cols, (e.col, str(e))
    assert "row" in str(e)
    return e


@pytest.mark.parametrize("kind", ("bf16", "f16"))
def test_statistics_of_the_next_row_are_caught(kind):
    """1. inside one 64-row pass, row m computed with the statistics of row m + 1: the fold consumer and the LayerNorm'd residual"""
    c = T.build(kind, 129, 264, 64, dict(out_lo=True, fold=True), gemm_variant=7)
    st = c.fold_stats.clone()
    st[64:127] = c.fold_stats[65:128]
    _raises_at(c, fc.emulate(c.replace(fold_stats=st)), rows=range(64, 127))
    c = T.build(kind, 129, 264, 64, dict(out_f32=True, fold=True, scale=True), gemm_variant=7)
    st = c.fold_stats.clone()
    st[5] = c.fold_stats[6]
    _raises_at(c, fc.emulate(c.replace(fold_stats=st)), rows=[5])
    c = T.build(kind, 129, 256, 64, dict(out_f32=True, out_lo=True, stats_part=True, residual="f32", res_stats=True), gemm_variant=7)
    st = c.res_stats.clone()
    st[70] = c.res_stats[71]
    _raises_at(c, fc.emulate(c.replace(res_stats=st)), rows=[70])
    c = T.build(kind, 129, 256, 64, dict(out_lo=True, stats_part=True, residual="lo", res_stats=True, res_index=True), gemm_variant=7)
    st = c.res_stats.clone()
    r = int(c.res_index[70])
    st[r] = c.res_stats[int(c.res_index[71])]
    hit = [i for i in range(c.m) if int(c.res_index[i]) == r]
    _raises_at(c, fc.emulate(c.replace(res_stats=st)), rows=hit)


@pytest.mark.parametrize("kind", ("bf16", "f16"))
def test_column_vectors_shifted_by_four_columns_are_caught(kind):
    """2. fold_c / gamma read four columns off"""
    c = T.build(kind, 65, 264, 64, dict(out_lo=True, fold=True), gemm_variant=7)
    _raises_at(c, fc.emulate(c.replace(fold_c=torch.roll(c.fold_c, 4))))
    c = T.build(kind, 65, 260, 64, dict(out_f32=True, fold=True, scale=True), gemm_variant=7)
    _raises_at(c, fc.emulate(c.replace(fold_c=torch.roll(c.fold_c, 4))))
    c = T.build(kind, 65, 264, 64, dict(out_f32=True, residual="f32", res_stats=True), gemm_variant=7)
    _raises_at(c, fc.emulate(c.replace(res_gamma=torch.roll(c.res_gamma, 4))))
    c = T.build(kind, 65, 256, 64, dict(out_lo=True, stats_part=True, residual="lo", res_stats=True), gemm_variant=7)
    _raises_at(c, fc.emulate(c.replace(res_gamma=torch.roll(c.res_gamma, 4))))


PRODUCERS = (dict(out_f32=True, out_lo=True, stats_part=True, residual="f32"), dict(out_lo=True, stats_part=True, residual="f32", act=1),
             dict(out_lo=True, stats_part=True, residual="lo", res_stats=True))


@pytest.mark.parametrize("flavour", PRODUCERS)
@pytest.mark.parametrize("kind", ("bf16", "f16"))
def test_misplaced_partials_are_caught(kind, flavour):
    """3. a partial written to slice s ^ 1; 4. two rows' partials swapped"""
    c = T.build(kind, 129, 384, 64, flavour, gemm_variant=7)
    outs = fc.emulate(c)
    p = outs["parts"].clone()
    p[[0, 1], 77] = p[[1, 0], 77]
    e = _raises_at(c, dict(outs, parts=p), rows=[0, 1], cols=[154, 155])
    assert "row 77" in str(e) and "slice" in str(e)
    p = outs["parts"].clone()
    p[2, [3, 64]] = p[2, [64, 3]]
    e = _raises_at(c, dict(outs, parts=p), rows=[2], cols=[6, 7, 128, 129])
    assert "slice 2" in str(e)


@pytest.mark.parametrize("kind", ("bf16", "f16"))
def test_partials_over_the_rounded_values_are_caught(kind):
    """5. F32_LN: a partial that sums the 16-bit-rounded values instead of the fp32 ones"""
    c = T.build(kind, 129, 384, 64, PRODUCERS[0], gemm_variant=7)
    outs = fc.emulate(c)
    _raises_at(c, dict(outs, parts=fc._parts32(outs["out_lo"].float(), fc.F32_LN)))


@pytest.mark.parametrize("kind", ("bf16", "f16"))
def test_a_residual_row_taken_from_m_is_caught(kind):
    """6. the residual row of output row m taken from row m instead of res_index[m]"""
    for f in (dict(out_f32=True, residual="f32", res_index=True), dict(out_lo=True, stats_part=True, residual="lo", res_index=True),
              dict(out_f32=True, out_lo=True, stats_part=True, residual="f32", res_stats=True, res_index=True)):
        c = T.build(kind, 65, 256, 64, f, gemm_variant=7)
        wrong = c.replace(res_index=None)
        fixed = [i for i in range(c.m) if int(c.res_index[i]) == i]
        e = _raises_at(c, fc.emulate(wrong))
        assert e.row not in fixed


@pytest.mark.parametrize("kind", ("bf16", "f16"))
def test_an_untouched_last_slice_is_caught(kind):
    """7. the last 128-column slice of an N = 384 launch left as it was: its elements still hold the canary"""
    c = T.build(kind, 65, 384, 64, PRODUCERS[0], gemm_variant=7)
    outs = fc.emulate(c)
    frames = fc.output_frames(c)
    for name in ("out_f32", "out_lo", "parts"):
        bufs = fc.place(frames, outs)
        view = frames[name].view(bufs[name])
        keep = frames[name].view(frames[name].buf)
        if name == "parts":
            view[2] = keep[2]
        else:
            view[:, 256:] = keep[:, 256:]
        with pytest.raises(AssertionError, match="not finite") as info:
            fc.check_launch(c, fc.expect(c), frames, bufs, "planted")
        assert ("[2, 0]" if name == "parts" else "[0, 256]") in str(info.value)


@pytest.mark.parametrize("dtype", (0, 1, 2))
def test_a_skipped_destination_row_that_is_written_is_caught(dtype):
    """8. a row with dst_rows < 0 stored anyway (at the row its index would have had)"""
    c = T.build("bf16", 65, 136, 64, dict(scale=True), dst=True, dst_dtype=dtype, gemm_variant=7)
    outs = fc.emulate(c)
    free = sorted(set(range(c.n_dst)) - set(int(r) for r in c.dst_rows if r >= 0))
    rows = c.dst_rows.clone()
    rows[3] = free[0]
    assert int(c.dst_rows[3]) < 0
    img = fc.dst_image(c.replace(dst_rows=rows), outs["v32"])
    e = _raises_at(c, dict(outs, dst=img), rows=[free[0]], f32_twin=outs["v32"])
    assert "must keep the canary" in str(e)


def _truncate(v32, dtype):
    """fp32 -> 16-bit by truncation (round toward zero)"""
    if dtype == torch.bfloat16:
        return (v32.contiguous().view(torch.int32) & -65536).view(F32).to(dtype)
    x = v32.to(dtype)
    bits = x.view(torch.int16)
    over = x.float().abs() > v32.abs()          # rounded away from zero: one step back (the magnitude bits of a finite half count up)
    return torch.where(over, bits - 1, bits).view(dtype)


@pytest.mark.parametrize("kind", ("bf16", "f16"))
def test_a_truncated_16_bit_output_is_caught(kind):
    """9. out_lo truncated instead of rounded to nearest even: against T(out_f32) where both leave, by lo_bound where only it does"""
    dt = fc.DT[kind]
    for f in (dict(out_f32=True, out_lo=True), dict(out_lo=True), dict(out_lo=True, fold=True, act=1), dict(out_lo=True, stats_part=True, residual="lo")):
        c = T.build(kind, 65, 256, 64, f, gemm_variant=7)
        outs = fc.emulate(c)
        _raises_at(c, dict(outs, out_lo=_truncate(outs["v32"], dt)))


@pytest.mark.parametrize("kind", ("bf16", "f16"))
def test_columns_past_split_col_in_out_f32_are_caught(kind):
    """10. columns >= split_col stored to out_f32 (at row * ld_f32 + column) as well as to out_f32_b"""
    for pad in (0, 160):
        c = T.build(kind, 65, 264, 64, dict(out_f32=True, out_lo=True, split="mid", pad=pad), gemm_variant=7)
        outs = fc.emulate(c)
        frames = fc.output_frames(c)
        bufs = fc.place(frames, outs)
        fr = frames["out_f32"]
        for r in range(c.m):
            bufs["out_f32"][fr.offset + r * fr.ld + c.split_col: fr.offset + r * fr.ld + c.n] = outs["v32"][r, c.split_col:]
        with pytest.raises((tc.OpMismatch, tc.CanaryBroken)) as info:
            fc.check_launch(c, fc.expect(c), frames, bufs, "planted")
        assert "row" in str(info.value)
        if pad:          # ld_f32 >= n: the stray columns land in the canary columns behind the row
            assert info.value.where[0] == (0, c.split_col)


# ---- what the case tables reach -------------------------------------------------------------------------------------------------------
def test_the_tables_reach_every_mode_tile_variant_and_destination():
    streamlined = set(range(1, 10))
    for kind in T.KINDS16:
        modes, tiles, early = set(), {}, set()
        for mode in T.MODES:
            for k in T.KS16:
                for c in T.sweep(mode, kind, k):
                    for ts in [0] + T.tail_options(c):
                        v, md, tile = fc.path_expected(c.replace(gemm_tail_split=ts))
                        if v in (7, 8):
                            modes.add(md)
                            tiles.setdefault(md, set()).add(tile)
                            if md == fc.LN16:
                                early.add((c.res_index is None, tile))
        assert modes == set(range(10)), (kind, modes)
        for md in streamlined:
            assert {"full", "half", "cut"} <= tiles[md], (kind, fc.MODE_NAMES[md], tiles[md])
        assert tiles[fc.GENERIC] == {"full"}
        # res16_early (LN16 without a row index) on and off, on both tiles
        assert early >= {(True, "full"), (True, "half"), (False, "full"), (False, "half")}
        # the six destination instantiations, each on full and half tiles
        dst = set()
        for mode in T.DST_MODES:
            for dtype in (0, 1, 2):
                for i, (m, n) in enumerate(T.DST_SHAPES):
                    for ts in (0, 1):
                        c = T.build(kind, m, n, T.KS16[i % 4], dict(T.MODES[mode][1][0], out_f32=False), gemm_variant=7, dst=True, dst_dtype=dtype, gemm_tail_split=ts)
                        v, md, tile = fc.path_expected(c)
                        if v == 7:
                            dst.add((md, dtype, tile))
        assert dst == {(md, dt, tile) for md in (fc.F32_SCALE, fc.F32_SCALE_FOLD) for dt in (0, 1, 2) for tile in ("full", "half")}
        # every feature the other tiles carry reaches variants 1, 2 and 8 (and 3 where that tile takes it), and the auto rule's 7
        reach = {}
        for m, n in T.SHARED_SHAPES:
            for f in T.SHARED:
                for opt in (1, 2, 3, 7, 8, 0):
                    c = T.build(kind, m, n, 64, f, gemm_variant=opt, a_slack=True)
                    v = fc.variant_expected(c)
                    feats = [name for name in ("bias", "residual", "res_stats", "res_index", "scale") if getattr(c, name) is not None]
                    feats += [f"act {c.act}"] + [name for name in ("out_f32", "out_lo") if getattr(c, name)] + (["split"] if c.split_col else [])
                    for name in feats:
                        reach.setdefault(name, set()).add(v)
        for name, vs in reach.items():
            want = {1, 2, 7, 8} | ({3} if name in ("bias", "act 0", "act 1", "act 2", "out_f32", "out_lo", "split") else set())
            assert want <= vs, (kind, name, vs)
        assert set(reach) == {"bias", "residual", "res_stats", "res_index", "scale", "act 0", "act 1", "act 2", "out_f32", "out_lo", "split"}
    # fp32 operands: the two tiles of the rule, and the 384-row tile by option
    f32 = {fc.variant_expected(T.build("f32", m, n, k, T.SHARED[(i + j) % len(T.SHARED)])) for k in T.KS32 for i, m in enumerate(T.MS) for j, n in enumerate(T.N_LO + T.N_FOUR)}
    assert f32 == {1, 2}
    # the K steps against the LDS stages: one, two, three, nine steps of 64
    assert [k // 64 for k in T.KS16] == [1, 2, 3, 9] and [k // 32 for k in T.KS32] == [1, 3, 17]


def test_the_restated_rule_at_its_cut_overs():
    b = lambda m, n, k, f, **o: T.build("f16", m, n, k, f, **o)
    lo = dict(out_lo=True)
    assert fc.path_expected(b(128, 264, 576, lo, gemm4d_min_k=512))[0] == 1 and fc.path_expected(b(129, 128, 576, lo, gemm4d_min_k=512))[0] == 1
    assert fc.path_expected(b(129, 136, 576, lo, gemm4d_min_k=512))[:2] == (7, fc.LO) and fc.path_expected(b(129, 136, 448, lo, gemm4d_min_k=512))[0] == 2
    assert fc.path_expected(b(129, 132, 576, dict(out_f32=True), gemm_variant=7))[0] == 1          # n % 8
    assert fc.path_expected(b(1, 8, 64, dict(out_lo=True, fold=True)))[:2] == (7, fc.LO_FOLD)          # a fold launch: gemm4d at any m
    assert fc.path_expected(b(300, 264, 64, dict(out_f32=True, residual="f32", scale=True), gemm_variant=7))[0] == 1
    assert fc.path_expected(b(300, 264, 64, dict(out_f32=True, act=2), gemm_variant=8))[:2] == (8, fc.GENERIC)
    assert fc.path_expected(b(300, 264, 64, dict(out_lo=True, fold=True), gemm_variant=8))[:2] == (7, fc.LO_FOLD)
    assert fc.path_expected(b(513, 512, 64, lo, gemm_variant=3, a_slack=True))[0] == 3 and fc.path_expected(b(513, 512, 64, lo, gemm_variant=3))[0] == 2
    assert fc.path_expected(b(513, 520, 64, lo, gemm_variant=7, gemm_tail_split=2))[2] == "cut" and fc.path_expected(b(255, 520, 64, lo, gemm_variant=7, gemm_tail_split=2))[2] == "full"
    assert fc.path_expected(b(300, 264, 64, dict(out_f32=True, act=1), gemm_variant=7, gemm_tail_split=3))[1:] == (fc.GENERIC, "full")


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def _lib():
    from zett_amd import _lib
    return _lib, _lib.load()


class _Host:
    """a descriptor on HOST addresses with m = 0: whatever the entry decides, nothing is launched"""

    def __init__(self):
        self.store = (C.c_float * 65536)()
        self.base = (C.addressof(self.store) + 255) & ~255

    def p(self, slot, off=0):
        return self.base + 4096 * slot + off

    def desc(self, **kw):
        L, _ = _lib()
        d = L.ZettFwdGemmDesc()
        d.size = C.sizeof(L.ZettFwdGemmDesc)
        d.a, d.w, d.lda, d.ldw, d.m, d.n, d.k = self.p(0), self.p(1), 128, 128, 0, 256, 128
        d.out_f32, d.ld_f32, d.gemm4d_min_k = self.p(2), 256, 512
        for name, v in kw.items():
            setattr(d, name, v)
        return d


def _call(prec, d):
    L, lib = _lib()
    return lib.zett_op_fwd_gemm(prec, C.byref(d), None, None, None)


def _refused(prec, d, *words):
    L, lib = _lib()
    rc = _call(prec, d)
    msg = lib.zett_last_error().decode()
    assert rc == L.E_INVALID, (rc, msg)
    assert all(w in msg for w in words), msg


def test_the_entry_refuses_what_the_header_says():
    L, lib = _lib()
    h = _Host()
    B, F, H = L.PREC_BF16, L.PREC_F32, L.PREC_F16
    assert _call(B, h.desc()) == 0 and _call(F, h.desc(k=32, lda=32, ldw=32)) == 0          # the baseline is accepted (m = 0: nothing launched)
    assert lib.zett_op_fwd_gemm(B, None, None, None, None) == L.E_INVALID
    _refused(B, h.desc(size=8), "descriptor size")
    _refused(B, h.desc(size=C.sizeof(L.ZettFwdGemmDesc) + 8), "descriptor size")
    _refused(3, h.desc(), "unknown precision")
    _refused(B, h.desc(act=3), "unknown act")
    _refused(B, h.desc(out_f32=None, dst=h.p(2), ld_dst=256, dst_dtype=3, scale=h.p(3), shift=h.p(4), gemm_variant=7), "unknown dst dtype")
    for k in (0, 32, 96, -64):
        _refused(B, h.desc(k=k), "multiple of 64")
    _refused(F, h.desc(k=48, lda=48, ldw=48), "multiple of 32")
    _refused(B, h.desc(lda=120), "at least k")
    _refused(B, h.desc(ldw=64), "at least k")
    _refused(B, h.desc(lda=132), "16-byte rows")
    _refused(F, h.desc(k=32, lda=34, ldw=32), "16-byte rows")
    for name in ("a", "w", "bias", "out_f32"):
        _refused(B, h.desc(**{name: h.p(5, 8)}), "16-byte aligned")
    _refused(B, h.desc(out_lo=h.p(5, 4), ld_lo=256), "16-byte aligned")
    _refused(B, h.desc(scale=h.p(5, 4), shift=h.p(6)), "16-byte aligned")
    _refused(B, h.desc(residual=h.p(5), ld_res=256, res_stats=h.p(6, 4), res_gamma=h.p(7), res_beta=h.p(8)), "8-byte aligned")
    _refused(B, h.desc(range_flag=h.p(5, 2)), "4-byte aligned")
    _refused(B, h.desc(a=None), "required")
    _refused(B, h.desc(ld_f32=255), "ld_f32")
    _refused(B, h.desc(out_lo=h.p(5), ld_lo=128), "ld_lo")
    _refused(B, h.desc(residual=h.p(5), ld_res=200), "ld_res")
    _refused(B, h.desc(out_f32=None, out_lo=h.p(5), ld_lo=256, stats_part=h.p(6), ld_part=-1, residual_lo=h.p(7), ld_res_lo=256), "ld_part")
    _refused(B, h.desc(out_f32=None, out_lo=h.p(5), ld_lo=256, stats_part=h.p(6), ld_part=8, residual_lo=h.p(7), ld_res_lo=8), "ld_res_lo")
    _refused(B, h.desc(out_f32=None, dst=h.p(2), ld_dst=128, scale=h.p(3), shift=h.p(4), gemm_variant=7), "ld_dst")
    _refused(B, h.desc(out_f32=None), "no output")
    for name in ("stats_part", "fold_stats", "residual_lo", "dst"):
        _refused(F, h.desc(k=32, lda=32, ldw=32, **{name: h.p(5)}), "16-bit features")
    _refused(B, h.desc(residual=h.p(5), ld_res=256, res_stats=h.p(6)), "res_gamma")
    _refused(B, h.desc(res_stats=h.p(6), res_gamma=h.p(7), res_beta=h.p(8)), "without a residual")
    _refused(B, h.desc(res_index=h.p(6)), "without a residual")
    _refused(B, h.desc(residual=h.p(5), ld_res=256, residual_lo=h.p(6), ld_res_lo=256), "together with residual_lo")
    _refused(B, h.desc(residual_lo=h.p(6), ld_res_lo=256), "stats_part is null")
    _refused(B, h.desc(scale=h.p(5)), "scale and shift together")
    _refused(B, h.desc(fold_stats=h.p(5)), "fold_stats and fold_c together")
    # stats_part / fold_stats combinations no instantiation carries (gemm4d_epi_mode returns -1)
    _refused(B, h.desc(stats_part=h.p(5), ld_part=8), "no gemm4d instantiation")                                              # a producer without out_lo / residual
    _refused(B, h.desc(stats_part=h.p(5), ld_part=8, out_lo=h.p(6), ld_lo=256, residual=h.p(7), ld_res=256, act=2), "no gemm4d instantiation")
    _refused(B, h.desc(n=264, ld_f32=264, stats_part=h.p(5), ld_part=8, out_lo=h.p(6), ld_lo=264, residual=h.p(7), ld_res=264), "no gemm4d instantiation")      # n % 128
    _refused(B, h.desc(fold_stats=h.p(5), fold_c=h.p(6)), "no gemm4d instantiation")                                          # an fp32 consumer without the Rescaler
    _refused(H, h.desc(fold_stats=h.p(5), fold_c=h.p(6), out_lo=h.p(7), ld_lo=256), "no gemm4d instantiation")                # both outputs
    _refused(B, h.desc(dst=h.p(5), ld_dst=256, scale=h.p(3), shift=h.p(4), gemm_variant=7), "cannot be combined")
    _refused(B, h.desc(dst_rows=h.p(5)), "dst_rows without dst")
    _refused(B, h.desc(out_f32=None, dst=h.p(2), ld_dst=256, gemm_variant=7), "no gemm4d instantiation stores")               # no Rescaler: not a head's epilogue
    _refused(B, h.desc(out_f32=None, dst=h.p(2), ld_dst=258, scale=h.p(3), shift=h.p(4), gemm_variant=7), "no gemm4d instantiation stores")
    _refused(B, h.desc(out_f32=None, dst=h.p(2), ld_dst=256, scale=h.p(3), shift=h.p(4), gemm_variant=2), "variant 7 only")
    _refused(B, h.desc(out_f32_b=h.p(5)), "split_col")
    _refused(B, h.desc(split_col=128), "split_col")
    for v in (-1, 4, 5, 6, 9):
        _refused(B, h.desc(gemm_variant=v), "gemm_variant")
    _refused(B, h.desc(gemm4d_min_k=32), "gemm4d_min_k")
    _refused(B, h.desc(gemm_tail_split=4), "gemm_tail_split")
    _refused(B, h.desc(gemm_tile_order=2), "gemm_tile_order")
    _refused(B, h.desc(gemm_group=65), "gemm_group")
    _refused(B, h.desc(m=-1), "negative")
    _refused(B, h.desc(a_rows_readable=-1), "a_rows_readable")
    _refused(B, h.desc(reserved=1), "reserved")
    # accepted shapes of the same descriptors (still m = 0)
    assert _call(B, h.desc(out_f32=None, dst=h.p(2), ld_dst=256, scale=h.p(3), shift=h.p(4), fold_stats=h.p(5), fold_c=h.p(6))) == 0
    assert _call(H, h.desc(out_f32=None, out_lo=h.p(5), ld_lo=256, stats_part=h.p(6), ld_part=8, residual_lo=h.p(7), ld_res_lo=256)) == 0
    assert _call(B, h.desc(split_col=128, out_f32_b=h.p(5))) == 0


def test_the_binding_matches_the_header():
    """struct zett_fwd_gemm_desc of include/zett_hip.h and ZettFwdGemmDesc name the same fields in the same order"""
    import os
    import re
    L, _ = _lib()
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "zett_hip.h")).read()
    body = text[text.index("typedef struct zett_fwd_gemm_desc {"):text.index("} zett_fwd_gemm_desc;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"^.*[\s*]", "", part.strip()) for part in decl.split(",")]
    assert names == [n for n, _ in L.ZettFwdGemmDesc._fields_]
