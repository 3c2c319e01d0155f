"""GPU: predicted rows straight into a destination matrix (zett_forward_into / zett_forward_table_into, HipEngine.forward_into,
ZettHypernet.predict_into).  Written rows equal forward()'s rows converted with torch's .to(dtype), bit for bit; skipped rows and
padding columns keep their sentinel."""
import warnings

import numpy as np
import pytest
import torch

from tests import util
from zett_amd import _lib, synth
from zett_amd.dims import HypernetDims

pytestmark = pytest.mark.gpu

TINY = util.golden_cases("fwd_tiny_*.npz")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
SENTINEL = {torch.float32: -0x21524111, torch.bfloat16: -0x2153, torch.float16: -0x2153}      # 0xdeadbeef / 0xdead bit patterns
INT = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}


def _cfg():
    cfg, *_ = synth.workload("tiny")
    return dict(cfg, n_embd=256, hn_hidden_size=512, hn_intermediate_size=1024, hn_num_attention_heads=8)


def _massive(weights, value=1.0e5):
    w = dict(weights)
    b = w["model.encoder.layer.0.attention.output.dense.bias"].copy()
    b[7] = value
    w["model.encoder.layer.0.attention.output.dense.bias"] = b
    return w


def _engine(cfg, weights, precision):
    from zett_amd.hypernet import HipEngine
    eng = HipEngine(HypernetDims.from_config(cfg), 1e-5, torch.device("cuda:0"), precision)
    eng.load_weights({k: torch.from_numpy(v).cuda() for k, v in weights.items()})
    return eng


def _filled(rows, cols, dtype):
    return torch.full((rows, cols), SENTINEL[dtype], dtype=INT[dtype], device="cuda").view(dtype)


def _dest(n, E, dtype, separate_out, ld_pad=64):
    """2n destination rows of ld E + ld_pad, sentinel everywhere; the [2n, E] views the call writes"""
    full_in = _filled(2 * n, E + ld_pad, dtype)
    full_out = _filled(2 * n, E + ld_pad, dtype) if separate_out else None
    full_bias = _filled(1, 2 * n, dtype)[0]
    return full_in, full_out, full_bias


def _rows(n, seed):
    g = np.random.default_rng(seed)
    rows = g.permutation(2 * n)[:n].astype(np.int64)
    rows[g.random(n) < 0.2] = -1
    return rows


def _check_into(ref, full, rows, E, dtype, what):
    """rows of `ref` (fp32 [n, E] or [n]) converted to dtype sit at rows[i] of full[:, :E]; everything else is the sentinel"""
    sentinel = _filled(1, 1, dtype).view(INT[dtype])[0, 0]
    bits = full.view(INT[dtype])
    r = torch.from_numpy(rows).cuda()
    keep = r >= 0
    want = ref.to(dtype).view(INT[dtype])[keep]
    assert torch.equal(bits[r[keep]][..., :E] if full.dim() == 2 else bits[r[keep]], want), what
    untouched = torch.ones(full.shape[0], dtype=torch.bool, device="cuda")
    untouched[r[keep]] = False
    assert bool((bits[untouched] == sentinel).all()), f"{what}: skipped rows overwritten"
    if full.dim() == 2:
        assert bool((bits[:, E:] == sentinel).all()), f"{what}: padding columns overwritten"


def _compare(eng, ids, src, lang, n, E, separate_out, dtype, seed, what):
    want = eng.forward(ids, src, lang)
    fi, fo, fb = _dest(n, E, dtype, separate_out)
    rows = _rows(n, seed)
    eng.forward_into(ids, src, lang, fi[:, :E], None if fo is None else fo[:, :E], fb, torch.from_numpy(rows).cuda())
    torch.cuda.synchronize()
    _check_into(want[0], fi, rows, E, dtype, f"{what} in")
    if separate_out:
        _check_into(want[1], fo, rows, E, dtype, f"{what} out")
    _check_into(want[2], fb, rows, E, dtype, f"{what} bias")


@pytest.mark.parametrize("path", TINY, ids=lambda p: p.split("/")[-1][:-4])
@pytest.mark.parametrize("precision", ["f32", "bf16", "f16"])
def test_tiny_golden_flags_into_every_dtype(path, precision):
    case = util.load_case(path)
    cfg = case["cfg"]
    w = synth.make_weights(cfg, case["seed"])
    src = torch.from_numpy(synth.make_source_embeddings(cfg, case["seed"], dtype=case["src_dtype"])).cuda()
    ids = torch.from_numpy(case["ids"].astype(np.int64)).cuda()
    eng = _engine(cfg, w, precision)
    lang = -1 if case["lang"] is None else case["lang"]
    for k, dtype in enumerate(DTYPES.values()):
        _compare(eng, ids, src, lang, ids.shape[0], cfg["n_embd"], bool(cfg.get("separate_out_embeddings")), dtype, k,
                 f"{case['name']} {precision} -> {dtype}")
    eng.close()


@pytest.mark.parametrize("precision,ln_fold", [("f32", 1), ("bf16", 1), ("f16", 1), ("bf16", 0), ("f16", 0)])
@pytest.mark.parametrize("n", [64, 700])
def test_h512_small_tile_and_fused_epilogue(precision, ln_fold, n):
    """H = 512: with the LayerNorm fold (the default) the heads are F32_SCALE_FOLD launches, which exist in gemm4d only (any M): fused
    at 64 and 700 rows.  Without it the heads are F32_SCALE launches: 64 rows take the 128x128 tile (staged fallback), 700 rows
    gemm4d (fused).  fp32 arithmetic: always staged."""
    cfg = _cfg()
    w = synth.make_weights(cfg, seed=31)
    src = torch.from_numpy(synth.make_source_embeddings(cfg, 31)).cuda()
    ids = torch.from_numpy(synth.make_surface_forms(cfg, n, seed=31, n_special=2)).cuda()
    eng = _engine(cfg, w, precision)
    eng.set_option("ln_fold", ln_fold)
    for k, dtype in enumerate(DTYPES.values()):
        _compare(eng, ids, src, 2, n, cfg["n_embd"], bool(cfg.get("separate_out_embeddings")), dtype, 100 + k, f"H512 {n} {precision} -> {dtype}")
        heads = [r for r in eng.gemm_log() if r["epilogue"] & (1024 | 2048)]
        assert len(heads) == 2, heads                                                  # pred_in and pred_out heads
        if precision != "f32" and (ln_fold or n == 700):
            assert all(r["epilogue"] & 1024 and not r["epilogue"] & 2048 and r["variant"] == 7 for r in heads), heads   # gemm4d's destination epilogues
        else:
            assert all(r["epilogue"] & 2048 and not r["epilogue"] & 1024 for r in heads), heads                         # staged + converting scatter
    eng.close()


def test_concurrent_lanes_and_chunks_match_identity():
    cfg = dict(_cfg(), separate_out_embeddings=False)
    w = synth.make_weights(cfg, seed=41)
    src = torch.from_numpy(synth.make_source_embeddings(cfg, 41)).cuda()
    n = 1500
    ids = torch.from_numpy(synth.make_surface_forms(cfg, n, seed=41, n_special=2)).cuda()
    E = cfg["n_embd"]
    eng = _engine(cfg, w, "f16")
    base = torch.empty((n, E), dtype=torch.bfloat16, device="cuda")
    bias = torch.empty((n,), dtype=torch.bfloat16, device="cuda")
    eng.forward_into(ids, src, 2, base, None, bias)
    for opt, val in (("concurrent_lanes", 2), ("max_chunk_tokens", 1024)):
        eng.set_option(opt, val)
        got = torch.empty_like(base)
        gb = torch.empty_like(bias)
        eng.forward_into(ids, src, 2, got, None, gb)
        if opt == "max_chunk_tokens":
            assert eng.stats()["chunks"] > 1
        assert torch.equal(got.view(torch.int16), base.view(torch.int16)) and torch.equal(gb.view(torch.int16), bias.view(torch.int16)), opt
        if opt == "concurrent_lanes":
            eng.set_option(opt, 0)
    eng.close()


@pytest.mark.parametrize("precision,single_head", [("f32", False), ("f16", True)], ids=["f32", "f16-single-head-split"])
def test_concurrent_lanes_on_the_staged_fallback(precision, single_head):
    """The staged fallback (fp32 arithmetic; the hn_single_head split in any mode) with two lanes at once: each lane stages its heads
    in its own buffer, so the pair equals the one-lane call and forward()'s rows, bit for bit, under a row map."""
    cfg = dict(_cfg(), hn_single_head=single_head, separate_out_embeddings=True)
    w = synth.make_weights(cfg, seed=43)
    src = torch.from_numpy(synth.make_source_embeddings(cfg, 43)).cuda()
    n = 1500
    ids = torch.from_numpy(synth.make_surface_forms(cfg, n, seed=43, n_special=2)).cuda()
    E = cfg["n_embd"]
    eng = _engine(cfg, w, precision)
    want = eng.forward(ids, src, 2)
    rows = _rows(n, 9)
    for lanes in (0, 2):
        eng.set_option("concurrent_lanes", lanes)
        for dtype in (torch.float32, torch.bfloat16):
            fi, fo, fb = _dest(n, E, dtype, True)
            eng.forward_into(ids, src, 2, fi[:, :E], fo[:, :E], fb, torch.from_numpy(rows).cuda())
            torch.cuda.synchronize()
            heads = [r for r in eng.gemm_log() if r["epilogue"] & (1024 | 2048)]
            assert heads and all(r["epilogue"] & 2048 for r in heads), heads          # (the staged path is what this test is about)
            if lanes:
                assert eng.stats()["chunks"] == 2                                       # (two lanes: one chunk each)
            what = f"{precision} single_head={single_head} lanes={lanes} -> {dtype}"
            _check_into(want[0], fi, rows, E, dtype, f"{what} in")
            _check_into(want[1], fo, rows, E, dtype, f"{what} out")
            _check_into(want[2], fb, rows, E, dtype, f"{what} bias")
    eng.close()


# ---- the headline shape (mistral_gpt2_32k: E = 4096, H = 4096; 16 column tiles per head, 128x256 row-split tiles) ---------------
@pytest.fixture(scope="module")
def headline():
    from bench import device_weights
    cfg, rows, src_dtype, hist = synth.workload("mistral_gpt2_32k")
    dev = torch.device("cuda:0")
    from zett_amd.hypernet import HipEngine
    eng = HipEngine(HypernetDims.from_config(cfg), 1e-5, dev, "f16")
    eng.load_weights(device_weights(cfg, dev, seed=0))
    g = torch.Generator(device=dev)
    g.manual_seed(1)
    src = (0.02 * torch.randn((cfg["original_vocab_size"], eng.dims.n_in_embd), device=dev, generator=g)).to(getattr(torch, src_dtype))
    ids = torch.from_numpy(synth.make_surface_forms(cfg, rows, seed=0, hist=hist)).to(dev).to(torch.int32).contiguous()
    lang = 3 if eng.dims.embed_lang else -1
    yield cfg, eng, src, ids, lang
    eng.close()


def test_headline_whole_vocabulary_into_bf16(headline):
    """The whole mistral_gpt2_32k vocabulary, f16, into bf16 destinations under a random permutation of the rows: forward()'s rows
    .to(bfloat16), bit for bit — the fused gemm4d destination epilogues at the production head width."""
    cfg, eng, src, ids, lang = headline
    n, E = ids.shape[0], cfg["n_embd"]
    want = eng.forward(ids, src, lang)
    rows = torch.randperm(n, generator=torch.Generator().manual_seed(3)).cuda()
    d_in = torch.empty((n, E), dtype=torch.bfloat16, device="cuda")
    d_out = torch.empty_like(d_in) if eng.dims.separate_out else None
    d_bias = torch.empty((n,), dtype=torch.bfloat16, device="cuda")
    eng.forward_into(ids, src, lang, d_in, d_out, d_bias, rows)
    torch.cuda.synchronize()
    heads = [r for r in eng.gemm_log() if r["epilogue"] & (1024 | 2048)]
    assert heads and all(r["epilogue"] & 1024 and r["variant"] == 7 for r in heads), heads
    for got, ref in zip((d_in, d_out, d_bias), want):
        if ref is None:
            continue
        assert torch.equal(got[rows].view(torch.int16), ref.to(torch.bfloat16).view(torch.int16))


def test_headline_forward_table_into_equals_forward_table(headline):
    """zett_forward_table_into against zett_forward_table on a 4 096-row slice of the headline shape (f16, folded table), bit for bit:
    an fp32 destination under a row map with skipped rows, and a bf16 one."""
    cfg, eng, src, ids, lang = headline
    n, E = 4096, cfg["n_embd"]
    part = ids[:n].contiguous()
    id_slot, id_list, n_ids = eng.table_plan(part)
    table, stats = eng.table_buffers(n_ids)
    eng.table_rows(id_list, 0, n_ids, src, table, stats)
    want = eng.forward_table(part, table, stats, id_slot, lang)
    for k, dtype in enumerate((torch.float32, torch.bfloat16)):
        rows = _rows(n, 20 + k)
        fi, fo, fb = _dest(n, E, dtype, eng.dims.separate_out)
        eng.forward_table_into(part, table, stats, id_slot, lang, fi[:, :E], None if fo is None else fo[:, :E], fb, torch.from_numpy(rows).cuda())
        torch.cuda.synchronize()
        _check_into(want[0], fi, rows, E, dtype, f"table in -> {dtype}")
        if fo is not None:
            _check_into(want[1], fo, rows, E, dtype, f"table out -> {dtype}")
        _check_into(want[2], fb, rows, E, dtype, f"table bias -> {dtype}")


def test_errors():
    cfg = dict(_cfg(), separate_out_embeddings=False)
    w = synth.make_weights(cfg, seed=51)
    src = torch.from_numpy(synth.make_source_embeddings(cfg, 51)).cuda()
    ids = torch.from_numpy(synth.make_surface_forms(cfg, 40, seed=51, n_special=2)).cuda()
    E = cfg["n_embd"]
    eng = _engine(cfg, w, "f16")
    dst = _filled(40, E, torch.float32)
    before = dst.clone()
    rows = torch.arange(40, dtype=torch.int64, device="cuda")
    rows[7] = 40
    with pytest.raises(IndexError):
        eng.forward_into(ids, src, 2, dst, None, None, rows)
    torch.cuda.synchronize()
    assert torch.equal(dst.view(torch.int32), before.view(torch.int32))
    wide = torch.empty((40, 2 * E), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        eng.forward_into(ids, src, 2, wide[:, :E - 4], None, None)          # shape[1] != n_embd
    d = _lib.ZettDest(in_=dst.data_ptr(), dtype=_lib.DTYPE_F32, ld_in=E - 1, n_dest_rows=40)
    import ctypes as C
    i32 = ids.to(torch.int32).contiguous()
    assert eng.lib.zett_forward_into(eng.handle, C.c_void_p(i32.data_ptr()), 40, i32.shape[1], C.c_void_p(src.data_ptr()), 0, src.shape[0], 2,
                                     C.byref(d), None) == _lib.E_INVALID       # ld < E (refused by the library)
    d.ld_in, d.dtype = E, 7
    assert eng.lib.zett_forward_into(eng.handle, C.c_void_p(i32.data_ptr()), 40, i32.shape[1], C.c_void_p(src.data_ptr()), 0, src.shape[0], 2,
                                     C.byref(d), None) == _lib.E_INVALID       # bad dtype
    with pytest.raises(ValueError):
        eng.forward_into(ids, src, 2, torch.empty((40, E), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        eng.forward_into(ids, src, 2, torch.empty((40, E), dtype=torch.float32))          # CPU destination
    eng.close()


def test_f16_destination_overflow_sets_range_dest():
    cfg = _cfg()
    w = synth.make_weights(cfg, seed=61)
    w["scaler.w"] = np.full_like(w["scaler.w"], 3.0e5)          # pred_in beyond 65 504, finite in fp32
    src = torch.from_numpy(synth.make_source_embeddings(cfg, 61)).cuda()
    ids = torch.from_numpy(synth.make_surface_forms(cfg, 300, seed=61, n_special=2)).cuda()
    model = util.hip_model(cfg, w, "f16")
    want = model(ids, source_embeddings=src, lang_index=torch.tensor(2))[0]
    assert model.precision == "f16"
    assert bool(want.isfinite().all()) and float(want.abs().max()) > 65520
    dst = torch.empty(want.shape, dtype=torch.float16, device="cuda")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        model.predict_into(ids, src, 2, out_in=dst, out_out=torch.empty_like(dst) if model.dims.separate_out else None)
    assert any("float16" in str(c.message) for c in caught)
    assert model._last_engine.range_flags() & _lib.RANGE_DEST
    assert model.precision == "f16"
    conv = want.to(torch.float16)
    assert torch.equal(dst.isinf(), conv.isinf()) and torch.equal(dst.view(torch.int16), conv.view(torch.int16))


def test_range_guard_repeats_in_bf16_into_the_same_rows():
    cfg = _cfg()
    w = _massive(synth.make_weights(cfg, seed=71))
    src = torch.from_numpy(synth.make_source_embeddings(cfg, 71)).cuda()
    ids = torch.from_numpy(synth.make_surface_forms(cfg, 300, seed=71, n_special=2)).cuda()
    ref = util.hip_model(cfg, w, "bf16")
    want = ref(ids, source_embeddings=src, lang_index=torch.tensor(2))
    model = util.hip_model(cfg, w, "f16")
    E = cfg["n_embd"]
    rows = _rows(300, 7)
    fi, fo, fb = _dest(300, E, torch.bfloat16, model.dims.separate_out)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        model.predict_into(ids, src, 2, out_in=fi[:, :E], out_out=None if fo is None else fo[:, :E], out_bias=fb, rows=list(rows))
    torch.cuda.synchronize()
    assert model.precision == "bf16"
    _check_into(want[0], fi, rows, E, torch.bfloat16, "in")
    _check_into(want[2], fb, rows, E, torch.bfloat16, "bias")


def test_vocabulary_extension_end_to_end():
    cfg = _cfg()
    w = synth.make_weights(cfg, seed=81)
    src = torch.from_numpy(synth.make_source_embeddings(cfg, 81)).cuda()
    k = 37
    ids = torch.from_numpy(synth.make_surface_forms(cfg, k, seed=81, n_special=2)).cuda()
    model = util.hip_model(cfg, w, "f16")
    V, E = 500, cfg["n_embd"]
    emb = torch.nn.Embedding(V, E).to(device="cuda", dtype=torch.bfloat16)
    old = emb.weight.detach().clone()
    grown = torch.nn.Embedding(V + k, E).to(device="cuda", dtype=torch.bfloat16)       # what resize_token_embeddings does
    with torch.no_grad():
        grown.weight[:V] = emb.weight
    want = model(ids, source_embeddings=src, lang_index=torch.tensor(2))[0]
    with torch.no_grad():
        model.predict_into(ids, src, 2, out_in=grown.weight, out_out=torch.empty_like(grown.weight) if model.dims.separate_out else None,
                           rows=np.arange(V, V + k))
    torch.cuda.synchronize()
    assert torch.equal(grown.weight[:V].view(torch.int16), old.view(torch.int16))
    assert torch.equal(grown.weight[V:].view(torch.int16), want.to(torch.bfloat16).view(torch.int16))
