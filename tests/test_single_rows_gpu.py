"""Lever 5: a vocabulary row with a single kept position attends to exactly one key, so its context is its own
value row and its query / key GEMM rows are skipped.  zett_set_option("single_rows", 2) against 0 must give the same bytes in all
three outputs through every entry point and option that touches the position-0 block, the launch log must lose exactly the skipped
rows, and under the default rule (auto) nothing may move at these sizes.

Shapes: H = 256, 4 heads, I = 512, seq 7, 600 rows (the smallest that reach the packed attention waves, the row kernels' rows8 path and
more than one 256-row tile), with 3, 2 and 1 encoder layers (a middle layer and the last; the last behind the per-pair one; only the
position-0-only layer).  H = 512 in addition: the LayerNorm fold, the 16-bit residual stream and the folded table (the shared-table
entry exists there only), whose per-row statistics the skipping launches offset."""
import functools

import numpy as np
import pytest
import torch

from zett_amd import synth
from zett_amd.dims import HypernetDims

pytestmark = pytest.mark.gpu

SEED = 23
ROWS = 600


def _cfg(hidden, heads, inter, layers, lang=False):
    return dict(synth.workload("tiny")[0], n_embd=128, hn_hidden_size=hidden, hn_num_attention_heads=heads, hn_intermediate_size=inter,
                hn_n_layers=layers, hn_embed_lang_id=lang)


SHAPES = {"h256": (256, 4, 512), "h512": (512, 8, 1024)}
DEFAULTS = {"pair_dedupe": 1, "cls_only_last_layer": 1, "ln_fold": 1}


@functools.lru_cache(maxsize=None)
def _engine(shape, layers, precision, lang=False, chunk=0):
    from zett_amd.hypernet import HipEngine
    cfg = _cfg(*SHAPES[shape], layers, lang)
    dev = torch.device("cuda:0")
    eng = HipEngine(HypernetDims.from_config(cfg), 1e-5, dev, precision)
    eng.load_weights({k: torch.from_numpy(v).to(dev) for k, v in synth.make_weights(cfg, SEED).items()})
    if chunk:
        eng.set_option("max_chunk_tokens", chunk)
    return eng, cfg, torch.from_numpy(synth.make_source_embeddings(cfg, SEED)).cuda()


@functools.lru_cache(maxsize=None)
def _default_ids():
    return synth.make_surface_forms(_cfg(256, 4, 512, 3), ROWS, seed=SEED, n_special=2)


def _ids_of_lengths(lengths, seq=7):
    """Surface forms with the given number of kept positions per row (ids drawn like synth.make_surface_forms draws them)."""
    cfg = _cfg(256, 4, 512, 3)
    lengths = np.asarray(lengths)
    full = synth.make_surface_forms(cfg, len(lengths), seed=SEED + 1, hist=(0.0,) * (seq - 1) + (1.0,), seq=seq)
    return np.where(np.arange(seq)[None, :] < lengths[:, None], full, cfg["pad_token_id"]).astype(np.int32)


def _singles(ids, cfg):
    """Rows the plan keeps one position of: one id that is not the pad, in column 0, and no language token."""
    if cfg["hn_embed_lang_id"] or ids.shape[1] < 2:
        return 0
    kept = ids != cfg["pad_token_id"]
    return int((kept.sum(1) == 1)[kept[:, 0]].sum())


def _run(eng, cfg, src, ids_np, single, kind="forward", **options):
    """One forward with "single_rows" = single -> (outputs, launch log, stats, single_rows())."""
    for key, value in dict(DEFAULTS, **options).items():
        eng.set_option(key, value)
    eng.set_option("single_rows", single)
    ids = torch.from_numpy(ids_np).cuda()
    lang = 3 if cfg["hn_embed_lang_id"] else -1
    n, d = ids.shape[0], eng.dims
    if kind == "forward":
        outs = eng.forward(ids, src, lang)
    elif kind == "into":          # a permuted bf16 destination with its own row map, two rows of it skipped
        rows = np.random.default_rng(SEED).permutation(n + 7)[:n].astype(np.int64)
        rows[[0, n // 2]] = -1
        outs = tuple(torch.zeros(shape, dtype=dt, device=eng.device) for shape, dt in
                     (((n + 7, d.n_embd), torch.bfloat16), ((n + 7, d.n_embd), torch.bfloat16), ((n + 7,), torch.float32)))
        eng.forward_into(ids, src, lang, outs[0], outs[1], outs[2], torch.from_numpy(rows).cuda())
    elif kind == "into_identity":          # no row map, no bias: the map is the position-0 block's own, the bias goes to the sink
        outs = tuple(torch.zeros((n, d.n_embd), dtype=torch.float16, device=eng.device) for _ in range(2))
        eng.forward_into(ids, src, lang, outs[0], outs[1], None, None)
    elif kind == "shared_table":
        id_slot, id_list, n_ids = eng.table_plan(ids)
        table, stats = eng.table_buffers(n_ids)
        eng.table_rows(id_list, 0, n_ids, src, table, stats)
        outs = eng.forward_table(ids, table, stats, id_slot, lang)
    elif kind == "prepared":
        first = ids.to(torch.int32).contiguous()
        eng.prepare(first)
        outs = eng.forward(first, src, lang)
    else:
        raise KeyError(kind)
    torch.cuda.synchronize()
    assert eng.range_flags() == 0
    log = [(r["m"], r["n"], r["k"], r["variant"], r["epilogue"], r["flops"]) for r in eng.gemm_log()]
    stats = {k: v for k, v in eng.stats().items() if k not in ("gemm_ms", "gemm_flops_timed")}
    return outs, log, stats, eng.single_rows()


def _assert_same_outputs(got, want, what):
    assert len(got) == len(want)
    for g, w, name in zip(got, want, ("pred_in", "pred_out", "bias")):
        assert torch.equal(g, w), f"{what}: {name} differs"


def test_the_workload_has_single_rows():
    """(CPU) 10-30 % of the rows keep one position: what the lever acts on at these sizes."""
    ids, cfg = _default_ids(), _cfg(256, 4, 512, 3)
    assert 0.10 * ROWS <= _singles(ids, cfg) <= 0.30 * ROWS
    assert _singles(ids, _cfg(256, 4, 512, 3, lang=True)) == 0 and _singles(ids[:, :1], cfg) == 0


VARIANTS = {
    "default": ("forward", {}),
    "nopairs": ("forward", {"pair_dedupe": 0}),
    "all_positions": ("forward", {"cls_only_last_layer": 0}),
    "all_positions_nopairs": ("forward", {"cls_only_last_layer": 0, "pair_dedupe": 0}),
    "ln_fold0": ("forward", {"ln_fold": 0}),
    "into": ("into", {}),
    "into_identity": ("into_identity", {}),
    "prepared": ("prepared", {}),
}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("layers", (3, 2, 1))
@pytest.mark.parametrize("precision", ("f32", "f16", "bf16"))
def test_forced_lever_gives_the_same_bytes(precision, layers, variant):
    eng, cfg, src = _engine("h256", layers, precision)
    kind, options = VARIANTS[variant]
    ids = _default_ids()
    want, _, _, off = _run(eng, cfg, src, ids, 0, kind, **options)
    got, _, _, on = _run(eng, cfg, src, ids, 2, kind, **options)
    assert off == 0 and on == _singles(ids, cfg)
    _assert_same_outputs(got, want, f"{precision} L{layers} {variant}")


# (the folded table, and so the shared-table entry, exists with the 16-bit residual stream: f16)
@pytest.mark.parametrize("precision,variant", [(p, v) for p in ("f16", "bf16") for v in sorted(VARIANTS)] + [("f16", "shared_table")])
@pytest.mark.parametrize("layers", (3, 1))
def test_forced_lever_gives_the_same_bytes_with_the_fold(precision, layers, variant):
    """H = 512: the fold's consumers read per-row statistics, the 16-bit stream and (f16) the folded table."""
    eng, cfg, src = _engine("h512", layers, precision)
    kind, options = ("shared_table", {}) if variant == "shared_table" else VARIANTS[variant]
    ids = _default_ids()
    want, _, _, _ = _run(eng, cfg, src, ids, 0, kind, **options)
    got, _, _, on = _run(eng, cfg, src, ids, 2, kind, **options)
    assert on == _singles(ids, cfg)
    _assert_same_outputs(got, want, f"h512 {precision} L{layers} {variant}")


EDGES = {
    "no_single_row": np.tile([2, 3, 7, 4], 40),
    "every_row_single": np.ones(300, dtype=np.int64),
    "singles_first": np.r_[np.ones(100, dtype=np.int64), np.tile([2, 5, 3], 60)],
    "singles_last": np.r_[np.tile([2, 5, 3], 60), np.ones(100, dtype=np.int64)],
    "one_single_row": np.array([1]),
    "one_longer_row": np.array([3]),
    "one_single_among_many": np.r_[np.tile([4, 2], 150), [1], np.tile([3], 20)],
}


@pytest.mark.parametrize("edge", sorted(EDGES))
@pytest.mark.parametrize("precision", ("f32", "f16"))
def test_edge_inputs(precision, edge):
    lengths = EDGES[edge]
    ids = _ids_of_lengths(lengths)
    for shape, layers in (("h256", 3), ("h256", 1), ("h512", 3)):
        if shape == "h512" and precision == "f32":
            continue
        eng, cfg, src = _engine(shape, layers, precision)
        want, log0, _, _ = _run(eng, cfg, src, ids, 0)
        got, log2, _, on = _run(eng, cfg, src, ids, 2)
        assert on == int((lengths == 1).sum()) == _singles(ids, cfg)
        if on == 0:
            assert log2 == log0
        _assert_same_outputs(got, want, f"{precision} {shape} L{layers} {edge}")


@pytest.mark.parametrize("precision", ("f32", "f16", "bf16"))
def test_the_lever_is_off_where_no_row_can_be_single_or_the_call_is_not_one_chunk(precision):
    ids = _default_ids()
    cases = (("language token", _engine("h256", 3, precision, True), ids),
             ("seq = 1", _engine("h256", 3, precision), np.ascontiguousarray(ids[:, :1])),
             ("two chunks", _engine("h256", 3, precision, False, 1024), ids),
             ("two lanes", _engine("h256", 3, precision), ids))
    for what, (eng, cfg, src), x in cases:
        extra = {"concurrent_lanes": 2} if what == "two lanes" else {}
        want, log0, stats0, _ = _run(eng, cfg, src, x, 0, **extra)
        got, log2, stats2, on = _run(eng, cfg, src, x, 2, **extra)
        if extra:
            eng.set_option("concurrent_lanes", 0)
        assert on == 0 and log2 == log0 and stats2 == stats0, what
        if what == "two chunks":
            assert stats0["chunks"] == 2
        _assert_same_outputs(got, want, f"{precision} {what}")


@pytest.mark.parametrize("pairs", (1, 0))
@pytest.mark.parametrize("layers", (3, 2, 1))
@pytest.mark.parametrize("precision", ("f32", "f16", "bf16"))
def test_launch_log_under_force(precision, layers, pairs):
    """The Q|K launch of a middle layer has m - n_s rows, the last layer's query launch rows - n_s, and the executed FLOPs fall by
    exactly n_s * 2H * H * 2 per middle layer (not the per-pair one) and n_s * 2H * H * 2 in the last."""
    eng, cfg, src = _engine("h256", layers, precision)
    ids, H = _default_ids(), 256
    _, log0, stats0, _ = _run(eng, cfg, src, ids, 0, pair_dedupe=pairs)
    _, log2, stats2, n_s = _run(eng, cfg, src, ids, 2, pair_dedupe=pairs)
    m, rows = stats0["packed_tokens"], stats0["rows"]
    assert n_s == _singles(ids, cfg) > 0 and eng.single_rows() == n_s
    by_pair = stats0["distinct_positions"] != m          # layer 0 ran per distinct pair: unchanged
    assert by_pair == bool(pairs and layers >= 2)
    middle = layers - 1 - (1 if by_pair else 0)
    shapes = [r[:3] for r in log2]
    assert shapes.count((m - n_s, 2 * H, H)) == middle and shapes.count((m, 3 * H, H)) == 0
    assert shapes.count((rows - n_s, H, H)) >= 1 and (m - n_s, H, H) in shapes          # the last layer's query and key launches
    assert len(log2) == len(log0) + middle + 1
    saved = sum(r[5] for r in log0) - sum(r[5] for r in log2)
    assert saved == n_s * 2 * H * H * 2 * (middle + 1)
    assert stats0["executed_flops"] - stats2["executed_flops"] == saved
    assert {k: v for k, v in stats2.items() if k not in ("executed_flops", "gemm_launches")} == \
           {k: v for k, v in stats0.items() if k not in ("executed_flops", "gemm_launches")}


@pytest.mark.parametrize("precision", ("f32", "f16", "bf16"))
def test_auto_changes_nothing_at_these_sizes(precision):
    """floor(n_s / 256) * (2H / 256) is 0 here, far from the 256 CUs of a round: the log, stats() and workspace_bytes() of the default are
    those of the lever switched off."""
    for shape in ("h256", "h512") if precision != "f32" else ("h256",):
        eng, cfg, src = _engine(shape, 3, precision)
        ids = _default_ids()
        want, log0, stats0, _ = _run(eng, cfg, src, ids, 0)
        ws0 = eng.workspace_bytes(ROWS, ids.shape[1])
        got, log1, stats1, on = _run(eng, cfg, src, ids, 1)
        assert on == 0 and log1 == log0 and stats1 == stats0 and eng.workspace_bytes(ROWS, ids.shape[1]) == ws0
        eng.set_option("single_rows", 2)
        assert eng.workspace_bytes(ROWS, ids.shape[1]) == ws0
        _assert_same_outputs(got, want, f"{precision} {shape} auto")
