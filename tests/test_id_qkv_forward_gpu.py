"""Lever 6 (zett_set_option("id_qkv")) through the whole forward: H = 512, two layers, no language position, 600
rows of seq 7 — the shape of tests/forward_launch_cases.py "h512_nolang" — with "id_qkv" = 2 (whenever possible; the default rule
starts at H = 4096).  The lever is decided from the configuration alone, so what must hold bit for bit is every invariance between
call shapes; against the oracle the outputs keep the f16 tolerance of tests/util.py; with "id_qkv" = 0, or on a configuration with a
language position, nothing differs from the forward without the lever."""
import functools

import numpy as np
import pytest
import torch

from oracle import hypernet_ref
from tests import util
from zett_amd import synth
from zett_amd.dims import HypernetDims

pytestmark = pytest.mark.gpu

SEED, ROWS, H = 11, 600, 512
FOLD_CONSUMER = 1 | 32          # zett_gemm_record.epilogue: a 16-bit output, LayerNorm-fold consumer


def _cfg(lang):
    return dict(synth.workload("tiny")[0], n_embd=128, hn_hidden_size=H, hn_num_attention_heads=8, hn_intermediate_size=1024, hn_n_layers=2, hn_embed_lang_id=lang)


@functools.lru_cache(maxsize=None)
def _setup(lang):
    from zett_amd.hypernet import HipEngine
    cfg = _cfg(lang)
    dev = torch.device("cuda:0")
    w = synth.make_weights(cfg, SEED)
    eng = HipEngine(HypernetDims.from_config(cfg), 1e-5, dev, "f16")
    eng.load_weights({k: torch.from_numpy(v).to(dev) for k, v in w.items()})
    src = synth.make_source_embeddings(cfg, SEED)
    ids = synth.make_surface_forms(cfg, ROWS, seed=SEED, n_special=2)
    return eng, cfg, w, src, ids


DEFAULTS = {"pair_dedupe": 1, "max_chunk_tokens": 1 << 30, "single_rows": 1}


def _run(lang, id_qkv, kind="forward", rows=None, **options):
    """-> (outputs on the CPU, launch log, stats, id_qkv())"""
    eng, cfg, _, src_np, ids_np = _setup(lang)
    for key, value in dict(DEFAULTS, **options).items():
        eng.set_option(key, value)
    eng.set_option("id_qkv", id_qkv)
    src = torch.from_numpy(src_np).cuda()
    ids = torch.from_numpy(ids_np if rows is None else ids_np[rows]).cuda()
    li = 3 if lang else -1
    if kind == "forward":
        outs = eng.forward(ids, src, li)
    elif kind == "shared_table":          # the table of the WHOLE vocabulary, whatever rows the call runs
        id_slot, id_list, n_ids = eng.table_plan(torch.from_numpy(ids_np).cuda())
        table, stats = eng.table_buffers(n_ids)
        eng.table_rows(id_list, 0, n_ids, src, table, stats)
        outs = eng.forward_table(ids, table, stats, id_slot, li)
    else:
        raise KeyError(kind)
    torch.cuda.synchronize()
    assert eng.range_flags() == 0
    log = [(r["m"], r["n"], r["k"], r["variant"], r["epilogue"]) for r in eng.gemm_log()]
    stats = {k: v for k, v in eng.stats().items() if k not in ("gemm_ms", "gemm_flops_timed")}
    return tuple(None if o is None else o.cpu() for o in outs), log, stats, eng.id_qkv()


def _same(got, want, what):
    for g, w, name in zip(got, want, ("pred_in", "pred_out", "bias")):
        assert (g is None) == (w is None) and (g is None or torch.equal(g, w)), f"{what}: {name} differs"


@functools.lru_cache(maxsize=None)
def _taken():
    return _run(False, 2)


def test_lever_is_taken_and_the_launch_log_shows_it():
    _, log, stats, n = _taken()
    _, log0, stats0, n0 = _run(False, 0)
    D, P = stats["distinct_ids"], stats["distinct_positions"]
    assert n == D > 0 and n0 == 0 and P > D
    # layer 0's QKV launch: one fold-consumer launch over the distinct ids instead of the launch over the distinct pairs
    assert (P, 3 * H, H) in [r[:3] for r in log0] and (P, 3 * H, H) not in [r[:3] for r in log]
    mine = [r for r in log if r[:3] == (D, 3 * H, H)]
    assert len(mine) == 1 and mine[0][4] & FOLD_CONSUMER == FOLD_CONSUMER and mine[0][3] == 7
    assert len(log) == len(log0)
    assert stats0["executed_flops"] - stats["executed_flops"] == 2.0 * (P - D) * 3 * H * H
    assert {k: v for k, v in stats.items() if k != "executed_flops"} == {k: v for k, v in stats0.items() if k != "executed_flops"}


def test_outputs_meet_the_f16_tolerance_against_the_oracle():
    eng, cfg, w, src, ids = _setup(False)
    want = hypernet_ref.forward(w, cfg, ids, src)
    got, _, _, _ = _taken()
    keep = ~util.all_pad_rows(cfg, ids)
    for g, r, what in zip(got, want, ("pred_in", "pred_out", "bias")):
        util.CLOSE["f16"](g.numpy()[keep], r[keep], f"id_qkv {what}")


def test_chunks_give_the_same_bits():
    got, _, stats, n = _run(False, 2, max_chunk_tokens=1024)
    assert stats["chunks"] >= 2 and n == _taken()[3]
    _same(got, _taken()[0], "max_chunk_tokens 1024")


def test_pair_dedupe_off_gives_the_same_bits():
    got, log, stats, n = _run(False, 2, pair_dedupe=0)
    assert n == _taken()[3] and stats["distinct_positions"] == stats["packed_tokens"]
    assert (stats["packed_tokens"], 3 * H, H) not in [r[:3] for r in log]
    _same(got, _taken()[0], "pair_dedupe 0")


def test_row_shards_give_the_same_bits():
    want = _taken()[0]
    for s in range(4):
        rows = np.arange(s * ROWS // 4, (s + 1) * ROWS // 4)
        got, _, _, n = _run(False, 2, rows=rows)
        assert n > 0
        _same(got, tuple(None if o is None else o[rows] for o in want), f"shard {s}")


def test_forward_table_gives_the_same_bits():
    got, log, stats, n = _run(False, 2, kind="shared_table")
    assert n == stats["distinct_ids"]
    _same(got, _taken()[0], "zett_forward_table")
    # a row shard on the table of the whole vocabulary: the launch covers the shard's own ids, gathered out of the table
    rows = np.arange(ROWS // 4, ROWS // 2)
    got, _, stats_s, n_s = _run(False, 2, kind="shared_table", rows=rows)
    assert n_s == stats_s["distinct_ids"] < stats["distinct_ids"]
    _same(got, tuple(None if o is None else o[rows] for o in _taken()[0]), "zett_forward_table on a shard")


def test_single_rows_lever_on_top_gives_the_same_bits():
    got, _, _, n = _run(False, 2, single_rows=2)
    eng = _setup(False)[0]
    assert n == _taken()[3] and eng.single_rows() > 0
    _same(got, _taken()[0], "single_rows 2")


def test_default_rule_declines_at_this_width_and_off_is_the_forward_without_the_lever():
    off = _run(False, 0)
    auto = _run(False, 1)
    assert auto[3] == 0 and auto[1] == off[1] and auto[2] == off[2]
    _same(auto[0], off[0], "id_qkv 1 at H = 512")
    eng, _, _, _, ids = _setup(False)
    ws = eng.workspace_bytes(ROWS, ids.shape[1])
    eng.set_option("id_qkv", 2)
    assert eng.workspace_bytes(ROWS, ids.shape[1]) == ws
    # one 16-bit rounding placed elsewhere: the two forwards differ, by little
    a, b = _taken()[0][0].double(), off[0][0].double()
    rel = float((a - b).norm() / b.norm())
    assert 0.0 < rel < util.F16_REL_L2, rel


def test_language_position_declines_the_lever():
    off = _run(True, 0)
    forced = _run(True, 2)
    assert forced[3] == 0 and forced[1] == off[1] and forced[2] == off[2]
    _same(forced[0], off[0], "language position")
    for kind, extra in (("forward", {"max_chunk_tokens": 1024}), ("forward", {"pair_dedupe": 0}), ("shared_table", {})):
        a, b = _run(True, 0, kind, **extra), _run(True, 2, kind, **extra)
        assert b[3] == 0 and a[1] == b[1]
        _same(b[0], a[0], f"language position {kind} {extra}")
