"""Whole lives of a forward handle, over and over in one process: what tests/test_handle_lifetime_gpu.py measures free device memory
around.  One cycle = create -> load -> finalize -> every kind of call that makes the handle allocate something lazily -> destroy, plus two
handles that fail on the way: one destroyed before zett_finalize with a weight missing, one whose zett_finalize returns ZETT_E_RANGE (f16)."""
import ctypes as C

import pytest
import torch

from tests import forward_launch_cases as cases
from zett_amd import _lib, synth
from zett_amd._glue import ptr, zett_dtypes
from zett_amd.dims import HypernetDims
from zett_amd.hypernet import HipEngine

ROWS = 600
# name -> (config of forward_launch_cases, precision, options, the 16-bit folded table exists)
HANDLES = {
    "tiny": ("tiny", "bf16", {}, False),
    "h512_nolang": ("h512_nolang", "f16", {"id_qkv": 2, "single_rows": 2}, True),
}


def _upload(eng, tensors):
    """zett_load_weight for every tensor, WITHOUT zett_finalize (HipEngine.load_weights calls both)"""
    for name, t in tensors.items():
        shape = (C.c_int64 * t.dim())(*t.shape)
        _lib.check(eng.lib.zett_load_weight(eng.handle, name.encode(), ptr(t), zett_dtypes()[t.dtype], shape, t.dim()), name)


def free_bytes():
    """free device memory as HIP reports it, not counting what torch's allocator holds (it keeps what the tensors of a cycle took)"""
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved()


def cycles(name, n, failing=True, working=True):
    """n cycles on HANDLES[name] -> free_bytes() after each"""
    cfg_name, precision, options, folded_table = HANDLES[name]
    cfg = cases.CONFIGS[cfg_name][0]
    dev = torch.device("cuda:0")
    dims = HypernetDims.from_config(cfg)
    lang = cases.LANG if cfg.get("hn_embed_lang_id") else -1
    weights = {k: torch.from_numpy(v).to(dev) for k, v in synth.make_weights(cfg, cases.SEED).items()}
    operand = "input_projection.0.weight"
    too_large = dict(weights, **{operand: weights[operand] * 1e6})          # beyond the half range
    src = torch.from_numpy(synth.make_source_embeddings(cfg, cases.SEED)).cuda()
    ids = torch.from_numpy(synth.make_surface_forms(cfg, ROWS, seed=cases.SEED, n_special=2)).cuda()
    ids32 = ids.to(torch.int32).contiguous()
    after = []
    for _ in range(n):
        if working:
            eng = HipEngine(dims, 1e-5, dev, precision)
            eng.load_weights(weights)
            for key, value in options.items():
                eng.set_option(key, value)
            eng.forward(ids, src, lang)
            eng.prepare(ids32)
            eng.forward(ids32, src, lang)
            cases._into(eng, ids, src, lang, torch.bfloat16, True, None)          # permuted row map, no bias destination
            id_slot, id_list, n_ids = eng.table_plan(ids)
            table, stats = eng.table_buffers(n_ids)
            if folded_table:
                eng.table_rows(id_list, 0, n_ids, src, table, stats)
                eng.forward_table(ids, table, stats, id_slot, lang)
            else:          # (refused: the handle has no folded table; the plan above was made all the same)
                with pytest.raises(Exception, match="folded"):
                    eng.table_rows(id_list, 0, n_ids, src, table, stats)
                with pytest.raises(Exception, match="folded"):
                    eng.forward_table(ids, table, stats, id_slot, lang)
            eng.set_option("concurrent_lanes", 2)
            eng.forward(ids, src, lang)
            torch.cuda.synchronize()
            eng.close()
        if failing:
            eng = HipEngine(dims, 1e-5, dev, precision)
            _upload(eng, {k: v for k, v in weights.items() if k != operand})
            eng.close()                                     # destroyed before zett_finalize, a weight missing
            eng = HipEngine(dims, 1e-5, dev, "f16")
            with pytest.raises(_lib.RangeError):
                eng.load_weights(too_large)                 # zett_finalize: ZETT_E_RANGE
            eng.close()
        after.append(free_bytes())
    return after
