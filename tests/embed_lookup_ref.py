"""What zett_amd.training.token_embeddings' backward is held to (tests/test_embed_lookup_host.py, tests/test_embed_lookup_gpu.py): the
numpy restatement of its definition, and the input recipe both files share.

THE SUM (include/zett_hip.h, zett_op_embed_lookup_bwd): with p_0 < p_1 < ... the flattened positions that hold id v and C = EMBED_BWD_CHUNK,

    partial_j    = ((g[p_jC] + g[p_jC+1]) + ...) + g[p_jC+C-1]          fp32, ascending positions, the last chunk ragged
    d pred_in[v] = ((partial_0 + partial_1) + ...) + partial_last       fp32, ascending chunks;  no position: zeros

An id outside [0, V) is in no list."""
import functools

import numpy as np
import torch

from zett_amd.training import EMBED_BWD_CHUNK

CASES = ((1, 5, 8), (257, 300, 29), (3000, 97, 64), (3000, 97, 200), (1500, 5000, 1032))          # (T, V, E)


def embed_bwd_ref(ids, g, v, chunk=EMBED_BWD_CHUNK):
    """ids: integers [T]; g: fp32 [T, E] -> fp32 [v, E]."""
    ids = np.asarray(ids).reshape(-1).astype(np.int64)
    g = np.ascontiguousarray(g, dtype=np.float32)
    assert g.shape[0] == ids.shape[0]
    out = np.zeros((v, g.shape[1]), dtype=np.float32)
    order = np.argsort(ids, kind="stable")          # by id, ascending positions within an id
    order = order[(ids[order] >= 0) & (ids[order] < v)]
    sorted_ids = ids[order]
    starts = np.flatnonzero(np.r_[True, sorted_ids[1:] != sorted_ids[:-1]]) if order.size else np.zeros(0, dtype=np.int64)
    ends = np.r_[starts[1:], order.size]
    for lo, hi in zip(starts, ends):
        total = None
        for c0 in range(lo, hi, chunk):
            partial = g[order[c0]].copy()
            for p in order[c0 + 1:min(c0 + chunk, hi)]:
                partial = partial + g[p]
            total = partial if total is None else total + partial
        out[sorted_ids[lo]] = total
    return out


@functools.lru_cache(maxsize=None)
def recipe(t, v, e):
    """(ids int64 [T], g fp32 [T, E]) of a case: a Zipf-like skew, and for T = 3000 planted counts of exactly 64 and 65 and an id that
    never occurs.  Shared between tests: treat as read-only."""
    gen = torch.Generator().manual_seed(1234)
    u = torch.rand(t, generator=gen)
    ids = torch.floor(v * u ** 3).to(torch.int64).clamp_(max=v - 1)
    g = torch.randn(t, e, generator=gen)
    if t == 3000:
        ids[ids >= v - 3] = 0
        low = torch.nonzero(ids < v // 2).reshape(-1)
        ids[low[-64:]] = v - 1
        ids[low[-129:-64]] = v - 2
    return ids, g


def counts(t, v, e):
    return np.bincount(recipe(t, v, e)[0].numpy(), minlength=v)
