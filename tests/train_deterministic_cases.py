"""The inputs that tests/test_train_deterministic_host.py and tests/test_train_deterministic_gpu.py share (no GPU in here): the index-sum
cases of Ops.index_sum_rows, the ids of the fallback-gradient test, and their references.

THE SUM (include/zett_hip.h, zett_op_embed_lookup_bwd; tests/embed_lookup_ref.py::embed_bwd_ref restates it): per destination the
positions ascending, fp32 partials of 64 positions added left to right, the partials added left to right in ascending chunk order, a
destination with no position zeros.

The addends are randn * 2^k with k uniform in [-12, 12] per element: magnitudes over seven decades, so that a sum taken in another order
differs in its bits with near certainty.  Everything is computed once and shared: treat as read-only."""
import functools

import numpy as np
import torch

from tests.embed_lookup_ref import embed_bwd_ref, recipe

# (T, n_dst, cols, what): the shapes at which the chunking can go wrong
SUM_CASES = (
    (1, 1, 1, "one"),
    (65, 1, 4, "one row, 64 + 1"),
    (4097, 3, 68, "64 * 64 + 1 positions on one index: 65 partials"),
    (3000, 97, 257, "the lookup's recipe: counts of 64 and 65, an index that never occurs, past the 256-column slice"),
    (500, 8, 256, "random"),
    (300, 5, 33, "some indices -1 and n_dst: in no list"),
)


def addends(gen, rows, cols):
    k = torch.randint(-12, 13, (rows, cols), generator=gen)
    return torch.randn(rows, cols, generator=gen) * torch.exp2(k.float())


@functools.lru_cache(maxsize=None)
def sum_case(t, n_dst, cols):
    """-> (idx int32 [T], src fp32 [T, cols], the defined sum fp32 numpy [n_dst, cols])"""
    gen = torch.Generator().manual_seed(1000 * t + cols)
    if (t, n_dst) == (4097, 3):
        idx = torch.ones(t, dtype=torch.int64)
    elif (t, n_dst) == (3000, 97):
        idx = recipe(3000, 97, 64)[0].clone()          # (the ids of the recipe do not depend on its width)
    elif (t, n_dst) == (300, 5):
        idx = torch.randint(-1, n_dst + 1, (t,), generator=gen)
    else:
        idx = torch.randint(0, n_dst, (t,), generator=gen)
    src = addends(gen, t, cols)
    return idx.to(torch.int32), src, embed_bwd_ref(idx.numpy(), src.numpy(), n_dst)


# the fallback gradient: ids around v0
FB_V0, FB_ROWS, FB_T = 20, 6, 400
FB_E_IN = (4, 68, 256)
FB_64, FB_65, FB_NONE = FB_V0 + 1, FB_V0 + 2, FB_V0 + 4          # fallback ids with exactly 64 uses, 65 uses, none


@functools.lru_cache(maxsize=None)
def fallback_ids():
    gen = torch.Generator().manual_seed(77)
    others = torch.tensor(list(range(FB_V0)) + [FB_V0, FB_V0 + 3, FB_V0 + 5])          # v0 - 1 and v0 are both among them
    rest = others[torch.randint(0, others.numel(), (FB_T - 129 - 2,), generator=gen)]
    ids = torch.cat([torch.full((64,), FB_64), torch.full((65,), FB_65), torch.tensor([FB_V0 - 1, FB_V0]), rest])
    return ids[torch.randperm(FB_T, generator=gen)].to(torch.int32)


@functools.lru_cache(maxsize=None)
def fallback_dx(e_in):
    return addends(torch.Generator().manual_seed(e_in), FB_T, e_in)


def bits(a):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
