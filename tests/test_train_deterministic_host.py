"""The order-stable mode of the hypernetwork's backward (ZettHypernet.train_deterministic) without a GPU: the C ABI surface of the
two entry points it adds, their argument validation (nothing is launched), and the definition of its sums on the CPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import train_ops_check as tc
from tests.train_deterministic_cases import FB_64, FB_65, FB_NONE, FB_T, FB_V0, SUM_CASES, fallback_ids, sum_case
from zett_amd import _lib, training

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zett_op_embed_lookup_plan_base", "zett_op_gather_bwd_rows_f32")


def _header(strip_comments=True):
    text = open(os.path.join(REPO, "include", "zett_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip_comments else text


def test_abi_version_is_still_8():
    assert _lib.ABI_VERSION == 8 and _lib.load().zett_abi_version() == 8
    assert re.search(r"#define ZETT_ABI_VERSION 8\b", _header(False))


@pytest.mark.parametrize("name", NEW)
def test_entry_points_are_exported_and_bound_as_declared(name):
    assert name in _lib.ABI_SYMBOLS
    fn = getattr(_lib.load(), name)
    params = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), re.S).group(1)
    want = ["ptr" if "*" in p else {"int64_t": C.c_int64, "int32_t": C.c_int32}[p.split()[0]] for p in (q.strip() for q in params.split(","))]
    assert len(fn.argtypes) == len(want), (name, len(fn.argtypes), len(want))
    for i, (have, w) in enumerate(zip(fn.argtypes, want)):
        if w == "ptr":
            assert have is C.c_void_p or issubclass(have, C._Pointer), (name, i, have)
        else:
            assert C.sizeof(have) == C.sizeof(w) and have(-1).value == -1, (name, i, have)


def test_the_units_stay_out_of_the_forward_hash():
    from zett_amd import build
    assert {"train_embed.hip", "train_gather.hip"} <= set(build.TRAINING_ONLY)


def test_entry_points_refuse_bad_arguments_before_touching_the_device():
    """No GPU needed: nothing is launched.  Every refusal is ZETT_E_INVALID and zett_last_error says why."""
    lib = _lib.load()
    P = C.c_void_p
    a, null = C.cast((C.c_float * 4096)(), P), P(0)
    t, v = 3000, 97
    plan_bytes, scratch_bytes, _ = training.embed_lookup_workspace(t, v, 64)

    def refused(rc, *words):
        assert rc == _lib.E_INVALID, rc
        msg = lib.zett_last_error().decode()
        assert all(w in msg for w in words), msg

    plan = lambda **k: lib.zett_op_embed_lookup_plan_base(*[k.get(n, d) for n, d in (          # noqa: E731
        ("ids", a), ("ids_bytes", 4), ("t", t), ("id_base", 20), ("v", v), ("plan", a), ("plan_bytes", plan_bytes), ("scratch", a), ("scratch_bytes", scratch_bytes),
        ("stream", null))])
    refused(plan(ids=null), "ids")
    refused(plan(ids_bytes=2), "int32 or int64")
    refused(plan(ids_bytes=0), "int32 or int64")
    refused(plan(t=-1), "t >= 0")
    refused(plan(v=0), "v > 0")
    refused(plan(v=-3), "v > 0")
    refused(plan(plan=null), "plan")
    refused(plan(plan_bytes=plan_bytes - 4), "plan holds")
    refused(plan(scratch=null), "scratch")
    refused(plan(scratch_bytes=scratch_bytes - 4), "scratch holds")
    # the ids of the rows, [id_base, id_base + v), must be 32-bit values
    refused(plan(id_base=2 ** 31 - v + 1), "32-bit")
    refused(plan(id_base=2 ** 31), "32-bit")
    refused(plan(id_base=-2 ** 31 - 1), "32-bit")
    refused(plan(id_base=2 ** 63 - 1), "32-bit")
    refused(plan(id_base=-2 ** 63), "32-bit")

    gather = lambda **k: lib.zett_op_gather_bwd_rows_f32(*[k.get(n, d) for n, d in (          # noqa: E731
        ("ids", a), ("n", 40), ("src", a), ("dtype", _lib.DTYPE_F32), ("e_in", 8), ("v0", 11), ("dx", a), ("prod", a), ("keep", a), ("stream", null))])
    for name in ("ids", "src", "dx", "prod", "keep"):
        refused(gather(**{name: null}), "null")
    refused(gather(dtype=7), "dtype")
    refused(gather(n=-1), "n_tokens")
    refused(gather(e_in=0), "e_in")
    refused(gather(e_in=-4), "e_in")
    refused(gather(v0=-1), "v0")
    assert gather(n=0) == 0          # nothing to do: no launch


@pytest.mark.parametrize("case", SUM_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
def test_the_defined_sum_is_within_the_any_order_bound_of_the_float64_sum(case):
    """embed_bwd_ref on the shared recipe (addends over seven decades) against the float64 sum, per element, under
    train_ops_check.sum_bound with n the destination's count — the bound the atomic sums are held to."""
    t, n_dst, cols, _ = case
    idx, src, want = sum_case(t, n_dst, cols)
    inside = (idx >= 0) & (idx < n_dst)
    i64 = idx[inside].long()
    exact = torch.zeros(n_dst, cols, dtype=torch.float64).index_add_(0, i64, src[inside].double())
    mag = torch.zeros(n_dst, cols, dtype=torch.float64).index_add_(0, i64, src[inside].double().abs())
    n = torch.bincount(i64, minlength=n_dst).double()[:, None]
    err = (torch.from_numpy(want).double() - exact).abs()
    assert bool((err <= tc.sum_bound(n, mag)).all())
    assert not want[(n == 0).reshape(-1).numpy()].any()
    if t >= 500:          # the recipe tells orders apart: a plain left-to-right sum gives other bits somewhere
        plain = np.zeros((n_dst, cols), dtype=np.float32)
        np.add.at(plain, i64.numpy(), src[inside].numpy())
        assert (plain.view(np.int32) != want.view(np.int32)).any()


def test_the_shared_cases_hold_what_they_are_for():
    count = lambda t, n, c: np.bincount(sum_case(t, n, c)[0].numpy().clip(-1) + 1, minlength=n + 2)          # noqa: E731 ([0]: the -1s)
    assert count(4097, 3, 68).tolist() == [0, 0, 4097, 0, 0]
    c = count(3000, 97, 257)[1:98]
    assert c[96] == 64 and c[95] == 65 and c[94] == 0 and c.max() > 600
    c = count(300, 5, 33)
    assert c[0] > 0 and c[6] > 0 and c[1:6].min() > 0          # -1 and n_dst both occur
    ids = fallback_ids()
    n = np.bincount(ids.numpy(), minlength=FB_V0 + 6)
    assert ids.numel() == FB_T and n[FB_64] == 64 and n[FB_65] == 65 and n[FB_NONE] == 0 and n[FB_V0 - 1] >= 1 and n[FB_V0] >= 1
