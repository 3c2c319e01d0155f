"""zett_amd.training.splice_special_rows / token_embeddings without a GPU: the restatement of the lookup's backward
(tests/embed_lookup_ref.py) against numpy, the properties of the shared input recipe, the host-side validation that runs before the library
is touched, and the C ABI surface of csrc/train_embed.hip."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests.embed_lookup_ref import CASES, counts, embed_bwd_ref, recipe
from zett_amd import _lib, training

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zett_op_splice_rows", "zett_op_embed_lookup", "zett_op_embed_lookup_workspace_bytes", "zett_op_embed_lookup_plan", "zett_op_embed_lookup_bwd")
UPSTREAM = (torch.float32, torch.float16, torch.bfloat16)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _upstream(g, dtype):
    return g.to(dtype).float().numpy()          # what the kernel adds: the incoming gradient converted exactly to fp32


def test_chunk_constant():
    assert training.EMBED_BWD_CHUNK == _lib.EMBED_BWD_CHUNK == 64
    header = open(os.path.join(REPO, "include", "zett_hip.h")).read()
    assert re.search(r"#define ZETT_EMBED_BWD_CHUNK 64\b", header) and re.search(r"#define ZETT_SPLICE_MAX_ROWS 256\b", header)
    assert _lib.SPLICE_MAX_ROWS == 256


@pytest.mark.parametrize("case", CASES)
def test_restatement_is_the_sequential_sum_up_to_one_chunk(case):
    """Wherever every count is <= 64 the definition is np.add.at, bit for bit; beyond, the rows of longer lists may differ and the others not."""
    t, v, e = case
    ids, g = recipe(*case)
    n = counts(*case)
    for dtype in UPSTREAM:
        up = _upstream(g, dtype)
        got = embed_bwd_ref(ids.numpy(), up, v)
        want = np.zeros((v, e), dtype=np.float32)
        np.add.at(want, ids.numpy(), up)
        short = n <= training.EMBED_BWD_CHUNK
        assert np.array_equal(_bits(got[short]), _bits(want[short])), (case, dtype)
        assert not got[n == 0].any()
        if t == 3000:          # the chunked definition and a plain sequential sum are told apart by these cases
            assert (_bits(got) != _bits(want)).any(1).sum() >= 2, (case, dtype)


@pytest.mark.parametrize("case", CASES)
def test_restatement_within_the_bound_of_fp32_summation(case):
    """|sum - float64 sum| <= c 2^-24 sum|g| per element, c the id's count: the standard bound for c - 1 fp32 additions in any order."""
    t, v, e = case
    ids, g = recipe(*case)
    n = counts(*case).astype(np.float64)
    for dtype in UPSTREAM:
        up = _upstream(g, dtype)
        got = embed_bwd_ref(ids.numpy(), up, v).astype(np.float64)
        exact, mass = np.zeros((v, e)), np.zeros((v, e))
        np.add.at(exact, ids.numpy(), up.astype(np.float64))
        np.add.at(mass, ids.numpy(), np.abs(up.astype(np.float64)))
        assert (np.abs(got - exact) <= n[:, None] * 2.0 ** -24 * mass).all(), (case, dtype)


def test_recipe_holds_what_the_cases_are_for():
    n = {case: counts(*case) for case in CASES}
    assert n[(1, 5, 8)].max() == 1 and (n[(1, 5, 8)] == 0).sum() == 4
    assert n[(257, 300, 29)].max() == 36 and (n[(257, 300, 29)] == 0).sum() == 167
    for case in ((3000, 97, 64), (3000, 97, 200)):
        c = n[case]
        assert c[96] == 64 and c[95] == 65 and c[94] == 0 and (c == 0).sum() == 1 and (c == 64).sum() == 2 and (c == 65).sum() == 1
        assert c.max() > 600 and c.max() % 64 != 0 and -(-c.max() // 64) == 10          # ten chunks, the last ragged
    assert n[(1500, 5000, 1032)].max() == 73 and (n[(1500, 5000, 1032)] == 0).sum() == 3950 and (n[(1500, 5000, 1032)] > 64).sum() == 1
    ids, g = recipe(3000, 97, 64)
    assert ids.dtype == torch.int64 and g.dtype == torch.float32 and recipe(3000, 97, 64)[0] is ids          # computed once, shared


def test_restatement_skips_ids_outside_the_table():
    ids = np.array([2, -1, 2, 7, 5, 1 << 31, 2, -100])
    g = np.arange(8 * 3, dtype=np.float32).reshape(8, 3)
    got = embed_bwd_ref(ids, g, 7)
    want = np.zeros((7, 3), dtype=np.float32)
    want[2] = (g[0] + g[2]) + g[6]
    want[5] = g[4]
    assert np.array_equal(got, want)


def test_splice_validation_runs_before_the_library_is_touched(monkeypatch):
    def untouched(*_a, **_k):
        raise AssertionError("the library was loaded before the index lists were validated")
    monkeypatch.setattr(_lib, "load", untouched)
    v, r, e = 10, 6, 4
    pred_in, pred_out, src = torch.zeros(v, e), torch.zeros(v, e), torch.zeros(r, 2 * e)
    with pytest.raises(ValueError, match="twice"):
        training.splice_special_rows(pred_in, pred_out, src, [1, 3, 1], [0, 1, 2])
    with pytest.raises(IndexError, match="special index 10"):
        training.splice_special_rows(pred_in, pred_out, src, np.array([0, v]), np.array([0, 1]))
    with pytest.raises(IndexError, match="special index -1"):
        training.splice_special_rows(pred_in, pred_out, src, [-1], [0])
    with pytest.raises(IndexError, match="reference row 6"):
        training.splice_special_rows(pred_in, pred_out, src, torch.tensor([0, 1]), torch.tensor([0, r]))
    with pytest.raises(ValueError, match="2 entries.*3"):
        training.splice_special_rows(pred_in, pred_out, src, [0, 1], [0, 1, 2])
    with pytest.raises(ValueError, match="output half"):
        training.splice_special_rows(pred_in, pred_out, src[:, :e], [0], [0])
    with pytest.raises(ValueError, match="integers"):
        training.splice_special_rows(pred_in, pred_out, src, [0.5], [0])
    big = torch.zeros(300, e)
    with pytest.raises(ValueError, match="257 entries, at most 256"):
        training.splice_special_rows(big, None, src, list(range(257)), [0] * 257)
    # no special indices: the inputs, as they are
    a, b = training.splice_special_rows(pred_in, None, src, [], np.zeros(0, dtype=np.int64))
    assert a is pred_in and b is None
    rows, refs = training.check_special_indices((3, 0, 9), torch.tensor([5, 0, 2], dtype=torch.int32), v, r)
    assert rows.dtype == refs.dtype == np.int32 and rows.tolist() == [3, 0, 9] and refs.tolist() == [5, 0, 2]


def test_token_embeddings_refuses_before_any_launch():
    pred = torch.zeros(5, 4)
    with pytest.raises(ValueError, match="GPU only"):
        training.token_embeddings(pred, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="pred_in must be"):
        training.token_embeddings(pred.double(), torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="pred_in must be"):
        training.token_embeddings(pred.t(), torch.zeros(3, dtype=torch.int64))


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "zett_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", NEW)
def test_header_binding_and_library_agree(name):
    """Every parameter of the declaration against the ctypes binding: pointers are void* / POINTER, integers by width."""
    assert name in _lib.ABI_SYMBOLS
    params = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, _header(), re.S).group(1)
    fn = getattr(_lib.load(), name)
    want = ["ptr" if "*" in p else {"int64_t": C.c_int64, "int32_t": C.c_int32}[p.split()[0]] for p in (q.strip() for q in params.split(","))]
    assert len(fn.argtypes) == len(want), (name, len(fn.argtypes), len(want))
    for i, (have, w) in enumerate(zip(fn.argtypes, want)):
        if w == "ptr":
            assert have is C.c_void_p or issubclass(have, C._Pointer), (name, i, have)
        else:
            assert C.sizeof(have) == C.sizeof(w) and have(-1).value == -1, (name, i, have)


def test_entry_points_refuse_bad_arguments_before_touching_the_device():
    """No GPU needed: nothing is launched.  The return code says what kind of error, zett_last_error why."""
    lib = _lib.load()
    P = C.c_void_p
    a, null = C.cast((C.c_float * 4096)(), P), P(0)
    i32 = lambda *x: (C.c_int32 * len(x))(*x)          # noqa: E731

    def refused(rc, code, *words):
        assert rc == code, rc
        msg = lib.zett_last_error().decode()
        assert all(w in msg for w in words), msg

    refused(lib.zett_op_splice_rows(null, 0, a, 8, 10, 8, a, _lib.DTYPE_F32, 16, 6, 0, i32(1, 10), i32(0, 1), 2, null), _lib.E_INDEX, "outside [0, 10)")
    refused(lib.zett_op_splice_rows(null, 0, a, 8, 10, 8, a, _lib.DTYPE_F32, 16, 6, 0, i32(1, 2), i32(0, 6), 2, null), _lib.E_INDEX, "source row")
    refused(lib.zett_op_splice_rows(null, 0, a, 8, 10, 8, a, _lib.DTYPE_F32, 16, 6, 0, i32(1, 2, 1), i32(0, 1, 2), 3, null), _lib.E_INVALID, "twice")
    refused(lib.zett_op_splice_rows(null, 0, a, 8, 10, 8, a, _lib.DTYPE_F32, 16, 6, 12, i32(1), i32(0), 1, null), _lib.E_INVALID, "leading dimension")
    refused(lib.zett_op_splice_rows(null, 0, a, 4, 10, 8, a, _lib.DTYPE_F32, 16, 6, 0, i32(1), i32(0), 1, null), _lib.E_INVALID, "leading dimension")
    refused(lib.zett_op_splice_rows(a, 8, a, 8, 10, 8, a, _lib.DTYPE_F32, 16, 6, 0, i32(1), i32(0), 1, null), _lib.E_INVALID, "in place")
    refused(lib.zett_op_splice_rows(null, 0, a, 8, 10, 8, a, 7, 16, 6, 0, i32(1), i32(0), 1, null), _lib.E_INVALID, "dtype")
    assert lib.zett_op_splice_rows(null, 0, a, 8, 10, 8, a, _lib.DTYPE_F32, 16, 6, 0, null, null, 0, null) == 0          # nothing to do
    refused(lib.zett_op_splice_rows(null, 0, a, 8, 300, 8, a, _lib.DTYPE_F32, 16, 6, 0, i32(*range(257)), i32(*[0] * 257), 257, null), _lib.E_INVALID, "at most 256")
    refused(lib.zett_op_embed_lookup(a, 5, 8, 10, 8, a, 8, 4, a, _lib.DTYPE_F32, null, null), _lib.E_INVALID, "dtype")
    refused(lib.zett_op_embed_lookup(a, _lib.DTYPE_F32, 4, 10, 8, a, 8, 4, a, _lib.DTYPE_F32, null, null), _lib.E_INVALID, "ld_table")
    refused(lib.zett_op_embed_lookup(a, _lib.DTYPE_F32, 8, 10, 8, a, 2, 4, a, _lib.DTYPE_F32, null, null), _lib.E_INVALID, "int32 or int64")
    assert lib.zett_op_embed_lookup(a, _lib.DTYPE_F32, 8, 10, 8, a, 8, 0, a, _lib.DTYPE_F32, null, null) == 0
    plan_bytes, scratch_bytes, partial_bytes = training.embed_lookup_workspace(3000, 97, 64)
    assert partial_bytes == (3000 // 32 + 1) * 64 * 4          # fewer than T / 32 chunks belong to lists longer than 64
    assert plan_bytes == (2 * 98 + 3000 + 3000 // 32 + 1) * 4          # all that is held until the backward: offsets, chunk starts, positions, chunk -> id
    assert scratch_bytes == (2 * 97 + 4 * 3000) * 4
    refused(lib.zett_op_embed_lookup_plan(a, 8, 3000, 97, a, plan_bytes - 4, a, scratch_bytes, null), _lib.E_INVALID, "plan holds")
    refused(lib.zett_op_embed_lookup_plan(a, 8, 3000, 97, a, plan_bytes, a, scratch_bytes - 4, null), _lib.E_INVALID, "scratch holds")
    refused(lib.zett_op_embed_lookup_plan(a, 8, 3000, 97, a, plan_bytes, null, scratch_bytes, null), _lib.E_INVALID, "scratch")
    refused(lib.zett_op_embed_lookup_plan(a, 8, 3000, 0, a, plan_bytes, a, scratch_bytes, null), _lib.E_INVALID, "v > 0")
    refused(lib.zett_op_embed_lookup_bwd(a, _lib.DTYPE_F32, 3000, 97, 64, a, plan_bytes, a, partial_bytes - 4, a, 64, null), _lib.E_INVALID, "partials holds")
    refused(lib.zett_op_embed_lookup_bwd(a, _lib.DTYPE_F32, 3000, 97, 64, a, plan_bytes, a, partial_bytes, a, 32, null), _lib.E_INVALID, "ld_d")
    refused(lib.zett_op_embed_lookup_bwd(a, 9, 3000, 97, 64, a, plan_bytes, a, partial_bytes, a, 64, null), _lib.E_INVALID, "dtype")


def test_the_unit_stays_out_of_the_forward_hash():
    from zett_amd import build
    assert "train_embed.hip" in build.SOURCES and "train_embed.hip" in build.TRAINING_ONLY
