"""zett_amd.training.subsample_batch_vocabulary without a GPU: the numpy restatement (tests/batch_vocab_ref.py) against what the
reference's Collator.encode returned (tests/golden/batch_vocab_*.npz), special_row_moves against Python's own del / insert, the host-side
validation that runs before the library is touched, and the C ABI surface of csrc/train_batch.hip."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest
import torch

from tests.batch_vocab_ref import FIXTURES, OUTPUTS, batch_vocab_ref, blank_labels, load_fixture, moves_by_list, recipe
from zett_amd import _lib, training

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zett_op_batch_vocab_workspace_bytes", "zett_op_batch_vocab")


def _ref(inputs, **override):
    a = dict(inputs, **override)
    return batch_vocab_ref(a["input_ids"], a["labels"], a["special_ids"], a["n"], a["surface_forms"], a["priors"], a["mode"], a["negative_order"])


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_equals_the_reference(name):
    inputs, expected = load_fixture(name)
    got = _ref(inputs)
    assert set(expected) == set(OUTPUTS)
    for key in OUTPUTS:
        assert np.array_equal(np.asarray(got[key]), expected[key]), (name, key)
    assert got["target_priors"].dtype == np.float32 and got["mask"].dtype == bool
    assert got["n_positive"] == len(np.union1d(np.union1d(inputs["input_ids"], inputs["labels"]), inputs["special_ids"]))


def test_fixtures_hold_what_the_cases_are_for():
    inputs, expected = load_fixture("batch_vocab_clm_random")
    assert inputs["special_ids"] == [1, 0, 299, 2] and inputs["n"] == 64 and inputs["surface_forms"].shape[0] == 300 and inputs["input_ids"].size == 32
    assert expected["special_indices"].tolist() == [1, 0, 63, 2]          # the special beyond N lands in the last row
    assert np.array_equal(np.sort(inputs["negative_order"]), np.arange(300))
    inputs, expected = load_fixture("batch_vocab_clm_positives_only")
    assert (expected["ids_to_embed"] == 0).sum() > 1          # id 0 repeated, and special: inv[0] is its LAST row
    assert (expected["input_ids"][inputs["input_ids"] == 0] == np.flatnonzero(expected["ids_to_embed"] == 0).max()).all()
    inputs, expected = load_fixture("batch_vocab_mlm_random")
    only = np.setdiff1d(inputs["labels"], inputs["input_ids"])
    assert np.isin([123, 250], only).all() and np.isin(only, expected["ids_to_embed"]).all()          # ids that occur in the labels alone, two of them planted
    inputs, expected = load_fixture("batch_vocab_absent_special_random")
    assert inputs["special_ids"] == [0, 1, 2] and 2 not in inputs["input_ids"] and expected["ids_to_embed"][:3].tolist() == [0, 1, 2]
    for name in FIXTURES:          # the condition under which the product equals the reference
        ids = load_fixture(name)[1]["ids_to_embed"]
        assert (ids >= 0).all() and (name.endswith("positives_only") or len(np.unique(ids)) == len(ids))


@pytest.mark.parametrize("name", FIXTURES)
def test_labels_of_minus_100_are_not_ids(name):
    """The reference lists -100 as an id (np.unique sees it); here the blanked labels change nothing but the labels themselves."""
    inputs, expected = load_fixture(name)
    labels = blank_labels(inputs)
    assert (labels == -100).mean() > 0.5 and (name != "batch_vocab_mlm_random" or np.isin([123, 250], labels).all())
    got = _ref(inputs, labels=labels)
    for key in OUTPUTS:
        want = np.where(labels == -100, -100, expected["labels"]) if key == "labels" else expected[key]
        assert np.array_equal(np.asarray(got[key]), want), (name, key)


def test_special_row_moves_equal_del_and_insert():
    rng = random.Random(5)
    cases = [([0], 4), ([7], 4), ([3, 1, 2], 3), ([2, 0, 1], 3), ([1, 0, 299, 2], 64), ([0, 1, 2, 70000], 4096), ([5, 4], 2), ([63, 64, 62, 0], 64)]
    for _ in range(200):
        k = rng.randint(1, 12)
        n = rng.choice([k, k + 1, k + rng.randint(0, 40)])          # N = number of specials included
        cases.append((rng.sample(range(0, 3 * n + 5), k), n))          # unsorted, some ids >= N
    for special, n in cases:
        moves, where = training.special_row_moves(special, n)
        final, want = moves_by_list(special, n)
        assert where == want, (special, n)
        assert len(moves) == len(special) and all(to == min(s, n - 1) for (_, to), s in zip(moves, sorted(special)))
        # every final row finds its source row by undoing the moves, last move first (what the rows kernel does: the moves that insert at
        # the last row — special ids >= N - 1, the end of the ascending order — only for rows they can touch, the others only below their reach)
        start = list(special) + [-1 - r for r in range(len(special), n)]
        n_low = next((m for m, (_, to) in enumerate(moves) if to >= n - 1), len(moves))
        hi_low = max([max(m) for m in moves[:n_low]], default=-1)
        tail_lo = min([min(m) for m in moves[n_low:]], default=n)

        def undo(q, frm, to):
            if q == to:
                return frm
            q -= 1 if q > to else 0
            return q + (1 if q >= frm else 0)

        for r in range(n):
            q = r
            if r >= tail_lo:
                for frm, to in reversed(moves[n_low:]):
                    q = undo(q, frm, to)
            if q <= hi_low:
                for frm, to in reversed(moves[:n_low]):
                    q = undo(q, frm, to)
            assert start[q] == final[r], (special, n, r)
    with pytest.raises(ValueError, match="twice"):
        training.special_row_moves([1, 2, 1], 8)
    with pytest.raises(ValueError, match="do not fit"):
        training.special_row_moves([1, 2, 3], 2)


def test_validation_runs_before_the_library_is_touched(monkeypatch):
    def untouched(*_a, **_k):
        raise AssertionError("the library was loaded before the arguments were validated")
    monkeypatch.setattr(_lib, "load", untouched)
    v, l = 10, 3
    ids = torch.zeros(2, 4, dtype=torch.int64)
    sf, priors, order = torch.zeros(v, l, dtype=torch.int64), torch.zeros(v), torch.arange(v)
    f = training.subsample_batch_vocabulary
    with pytest.raises(ValueError, match="n_token_subsample = 11"):
        f(ids, ids, [0], v + 1, sf, priors, negative_order=order)
    with pytest.raises(ValueError, match="twice"):
        f(ids, ids, [0, 3, 0], 8, sf, priors, negative_order=order)
    with pytest.raises(ValueError, match="needs negative_order"):
        f(ids, ids, [0], 8, sf, priors)
    with pytest.raises(ValueError, match="int32 / int64"):
        f(ids.float(), ids, [0], 8, sf, priors, negative_order=order)
    with pytest.raises(ValueError, match="int32 / int64"):
        f(ids, ids, [0], 8, sf.float(), priors, negative_order=order)
    with pytest.raises(ValueError, match="same shape"):
        f(ids, ids[:, :3], [0], 8, sf, priors, negative_order=order)
    with pytest.raises(ValueError, match="negative_order must be"):
        f(ids, ids, [0], 8, sf, priors, negative_order=order[:-1])
    with pytest.raises(IndexError, match="special id 10"):
        f(ids, ids, [0, v], 8, sf, priors, negative_order=order)
    with pytest.raises(ValueError, match="do not fit"):
        f(ids, ids, [0, 1, 2], 2, sf, priors, mode="positives_only")
    with pytest.raises(ValueError, match="mode must be"):
        f(ids, ids, [0], 8, sf, priors, mode="highest_scores")
    with pytest.raises(ValueError, match="GPU only"):
        f(ids, ids, [0], 8, sf, priors, negative_order=order)


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "zett_hip.h")).read(), flags=re.S)


@pytest.mark.parametrize("name", NEW)
def test_header_binding_and_library_agree(name):
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


def test_abi_is_additive_and_the_unit_stays_out_of_the_forward_hash():
    from zett_amd import build
    assert "train_batch.hip" in build.SOURCES and "train_batch.hip" in build.TRAINING_ONLY
    assert _lib.ABI_VERSION == 8 and re.search(r"#define ZETT_ABI_VERSION 8\b", open(os.path.join(REPO, "include", "zett_hip.h")).read())
    header = _header()
    for name, value in (("ZETT_BATCH_BAD_ID", 1), ("ZETT_BATCH_OVERFLOW", 2), ("ZETT_BATCH_BAD_ORDER", 4), ("ZETT_BATCH_REPEAT", 8), ("ZETT_BATCH_RANDOM", 1)):
        assert re.search(r"\b%s = %d\b" % (name, value), header), name
    assert (training.BATCH_BAD_ID, training.BATCH_OVERFLOW, training.BATCH_BAD_ORDER, training.BATCH_REPEAT) == (1, 2, 4, 8)


def test_entry_points_refuse_bad_arguments_before_touching_the_device():
    """No GPU needed: nothing is launched."""
    lib = _lib.load()
    P = C.c_void_p
    a, null = C.cast((C.c_int64 * 4096)(), P), P(0)
    i32 = lambda *x: (C.c_int32 * len(x))(*x)          # noqa: E731

    def call(t=8, v=100, n=16, sf_bytes=8, ld=3, l=3, order=a, mode=_lib.BATCH_RANDOM, special=(1, 0), frm=(1, 1), to=(0, 1), k=2, work=a, work_bytes=1 << 15):
        return lib.zett_op_batch_vocab(a, 8, a, 8, t, v, n, a, sf_bytes, ld, l, a, order, 8, mode, i32(*special), i32(*frm), i32(*to), k, a, a, a, a, a, a, a, a, work,
                                       work_bytes, null)

    def refused(rc, code, *words):
        assert rc == code, rc
        msg = lib.zett_last_error().decode()
        assert all(w in msg for w in words), msg

    refused(call(n=101), _lib.E_INVALID, "cannot be filled")
    refused(call(v=0), _lib.E_INVALID, "v > 0")
    refused(call(mode=2), _lib.E_INVALID, "mode")
    refused(call(sf_bytes=2), _lib.E_INVALID, "int32 or int64")
    refused(call(ld=2), _lib.E_INVALID, "ld_sf")
    refused(call(ld=65537, l=65537), _lib.E_INVALID, "l <= 65536")
    refused(call(order=null), _lib.E_INVALID, "null")
    refused(call(special=(1, 100)), _lib.E_INDEX, "special id 100")
    refused(call(special=(1, 1)), _lib.E_INVALID, "twice")
    refused(call(to=(0, 16)), _lib.E_INDEX, "leaves the 16 rows")
    refused(call(k=257), _lib.E_INVALID, "at most 256")
    refused(call(n=1), _lib.E_INVALID, "do not fit")
    need = training.batch_vocab_workspace(8, 100, 16)
    assert need == (2 * 100 + 2 * 16 + 4 * 1 + 4) * 4          # flags and inv over V, two lists of N, counts and offsets of one segment of 1024 ids, totals
    assert training.batch_vocab_workspace(1, 70001, 4096) == (2 * 70001 + 2 * 4096 + 4 * 69 + 4) * 4
    refused(call(work_bytes=need - 4), _lib.E_INVALID, "workspace holds")
    refused(call(work=null), _lib.E_INVALID, "workspace")
    refused(lib.zett_op_batch_vocab_workspace_bytes(8, 100, 101, C.byref(C.c_int64())), _lib.E_INVALID, "cannot be filled")


def test_recipe_is_shared_and_read_only():
    a = recipe(70001, 3000, 7, (0, 1, 2, 70000))
    assert recipe(70001, 3000, 7, (0, 1, 2, 70000))[0] is a[0] and not a[0].flags.writeable
    ids, labels, sf, priors, order = a
    assert (labels == -100).sum() == 375 and len(np.setdiff1d(labels[labels != -100], ids)) >= 1 and np.array_equal(np.sort(order), np.arange(70001))
