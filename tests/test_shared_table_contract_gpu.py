"""The contract of the hoisted table shared between ranks (ABI 8: zett_table_plan / zett_table_rows / zett_forward_table[_into],
sharding.SharedTable, the job table of transfer.predict_vocabulary) at its BOUNDARIES.  tests/test_invariants_gpu.py pins the happy
case — a complete, correctly built table gives zett_forward's bits; here the table is not what the forward assumes:

  A1  an id the table's matrix never referenced is refused (IndexError, ZETT_E_INDEX, its own message, the row's number, nothing
      written) in both slot modes — plan_tokens_kernel reads the caller's id_slot (h512, id_qkv 0), lever 6's gather does (h512_nolang,
      id_qkv 2) — and what is valid stays accepted, bit for bit;
  A2  whether a handle builds table rows does not depend on the slice asked for: an empty slice is refused exactly when a full one is;
  A3  a table of 3 ids over 8 ranks: every rank's construction fills the same table or raises, none returns alone;
  A4  the range bits the table's build raised survive the forwards on it (SharedTable.range_flags; the accumulating word of a job);
  A5  predict_vocabulary decides "table or no table" from the engine, and an error of the build propagates;
  A6  forward_table[_into] refuse a table / stats / id_slot of the wrong type, shape, layout or device before any library call.

Every comparison is bit for bit, an error code or a flag word: there is no tolerance.  The restatement of "referenced" is numpy's, the
formula tests/test_invariants_gpu.py holds zett_table_plan to.  In every negative case of A1 the table is allocated with n_ids + 5 rows
(filled), so every slot a library WITHOUT the refusal would read — the next id's, or n_ids — lies inside the allocation."""
import re

import numpy as np
import pytest
import torch

from tests import forward_launch_cases as flc
from zett_amd import _glue, _lib, synth
from zett_amd.dims import HypernetDims

pytestmark = pytest.mark.gpu

N_ROWS = 600
LANG = flc.LANG
ARMS = {"direct_slots": ("h512", 0), "id_qkv_gather": ("h512_nolang", 2)}      # arm -> (config, "id_qkv")


def referenced(m, pad):
    """the ids a forward over the matrix looks up: position 0 and every visible position (all positions of an all-pad row are the pad id)"""
    return np.unique(np.concatenate([m[m != pad], m[:, 0]]))


def _eq(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Arm:
    """One engine with a table planned from P — the seeded matrix with id_mid and id_top written out of it — and the reference bits."""

    def __init__(self, cfg_name, id_qkv):
        self.cfg, _ = flc.CONFIGS[cfg_name]
        d = HypernetDims.from_config(self.cfg)
        self.pad, self.V, self.E, self.separate_out = d.pad_token_id, d.original_vocab_size + d.n_extra, d.n_embd, d.separate_out
        self.lang = LANG if self.cfg.get("hn_embed_lang_id") else -1
        self.eng = flc._engine(self.cfg, "f16")
        self.eng.set_option("id_qkv", id_qkv)
        self.src = _cuda(synth.make_source_embeddings(self.cfg, flc.SEED))
        m = synth.make_surface_forms(self.cfg, N_ROWS, seed=flc.SEED)
        refs = referenced(m, self.pad)
        assert self.pad not in refs and len(refs) > 8          # (no all-pad row, pad never at position 0: the pad id is NOT in the table)
        self.id_top, self.id_mid = int(refs[-1]), int(refs[len(refs) // 2])
        p = m.copy()
        p[p == self.id_top] = refs[1]
        p[p == self.id_mid] = refs[2]
        self.P = p
        self.refP = referenced(p, self.pad)
        assert set(refs) - set(self.refP) == {self.id_mid, self.id_top} and self.refP[0] < self.id_mid < self.refP[-1] < self.id_top < self.V
        self.ids = _cuda(p)
        self.id_slot, self.id_list, self.n = self.eng.table_plan(self.ids)
        assert self.n == len(self.refP) and np.array_equal(self.id_list.cpu().numpy(), self.refP)
        self.table, self.stats = self.eng.table_buffers(self.n + 5)          # (the slack every negative case relies on)
        self.table.fill_(float("nan")); self.stats.fill_(float("nan"))
        self.eng.table_rows(self.id_list, 0, self.n, self.src, self.table, self.stats)
        self.ref = self.forward(self.ids)
        self.long_row = int(np.flatnonzero((p != self.pad).sum(1) >= 3)[4])          # a row with visible positions 1 and 2

    def forward(self, ids):
        out = self.eng.forward(ids, self.src, self.lang)
        torch.cuda.synchronize()
        return out

    def forward_table(self, ids):
        out = self.eng.forward_table(ids, self.table, self.stats, self.id_slot, self.lang)
        torch.cuda.synchronize()
        return out

    def planted(self, q):
        return set(referenced(q, self.pad).tolist()) - set(self.refP.tolist())

    def return_code(self, ids32):
        """zett_forward_table's own return code and message"""
        n, seq = ids32.shape
        out_in = torch.empty((n, self.E), device="cuda")
        out_out = torch.empty((n, self.E), device="cuda") if self.separate_out else None
        out_bias = torch.empty((n,), device="cuda")
        ptr = _glue.ptr
        rc = self.eng.lib.zett_forward_table(self.eng.handle, ptr(ids32), n, seq, ptr(self.table), ptr(self.stats), ptr(self.id_slot), self.lang,
                                             ptr(out_in), ptr(out_out), ptr(out_bias), _glue.stream(self.eng.device))
        return rc, self.eng.lib.zett_last_error().decode()

    def destinations(self, n):
        """(fp32 identity destination, bf16 destination behind a row map), canary-filled, as forward_table_into arguments"""
        def mats(rows, dtype, bias_dtype):
            return (torch.full((rows, self.E), 7.25, dtype=dtype, device="cuda"),
                    torch.full((rows, self.E), -3.5, dtype=dtype, device="cuda") if self.separate_out else None,
                    torch.full((rows,), 0.625, dtype=bias_dtype, device="cuda"))
        rowmap = _cuda(np.random.default_rng(3).permutation(n + 7)[:n].astype(np.int64))
        return [(mats(n, torch.float32, torch.float32), None), (mats(n + 7, torch.bfloat16, torch.float32), rowmap)]


@pytest.fixture(scope="module", params=sorted(ARMS))
def arm(request):
    a = Arm(*ARMS[request.param])
    yield a
    a.eng.close()


def _negative_cases(a):
    """name -> (Q, offending row, planted id): P with exactly one row that references an id the table does not hold"""
    r = a.long_row
    cases = {}
    q = a.P.copy(); q[r, 1] = a.id_mid; cases["mid_visible"] = (q, r, a.id_mid)
    q = a.P.copy(); q[r + 1, 0] = a.id_mid; cases["mid_position0"] = (q, r + 1, a.id_mid)
    q = a.P.copy(); q[r + 2, 0] = a.id_top; cases["top"] = (q, r + 2, a.id_top)          # slot == n_ids: the row BEHIND the table
    q = a.P.copy()
    if a.lang < 0:
        q[r + 3, :] = a.pad          # an all-pad row: without a language position it attends uniformly, every position is looked up
    else:
        q[r + 3, 0] = a.pad          # pad at position 0 is a query
    cases["pad"] = (q, r + 3, a.pad)
    return cases


@pytest.mark.parametrize("case", ["mid_visible", "mid_position0", "top", "pad"])
def test_an_id_absent_from_the_table_is_refused(arm, case):
    a = arm
    q, row, planted = _negative_cases(a)[case]
    assert a.planted(q) == {planted} and np.flatnonzero((q != a.P).any(1)).tolist() == [row]          # (CPU: exactly the planted id, in one row)
    assert a.table.shape[0] >= a.n + 1 and a.stats.shape[0] >= a.n + 1
    ids = _cuda(q)

    def refused(err):
        msg = str(err)
        assert "not in the table" in msg and "outside [0" not in msg, msg
        assert [int(x) for x in re.findall(r"row (\d+)", msg)] == [row], msg

    rc, msg = a.return_code(ids)
    assert rc == _lib.E_INDEX, (rc, msg)
    refused(msg)
    with pytest.raises(IndexError) as e:
        a.eng.forward_table(ids, a.table, a.stats, a.id_slot, a.lang)
    refused(e.value)
    for (out_in, out_out, out_bias), rowmap in a.destinations(len(q)):
        before = [None if t is None else t.clone() for t in (out_in, out_out, out_bias)]
        with pytest.raises(IndexError) as e:
            a.eng.forward_table_into(ids, a.table, a.stats, a.id_slot, a.lang, out_in, out_out, out_bias, rowmap)
        refused(e.value)
        torch.cuda.synchronize()
        assert _eq((out_in, out_out, out_bias), before), "a refused call wrote into its destination"
    # the engine is as good as before: on the table, on the source embeddings, and behind a prepared plan
    assert _eq(a.forward_table(a.ids), a.ref)
    assert _eq(a.forward(a.ids), a.ref)
    a.eng.prepare(a.ids)
    assert _eq(a.forward(a.ids), a.ref)


def test_valid_calls_on_the_table_stay_accepted(arm):
    a = arm
    taken = a.eng.id_qkv
    # pad at positions j > 0 only, pad absent from the table: such a position is never looked up
    assert a.planted(a.P) == set() and (a.P[:, 1:] == a.pad).any() and a.pad not in a.refP
    got = a.forward_table(a.ids)
    assert (taken() > 0) == (a.lang < 0), "the arm does not read id_slot where it claims to"
    assert _eq(got, a.ref)
    lo, hi = 137, 401
    assert a.planted(a.P[lo:hi]) == set()
    assert _eq(a.forward_table(a.ids[lo:hi].contiguous()), [None if t is None else t[lo:hi] for t in a.ref])
    perm = np.random.default_rng(5).permutation(N_ROWS)
    assert a.planted(a.P[perm]) == set()
    at = torch.from_numpy(perm).cuda()
    assert _eq(a.forward_table(_cuda(a.P[perm])), [None if t is None else t[at] for t in a.ref])
    # an id outside the vocabulary keeps its own message — also beside an absent id in a later row
    for extra in (None, a.id_mid):
        q = a.P.copy(); q[9, 1] = a.V
        if extra is not None:
            q[300, 0] = extra
        rc, msg = a.return_code(_cuda(q))
        assert rc == _lib.E_INDEX and "outside [0" in msg and "not in the table" not in msg and "row 9 " in msg, msg
    with pytest.raises(IndexError, match=r"outside \[0"):
        a.eng.forward_table(_cuda(q), a.table, a.stats, a.id_slot, a.lang)
    assert _eq(a.forward_table(a.ids), a.ref)


# ---- A2: the mode refusal does not depend on the slice ------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg_name,precision,options,folded", [
    ("h512", "f16", {}, True), ("h512", "bf16", {}, False), ("h512", "f32", {}, False), ("h512", "f16", {"table_lo": 0}, False),
    ("h512", "f16", {"ln_fold": 0}, False), ("tiny", "f16", {}, False)])
def test_the_mode_refusal_does_not_depend_on_the_slice(cfg_name, precision, options, folded):
    cfg, _ = flc.CONFIGS[cfg_name]
    eng = flc._engine(cfg, precision)
    for key, value in options.items():
        eng.set_option(key, value)
    src = _cuda(synth.make_source_embeddings(cfg, flc.SEED))
    ids = _cuda(synth.make_surface_forms(cfg, 64, seed=flc.SEED))
    _, id_list, n = eng.table_plan(ids)
    hidden = HypernetDims.from_config(cfg).hidden
    table = torch.zeros((n, hidden), dtype=torch.bfloat16 if precision == "bf16" else torch.float16, device="cuda")
    stats = torch.zeros((n, 2), device="cuda")

    def raises(first, count):
        try:
            eng.table_rows(id_list, first, count, src, table, stats)
        except ValueError:
            return True
        torch.cuda.synchronize()
        return False

    whole = raises(0, n)
    assert whole == (not folded)
    assert raises(0, 0) == whole and raises(n, 0) == whole
    assert eng.has_folded_table() == (not whole)
    # the probe itself: an empty slice with null tensors
    rc = eng.lib.zett_table_rows(eng.handle, None, 0, 0, None, _lib.DTYPE_F32, 0, None, None, None)
    assert rc == (_lib.ZETT_OK if folded else _lib.E_INVALID)
    eng.close()


# ---- A3: a table smaller than the world ---------------------------------------------------------------------------------------------
def test_a_table_smaller_than_the_world():
    from zett_amd.sharding import SharedTable
    cfg, _ = flc.CONFIGS["h512"]
    pad = cfg["pad_token_id"]
    m = np.full((5, 7), pad, dtype=np.int32)
    m[:, 0] = [17, 230, 17, 99, 230]
    m[1, 1] = 99; m[4, 1:3] = [17, 17]
    assert referenced(m, pad).tolist() == [17, 99, 230]
    ids = _cuda(m)
    src = _cuda(synth.make_source_embeddings(cfg, flc.SEED))
    eng = flc._engine(cfg, "f16")
    ref = eng.forward(ids, src, LANG)
    one = SharedTable(eng, ids, src, only_rank=0, world=1)
    assert one.n_ids == 3
    for pieces in (None, 2):
        rows = 8 * (pieces or 1)
        table, stats = eng.table_buffers(rows)
        table.fill_(float("nan")); stats.fill_(float("nan"))
        for r in range(8):
            part = SharedTable(eng, ids, src, only_rank=r, world=8, buffers=(table, stats), pieces=pieces)
            assert part.per * 8 == rows and sum(hi - lo for lo, hi in part.ranges) == (1 if r < 3 else 0)
        assert torch.equal(table[:3].view(torch.int16), one.table[:3].view(torch.int16)) and torch.equal(stats[:3], one.stats[:3])
        assert _eq(part.predict(LANG)(ids), ref)
    eng.close()
    b16 = flc._engine(cfg, "bf16")
    bufs = b16.table_buffers(8)
    for r in range(8):          # every rank refuses — also the five whose slice is empty: none enters an exchange alone
        with pytest.raises(ValueError):
            SharedTable(b16, ids, src, only_rank=r, world=8, buffers=bufs)
    b16.close()


# ---- A4: range flags ------------------------------------------------------------------------------------------------------------------
def _range_inputs(hot_row=5):
    from tests.test_range_guard_gpu import _cfg
    cfg = _cfg()
    w = synth.make_weights(cfg, seed=22)
    src_np = synth.make_source_embeddings(cfg, 22)
    ids_np = synth.make_surface_forms(cfg, 300, seed=22)
    hot = src_np.copy()
    hot[int(ids_np[hot_row, 0]), 3] = 3.0e5            # a referenced row
    unused = sorted(set(range(3, cfg["original_vocab_size"])) - set(ids_np.ravel().tolist()))[0]
    stray = src_np.copy()
    stray[unused] = float("inf")                       # an unreferenced row may hold anything
    return cfg, w, ids_np, src_np, hot, stray


def test_the_range_flags_of_the_table_build_survive_the_forwards():
    from tests.test_range_guard_gpu import _engine
    from zett_amd.sharding import SharedTable
    cfg, w, ids_np, src_np, hot, stray = _range_inputs()
    ids, src, hot, stray = _cuda(ids_np), _cuda(src_np), _cuda(hot), _cuda(stray)
    eng = _engine(cfg, w, "f16")
    _, id_list, n = eng.table_plan(ids)
    table, stats = eng.table_buffers(n)
    eng.table_rows(id_list, 0, n, hot, table, stats)
    assert eng.range_flags() & _lib.RANGE_SOURCE
    shared = SharedTable(eng, ids, hot)
    assert shared.range_flags is not None and shared.range_flags & _lib.RANGE_SOURCE
    assert eng.range_accumulate is False
    shared.predict(1)(ids)
    later = eng.range_flags()          # the word of the forward: whatever it holds, the build's bit is kept by the table
    assert shared.range_flags & _lib.RANGE_SOURCE and (shared.range_flags | later) & _lib.RANGE_SOURCE
    # a clean build behind a dirty one, and an unreferenced infinite row
    assert SharedTable(eng, ids, src).range_flags == 0
    assert SharedTable(eng, ids, stray).range_flags == 0
    # accumulating engine: its word carries the build's bits to the caller's one check; the table does not consume it
    eng.set_option("range_accumulate", 1)
    eng.range_flags()
    acc = SharedTable(eng, ids, hot)
    assert acc.range_flags is None and eng.range_accumulate is True
    acc.predict(1)(ids)
    assert eng.range_flags() & _lib.RANGE_SOURCE
    eng.close()


def _model(cfg, w):
    from zett_amd.config import ZettHypernetConfig
    from zett_amd.hypernet import ZettHypernet
    model = ZettHypernet(ZettHypernetConfig(**cfg))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return model.to("cuda:0").eval()


def _predict_vocabulary(model, ids, src, lang, batch_size):
    from zett_amd.transfer import Args, predict_vocabulary
    with torch.no_grad():
        out = predict_vocabulary(model, ids.long(), src, lang, Args(output="", batch_size=batch_size), rng=np.random.default_rng(7))
    torch.cuda.synchronize()
    return out


def test_a_job_table_keeps_the_range_flags_of_its_build(monkeypatch):
    import zett_amd.sharding as sharding
    from zett_amd.transfer import predict_vocabulary
    # The plain path asks after every batch and keeps what earlier batches predicted in f16; the job asks once and repeats everything.
    # Both are the bf16 prediction of the whole vocabulary when the FIRST batch walked (the seeded permutation's head) trips the guard.
    first_batch = np.random.default_rng(7).permutation(300)[:128]
    cfg, w, ids_np, _, hot, _ = _range_inputs(hot_row=int(first_batch[0]))
    ids, hot = _cuda(ids_np), _cuda(hot)
    built = []

    class Recording(sharding.SharedTable):
        def __init__(self, engine, *args, **kwargs):
            super().__init__(engine, *args, **kwargs)
            built.append((engine.precision, engine.range_accumulate, self.range_flags, predict_vocabulary.last_direct))

    monkeypatch.setattr(sharding, "SharedTable", Recording)
    monkeypatch.delenv("ZETT_JOB_TABLE", raising=False)
    model = _model(cfg, w)
    with pytest.warns(UserWarning, match="left the half range"):
        got = _predict_vocabulary(model, ids, hot, 1, 128)          # 300 rows in 3 batches: the job table is taken
    assert built == [("f16", True, None, True)], built               # once, on the first (f16) attempt, on the accumulating word
    assert predict_vocabulary.last_job_table is False and model.precision == "bf16"          # (the repeat in bf16 has no folded table)
    monkeypatch.setenv("ZETT_JOB_TABLE", "0")
    plain = _model(cfg, w)
    with pytest.warns(UserWarning, match="left the half range"):
        want = _predict_vocabulary(plain, ids, hot, 1, 128)
    assert len(built) == 1 and plain.precision == "bf16"
    assert _eq(got, want)


# ---- A5: the capability decision of predict_vocabulary ------------------------------------------------------------------------------
def test_predict_vocabulary_decides_table_or_no_table_from_the_engine(monkeypatch):
    import zett_amd.sharding as sharding
    from zett_amd.transfer import predict_vocabulary
    monkeypatch.delenv("ZETT_JOB_TABLE", raising=False)
    cfg, _ = flc.CONFIGS["tiny"]
    w = synth.make_weights(cfg, flc.SEED)
    ids = _cuda(synth.make_surface_forms(cfg, 300, seed=flc.SEED, n_special=2))
    src = _cuda(synth.make_source_embeddings(cfg, flc.SEED))
    predict_vocabulary.last_job_table = None
    got = _predict_vocabulary(_model(cfg, w), ids, src, LANG, 128)
    assert predict_vocabulary.last_job_table is False          # H = 128: no folded table, decided without an exception
    monkeypatch.setenv("ZETT_JOB_TABLE", "0")
    want = _predict_vocabulary(_model(cfg, w), ids, src, LANG, 128)
    assert _eq(got, want)
    monkeypatch.delenv("ZETT_JOB_TABLE")

    # where the table exists, an error of its build is the caller's to see
    class Boom:
        def __init__(self, *args, **kwargs):
            raise ValueError("boom")

    monkeypatch.setattr(sharding, "SharedTable", Boom)
    cfg5, _ = flc.CONFIGS["h512"]
    with pytest.raises(ValueError, match="boom"):
        _predict_vocabulary(_model(cfg5, synth.make_weights(cfg5, flc.SEED)), ids, _cuda(synth.make_source_embeddings(cfg5, flc.SEED)), LANG, 128)


# ---- A6: the arguments of forward_table[_into] --------------------------------------------------------------------------------------
def test_forward_table_refuses_bad_table_arguments(arm):
    a = arm
    table, stats, id_slot = a.table, a.stats, a.id_slot
    rows, H = table.shape
    wide = torch.zeros((rows, 2 * H), dtype=torch.float16, device="cuda")
    bad = {
        "the other 16-bit type": (table.to(torch.bfloat16), stats, id_slot),
        "a float32 table": (table.float(), stats, id_slot),
        "a non-contiguous table": (wide[:, :H], stats, id_slot),
        "a table on the CPU": (table.cpu(), stats, id_slot),
        "stats on the CPU": (table, stats.cpu(), id_slot),
        "float64 stats": (table, stats.double(), id_slot),
        "stats [rows, 3]": (table, torch.zeros((rows, 3), device="cuda"), id_slot),
        "stats [rows]": (table, torch.zeros((rows,), device="cuda"), id_slot),
        "non-contiguous stats": (table, torch.zeros((rows, 4), device="cuda")[:, :2], id_slot),
        "fewer stats rows than table rows": (table, stats[:-1], id_slot),
        "fewer table rows than stats rows": (table[:-1], stats, id_slot),
        "a table of another width": (wide, stats, id_slot),
        "int64 id_slot": (table, stats, id_slot.long()),
        "id_slot [V]": (table, stats, id_slot[:-1].contiguous()),
        "id_slot [V + 2]": (table, stats, torch.cat([id_slot, id_slot[-1:]])),
        "id_slot on the CPU": (table, stats, id_slot.cpu()),
    }
    (out_in, out_out, out_bias), _ = a.destinations(N_ROWS)[0]
    before = [None if t is None else t.clone() for t in (out_in, out_out, out_bias)]
    for what, (t, s, slot) in bad.items():
        with pytest.raises(ValueError):
            a.eng.forward_table(a.ids, t, s, slot, a.lang)
            pytest.fail(f"forward_table accepted {what}")
        with pytest.raises(ValueError):
            a.eng.forward_table_into(a.ids, t, s, slot, a.lang, out_in, out_out, out_bias)
            pytest.fail(f"forward_table_into accepted {what}")
    torch.cuda.synchronize()
    assert _eq((out_in, out_out, out_bias), before)
    assert _eq(a.forward_table(a.ids), a.ref)
