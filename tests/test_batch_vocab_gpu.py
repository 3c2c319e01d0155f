"""zett_amd.training.subsample_batch_vocabulary on the GPU (csrc/train_batch.hip): every member equal (torch.equal) to the numpy
restatement of tests/batch_vocab_ref.py — which tests/test_batch_vocab_host.py holds to the reference's own outputs —, the status word,
and the call in front of a training step of the tiny hypernetwork."""
import numpy as np
import pytest
import torch

from tests.batch_vocab_ref import FIXTURES, batch_vocab_ref, blank_labels, load_fixture, recipe
from zett_amd import synth
from zett_amd.training import (BATCH_BAD_ID, BATCH_BAD_ORDER, BATCH_OVERFLOW, BATCH_REPEAT, lm_head_loss, splice_special_rows, subsample_batch_vocabulary,
                               token_embeddings)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INTS = (torch.int32, torch.int64)
MODES = ("random", "positives_only")


def _case(v, t, l, special, seed=0):
    ids, labels, sf, priors, order = recipe(v, t, l, tuple(special), seed)
    return {"input_ids": ids, "labels": labels, "special_ids": list(special), "surface_forms": sf, "priors": priors, "negative_order": order}


def _ref(a, n, mode):
    return batch_vocab_ref(a["input_ids"], a["labels"], a["special_ids"], n, a["surface_forms"], a["priors"], mode, a["negative_order"])


def _call(a, n, mode, ids_dtype=torch.int64, sf_dtype=torch.int64, pad=0, labels_dtype=None, order_dtype=torch.int64, **kw):
    """The device call on the arrays of a case: surface forms as a view with row stride L + pad."""
    sf = torch.from_numpy(np.array(a["surface_forms"])).to(sf_dtype)
    wide = torch.full((sf.shape[0], sf.shape[1] + pad), -7, dtype=sf_dtype, device=DEV)
    wide[:, :sf.shape[1]] = sf.to(DEV)
    order = torch.from_numpy(np.array(a["negative_order"])).to(order_dtype).to(DEV) if mode == "random" else None
    return subsample_batch_vocabulary(torch.from_numpy(np.array(a["input_ids"])).to(ids_dtype).to(DEV),
                                      torch.from_numpy(np.array(a["labels"])).to(labels_dtype or ids_dtype).to(DEV), a["special_ids"], n,
                                      wide[:, :sf.shape[1]], torch.from_numpy(np.array(a["priors"])).to(DEV), mode=mode, negative_order=order, **kw)


def _same(bv, want, ids_dtype=torch.int64, sf_dtype=torch.int64, labels_dtype=None, what=None):
    """torch.equal on every member (dtypes included)"""
    pairs = (("input_ids", ids_dtype), ("labels", labels_dtype or ids_dtype), ("ids_to_embed", ids_dtype), ("target_surface_forms", sf_dtype),
             ("target_priors", torch.float32), ("mask", torch.bool))
    for key, dtype in pairs:
        got, exp = getattr(bv, key).cpu(), torch.from_numpy(np.array(want[key])).to(dtype)
        assert got.dtype == dtype and torch.equal(got, exp), (what, key, int((got != exp).sum()) if got.shape == exp.shape else (got.shape, exp.shape))
    assert bv.target_surface_forms.is_contiguous()
    assert isinstance(bv.special_indices, list) and bv.special_indices == [int(x) for x in want["special_indices"]], what
    assert bv.n_positive.dtype == torch.int32 and bv.n_positive.dim() == 0 and int(bv.n_positive) == want["n_positive"], what
    assert bv.status.dtype == torch.int32 and int(bv.status) == 0, what


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("ids_dtype", INTS, ids=("i32", "i64"))
def test_fixtures_of_the_reference(name, ids_dtype):
    """The reference's own outputs, with every combination of int32 / int64 surface forms and row stride L / L + 3; then the same batch with
    most labels -100, which changes the labels alone."""
    inputs, expected = load_fixture(name)
    n, mode = inputs["n"], inputs["mode"]
    want = dict(expected, n_positive=len(np.union1d(np.union1d(inputs["input_ids"], inputs["labels"]), inputs["special_ids"])))
    for sf_dtype in INTS:
        for pad in (0, 3):
            _same(_call(inputs, n, mode, ids_dtype, sf_dtype, pad), want, ids_dtype, sf_dtype, what=(name, sf_dtype, pad))
    flat = dict(inputs, input_ids=inputs["input_ids"].reshape(-1), labels=inputs["labels"].reshape(-1))          # [T] instead of [B, S]
    _same(_call(flat, n, mode, ids_dtype), dict(want, input_ids=want["input_ids"].reshape(-1), labels=want["labels"].reshape(-1)), ids_dtype, what=(name, "flat"))
    blank = blank_labels(inputs)
    _same(_call(dict(inputs, labels=blank), n, mode, ids_dtype, labels_dtype=torch.int64), dict(want, labels=np.where(blank == -100, -100, want["labels"])), ids_dtype,
          labels_dtype=torch.int64, what=(name, "blank"))


@pytest.mark.parametrize("mode", MODES)
def test_the_smallest_case(mode):
    a = _case(5, 1, 1, [0])
    _same(_call(a, 4, mode), _ref(a, 4, mode), what=mode)


@pytest.mark.parametrize("mode", MODES)
def test_several_scan_segments_a_ragged_tail_and_a_special_beyond_n(mode):
    """V = 70 001 is 68 full segments of 1024 ids and one of 369; special id 70 000 goes to the last row; id 0 is special, in the batch, and in
    positives_only the repeated negative, so the LAST row of id 0 is what input_ids are remapped to."""
    v, t, n, l = 70001, 3000, 4096, 7
    a = _case(v, t, l, [0, 1, 2, 70000])
    want = _ref(a, n, mode)
    assert want["special_indices"] == [0, 1, 2, n - 1] and want["n_positive"] < n and (a["input_ids"] == 0).any()
    bv = _call(a, n, mode, torch.int32, torch.int32, order_dtype=torch.int32)
    _same(bv, want, torch.int32, torch.int32, what=mode)
    if mode == "positives_only":
        last = int(np.flatnonzero(want["ids_to_embed"] == 0).max())
        assert last == n - 2 and (want["input_ids"][a["input_ids"] == 0] == last).all()
    again = _call(a, n, mode, torch.int32, torch.int32, order_dtype=torch.int32)          # a second run: the same bits
    for x, y in zip(bv, again):
        assert torch.equal(x, y) if isinstance(x, torch.Tensor) else x == y


@pytest.mark.parametrize("v", (1023, 1024, 1025))
@pytest.mark.parametrize("mode", MODES)
def test_the_edges_of_one_scan_segment(mode, v):
    """V one short of a segment of 1024 ids (a ragged tail alone), exactly one segment, and one id into a second segment; the last id is
    special."""
    a = _case(v, 200, 2, [0, v - 1])
    _same(_call(a, 256, mode), _ref(a, 256, mode), what=(mode, v))


@pytest.mark.parametrize("mode", MODES)
def test_more_than_1024_scan_segments(mode):
    """V = 2^20 + 1325 is 1026 segments: the workgroup that scans the segment counts takes a second round of two segments, whose offsets are
    the first round's total (the carry) and what follows.  Positives in both of those segments — 2^20 + 7 put there by hand, V - 2 and V - 3
    the recipe's label-only ids — and the special id V - 1 land in the right rows only if the carry is right."""
    v, t, n = (1 << 20) + 1025 + 300, 3000, 4096
    a = _case(v, t, 1, [0, 1, v - 1])
    ids = a["input_ids"].copy()
    ids[5] = (1 << 20) + 7
    a = dict(a, input_ids=ids)
    want = _ref(a, n, mode)
    beyond = want["ids_to_embed"][:want["n_positive"]]
    assert ((beyond >= 1 << 20) & (beyond < (1 << 20) + 1024)).any() and ((beyond >= (1 << 20) + 1024) & (beyond < v - 1)).any()
    _same(_call(a, n, mode, torch.int32, torch.int32, order_dtype=torch.int32), want, torch.int32, torch.int32, what=mode)


def test_no_negative_at_all():
    """N = n_positive exactly: K = 0."""
    a = _case(5000, 700, 4, [3, 0])
    n = _ref(a, 5000, "random")["n_positive"]
    for mode in MODES:
        want = _ref(a, n, mode)
        assert want["n_positive"] == n and sorted(want["ids_to_embed"].tolist()) == sorted(set(a["input_ids"].tolist()) | set(a["labels"].tolist()) - {-100} | {0, 3})
        _same(_call(a, n, mode), want, what=mode)


def test_every_id_is_taken():
    """N = V: every absent id is a negative and ids_to_embed is a permutation."""
    v = 3000
    a = _case(v, 500, 3, [2, 1, v - 1])
    want = _ref(a, v, "random")
    assert np.array_equal(np.sort(want["ids_to_embed"]), np.arange(v))
    _same(_call(a, v, "random", torch.int64, torch.int32), want, torch.int64, torch.int32)


def test_positives_only_remaps_id_0_to_its_last_row():
    a = _case(50, 40, 2, [0, 3])
    ids = a["input_ids"].copy()
    ids[:4] = 0
    a = dict(a, input_ids=ids)
    want = _ref(a, 32, "positives_only")
    assert want["ids_to_embed"][0] == 0 and want["ids_to_embed"][-1] == 0 and (want["input_ids"][:4] == 31).all()
    _same(_call(a, 32, "positives_only"), want)


@pytest.mark.parametrize("l", (1, 8, 15))
def test_surface_form_widths(l):
    """L = 8: rows of 32 / 64 bytes, copied 16 bytes per lane where the stride allows it; L = 1 and 15 and the stride L + 3: by element."""
    a = _case(900, 300, l, [1, 0])
    for mode in MODES:
        want = _ref(a, 400, mode)
        for sf_dtype in INTS:
            for pad in (0, 3, 4):
                _same(_call(a, 400, mode, torch.int64, sf_dtype, pad), want, torch.int64, sf_dtype, what=(l, mode, sf_dtype, pad))


def _status_case():
    return _case(400, 64, 3, [1, 0]), 128


@pytest.mark.parametrize("bad", (-1, 400, 2 ** 31 + 5))
@pytest.mark.parametrize("where", ("input_ids", "labels"))
def test_an_id_outside_the_vocabulary(bad, where):
    """IndexError with check=True; with check=False the call returns, bit 1 is set and nothing faults: the id is never an address."""
    a, n = _status_case()
    x = a[where].copy()
    x[5] = bad
    a = dict(a, **{where: x})
    for mode in MODES:
        with pytest.raises(IndexError, match="outside"):
            _call(a, n, mode)
        bv = _call(a, n, mode, check=False)
        assert int(bv.status) & BATCH_BAD_ID and not int(bv.status) & (BATCH_OVERFLOW | BATCH_BAD_ORDER)
        assert bv.ids_to_embed.shape == (n,) and bool(((bv.ids_to_embed >= 0) & (bv.ids_to_embed < 400)).all())
        assert bool(((bv.input_ids >= 0) & (bv.input_ids < n)).all())
    torch.cuda.synchronize()


def test_one_id_too_many():
    a, _ = _status_case()
    n = _ref(a, 400, "random")["n_positive"] - 1
    for mode in MODES:
        with pytest.raises(ValueError, match="more than n_token_subsample"):
            _call(a, n, mode)
        bv = _call(a, n, mode, check=False)
        assert int(bv.status) & BATCH_OVERFLOW and int(bv.n_positive) == n + 1
        assert bool(((bv.ids_to_embed >= 0) & (bv.ids_to_embed < 400)).all()) and bool(((bv.input_ids >= 0) & (bv.input_ids < n)).all())
    torch.cuda.synchronize()


def test_a_negative_order_that_is_no_permutation():
    a, n = _status_case()
    want = _ref(a, n, "random")
    batch = np.concatenate([a["input_ids"], a["labels"], a["special_ids"]])
    taken = want["ids_to_embed"][~np.isin(want["ids_to_embed"], batch)]          # the negatives, in negative_order's order
    order = a["negative_order"].copy()
    first, second = (int(np.flatnonzero(order == x)[0]) for x in taken[-2:])
    order[second] = order[first]          # a repeated entry among those taken
    with pytest.raises(ValueError, match="twice"):
        _call(dict(a, negative_order=order), n, "random")
    bv = _call(dict(a, negative_order=order), n, "random", check=False)
    assert int(bv.status) == BATCH_REPEAT
    order = a["negative_order"].copy()
    order[:] = a["input_ids"][0]          # every entry an id of the batch: nothing to take
    assert int(_call(dict(a, negative_order=order), n, "random", check=False).status) == BATCH_REPEAT
    order = a["negative_order"].copy()
    order[3] = 400
    with pytest.raises(IndexError, match="negative_order"):
        _call(dict(a, negative_order=order), n, "random")
    order[7] = -(2 ** 40)
    bv = _call(dict(a, negative_order=order), n, "random", check=False)
    assert int(bv.status) & BATCH_BAD_ORDER and bool(((bv.ids_to_embed >= 0) & (bv.ids_to_embed < 400)).all())
    _same(_call(dict(a, negative_order=order), n, "positives_only"), _ref(a, n, "positives_only"))          # negative_order is not read there
    torch.cuda.synchronize()


def test_in_front_of_a_training_step_of_the_tiny_hypernet():
    """subsample_batch_vocabulary -> hypernet -> splice -> lookup -> a toy causal backbone -> lm_head_loss, against the same chain fed from the
    restatement's arrays: the loss and the gradients arriving at the hypernetwork's outputs are the same bits."""
    from zett_amd.config import ZettHypernetConfig
    from zett_amd.hypernet import ZettHypernet
    cfg, *_ = synth.workload("tiny")
    v, n, batch, seq, e = 200, 96, 4, 24, cfg["n_embd"]
    model = ZettHypernet(ZettHypernetConfig(**cfg))
    model.load_state_dict({k: torch.from_numpy(x) for k, x in synth.make_weights(cfg, seed=83).items()})
    model = model.to(DEV).requires_grad_(True).train()
    src = torch.from_numpy(synth.make_source_embeddings(cfg, 83)).to(DEV)
    sf = synth.make_surface_forms(cfg, v, seed=83, n_special=1)
    rng = np.random.default_rng(9)
    ids = np.minimum(np.floor(v * rng.random((batch, seq)) ** 2).astype(np.int64), v - 1)
    ids[1, 15:] = 3
    labels = np.where(rng.random((batch, seq)) < 0.2, -100, np.roll(ids, -1, 1))
    labels[0, 0] = np.setdiff1d(np.arange(4, v - 1), ids)[-1]          # an id of the labels alone
    special, in_reference = [3, 0, v - 1], [1, 7, 4]
    a = {"input_ids": ids, "labels": labels, "special_ids": special, "surface_forms": sf, "priors": rng.standard_normal(v).astype(np.float32),
         "negative_order": rng.permutation(v)}
    want = _ref(a, n, "random")
    mix = (torch.randn(e, e, generator=torch.Generator().manual_seed(1)) / e ** 0.5).to(DEV)
    steps = torch.arange(1, seq + 1, device=DEV, dtype=torch.float32)[:, None]

    def chain(input_ids, lab, surface_forms, priors, mask, special_indices):
        tap = {}
        pred_in, pred_out, _bias = model(surface_forms, source_embeddings=src, lang_index=torch.tensor(2))
        pred_in.register_hook(lambda g: tap.__setitem__("d pred_in", g.clone()))
        pred_out.register_hook(lambda g: tap.__setitem__("d pred_out", g.clone()))
        pred_in, pred_out = splice_special_rows(pred_in, pred_out, src, special_indices, in_reference, inplace=True)
        x = token_embeddings(pred_in, input_ids)
        hidden = x + torch.tanh(torch.cumsum(x, 1) / steps @ mix)
        loss = lm_head_loss(hidden, pred_out, lab, mode="mlm", priors=priors, vocab_mask=mask, precision="f32")[0]
        loss.backward()
        model.zero_grad(set_to_none=True)
        return loss.detach(), tap

    bv = _call(a, n, "random", torch.int64, torch.int32)
    _same(bv, want, torch.int64, torch.int32)
    ours = chain(bv.input_ids, bv.labels, bv.target_surface_forms, bv.target_priors, bv.mask, bv.special_indices)
    up = lambda key, dtype=None: torch.from_numpy(np.array(want[key])).to(DEV) if dtype is None else torch.from_numpy(np.array(want[key])).to(dtype).to(DEV)          # noqa: E731
    theirs = chain(up("input_ids"), up("labels"), up("target_surface_forms", torch.int32), up("target_priors"), up("mask"), want["special_indices"])
    assert torch.equal(ours[0].view(torch.int32), theirs[0].view(torch.int32)) and bool(torch.isfinite(ours[0]))
    assert set(ours[1]) == {"d pred_in", "d pred_out"}
    for key in ours[1]:
        assert torch.equal(ours[1][key].view(torch.int32), theirs[1][key].view(torch.int32)) and bool(ours[1][key].any()), key
