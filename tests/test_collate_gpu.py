"""zett_amd.collate on the GPU (csrc/train_batch.hip: zett_op_label_batch, zett_op_pad_vocabulary; DeviceCollator): every output equal
(torch.equal, dtypes included) to the numpy restatement of tests/collate_ref.py, which tests/test_collate_host.py holds to the installed
library and to the reference's own dicts."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import collate_ref as cr
from zett_amd import _lib
from zett_amd.collate import LABEL_BAD_ID, DeviceCollator, derived_seed, label_batch, mlm_thresholds, pad_vocabulary, padded_rows
from zett_amd.training import BATCH_OVERFLOW, subsample_batch_vocabulary

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INTS = (torch.int32, torch.int64)
SHAPES = ((1, 1), (1, 63), (3, 64), (5, 65), (2, 257), (7, 300), (33, 128))
SPECIALS = {0: [], 1: [2], 5: [3, 0, 49, 7, 21], 256: list(range(40, 296))}
TWO53 = 1 << 53


def _ids(shape, v, special, seed=0):
    rng = np.random.default_rng(seed + shape[1])
    ids = np.minimum(np.floor(v * rng.random(shape) ** 2).astype(np.int64), v - 1)
    if special:
        ids.reshape(-1)[::7] = special[0]
    return ids


def _table(v, seed=0):
    return np.random.default_rng(seed).integers(1, 17, v).astype(np.int64)


def _same(got, want, dtype, what=None):
    for key, dt in (("input_ids", dtype), ("labels", dtype), ("byte_lengths", torch.int64), ("record", torch.int64)):
        g, w = getattr(got, key).cpu(), torch.from_numpy(np.array(want[key])).to(dt)
        assert g.dtype == dt and g.shape == w.shape and torch.equal(g, w), (what, key, (g != w).nonzero()[:4].tolist() if g.shape == w.shape else (g.shape, w.shape))
    g = got.metrics.cpu()
    assert g.dtype == torch.float64 and g.shape == (2,)
    for i in range(2):          # float64 bits; NaN (no non-special position) as NaN
        assert (np.isnan(want["metrics"][i]) and bool(torch.isnan(g[i]))) or g[i].numpy().tobytes() == np.float64(want["metrics"][i]).tobytes(), (what, i, g, want["metrics"])


def _call(ids, special, table, dtype=torch.int64, table_dtype=torch.int64, pad=0, inplace=False, **kw):
    """The device call: the ids as a view with row stride S + pad."""
    b, s = ids.shape
    wide = torch.full((b, s + pad), -7, dtype=dtype, device=DEV)
    wide[:, :s] = torch.from_numpy(ids).to(dtype).to(DEV)
    view = wide[:, :s]
    got = label_batch(view, special, torch.from_numpy(table).to(table_dtype).to(DEV), inplace=inplace, **kw)
    if inplace:
        assert got.input_ids.data_ptr() == wide.data_ptr()
    else:
        assert torch.equal(view.cpu(), torch.from_numpy(ids).to(dtype)) and got.input_ids.is_contiguous()
    assert bool((wide[:, s:] == -7).all())
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dtype", INTS, ids=("i32", "i64"))
def test_label_batch_shapes(shape, dtype):
    """One position, the edges of a wave and of a workgroup, rows that straddle workgroups; contiguous and with row stride S + 3, in place
    and out of place; both losses."""
    v, special = 300, SPECIALS[5]
    ids, table = _ids(shape, v, special), _table(v)
    kw = dict(vocab_len=v, mask_token_id=3, unk_token_id=1, seed=11)
    for loss in ("mlm", "clm"):
        want = cr.label_batch(ids, special, table, loss=loss, **kw)
        for pad in (0, 3):
            for inplace in (False, True):
                _same(_call(ids, special, table, dtype, pad=pad, inplace=inplace, loss=loss, **kw), want, dtype, (loss, pad, inplace))
    if shape == (33, 128):
        r = cr.label_batch(ids, special, table, loss="mlm", **kw)["record"]
        assert r[4] > 0 and r[5] > 0 and r[6] > 0 and r[3] > 0          # the case exercises every branch


@pytest.mark.parametrize("n_special", sorted(SPECIALS))
@pytest.mark.parametrize("table_dtype", INTS, ids=("t32", "t64"))
def test_label_batch_special_lists_and_table_widths(n_special, table_dtype):
    v, special = 300, SPECIALS[n_special]
    ids, table = _ids((5, 65), v, special, seed=n_special), _table(v, 1)
    kw = dict(vocab_len=v, loss="mlm", mask_token_id=special[0] if special else 4, unk_token_id=1, seed=3, thresholds_=cr.thresholds(0.5, 0.5, 0.25))
    want = cr.label_batch(ids, special, table, **kw)
    kw["thresholds"] = kw.pop("thresholds_")
    assert kw["thresholds"] == mlm_thresholds(0.5, 0.5, 0.25)
    _same(_call(ids, special, table, table_dtype=table_dtype, **kw), want, torch.int64, n_special)


@pytest.mark.parametrize("vocab_len", (1, 50, 70000))
def test_label_batch_vocab_len(vocab_len):
    """every masked position gets a random id below vocab_len: (1, 0, 1)"""
    v = 70001
    ids, table = _ids((7, 300), v, []), _table(v, 2)
    t = cr.thresholds(1.0, 0.0, 1.0)
    want = cr.label_batch(ids, [], table, vocab_len=vocab_len, loss="mlm", mask_token_id=0, seed=5, thresholds_=t)
    assert want["record"][6] == ids.size and want["input_ids"].max() < vocab_len and (vocab_len < 70000 or want["input_ids"].max() > 65536)
    _same(_call(ids, [], table, torch.int32, vocab_len=vocab_len, loss="mlm", mask_token_id=0, seed=5, thresholds=t), want, torch.int32, vocab_len)


def test_label_batch_no_unk_all_special_and_the_threshold_edges():
    v, special = 300, SPECIALS[5]
    ids, table = _ids((5, 65), v, special), _table(v)
    kw = dict(vocab_len=v, loss="mlm", mask_token_id=3, seed=1)
    _same(_call(ids, special, table, unk_token_id=None, **kw), cr.label_batch(ids, special, table, unk_token_id=None, **kw), torch.int64, "no unk")
    every = np.array(special, dtype=np.int64)[np.arange(5 * 65) % 5].reshape(5, 65)          # all positions special: nothing masked, 0 / 0
    want = cr.label_batch(every, special, table, unk_token_id=0, **kw)
    assert np.isnan(want["metrics"][0]) and want["record"][1] == 0 and want["record"][4] == 0 and (want["labels"] == -100).all()
    _same(_call(every, special, table, unk_token_id=0, **kw), want, torch.int64, "all special")
    for t, n_masked in (((0, TWO53, TWO53), 0), ((TWO53, TWO53, 0), int((~np.isin(ids, special)).sum()))):
        want = cr.label_batch(ids, special, table, unk_token_id=1, thresholds_=t, **kw)
        assert want["record"][4] == n_masked == want["record"][5]
        _same(_call(ids, special, table, unk_token_id=1, thresholds=t, **kw), want, torch.int64, t)
    with pytest.raises(ValueError, match="mask token"):
        _call(ids, special, table, vocab_len=v, loss="mlm")


def test_label_batch_same_bits_twice_and_another_mask_for_another_seed():
    v, special = 300, SPECIALS[1]
    ids, table = _ids((33, 128), v, special), _table(v)
    kw = dict(vocab_len=v, loss="mlm", mask_token_id=2, unk_token_id=1)
    a, b, c = (_call(ids, special, table, seed=s, **kw) for s in (7, 7, 8))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a.labels, c.labels)
    _same(c, cr.label_batch(ids, special, table, seed=8, **kw), torch.int64)


def _guarded(n_bytes, guard=64):
    buf = torch.full((n_bytes + 2 * guard,), 0xAB, dtype=torch.uint8, device=DEV)
    return buf, buf[guard:guard + n_bytes]


def _guards_intact(buf, n_bytes, guard=64):
    return bool((buf[:guard] == 0xAB).all()) and bool((buf[guard + n_bytes:] == 0xAB).all())


@pytest.mark.parametrize("dtype", INTS, ids=("i32", "i64"))
def test_label_batch_ids_outside_the_table(dtype):
    """-1 and V: the status bit, IndexError with check=True, the restatement's values (never masked, byte length 0), and through the C
    interface 0xAB guard bytes around every output stay as they were."""
    v, special = 300, SPECIALS[5]
    ids, table = _ids((5, 65), v, special), _table(v)
    ids[1, 2], ids[4, 64] = -1, v
    kw = dict(vocab_len=v, loss="mlm", mask_token_id=3, unk_token_id=1, seed=2, thresholds_=cr.thresholds(1.0, 0.8, 0.1))
    want = cr.label_batch(ids, special, table, **kw)
    assert want["record"][7] == LABEL_BAD_ID and want["labels"][1, 2] == -100 and want["byte_lengths"][4, 64] == 0 and want["input_ids"][4, 64] == v
    kw["thresholds"] = kw.pop("thresholds_")
    with pytest.raises(IndexError, match="outside"):
        _call(ids, special, table, dtype, **kw)
    _same(_call(ids, special, table, dtype, check=False, **kw), want, dtype)
    b, s = ids.shape
    w = 4 if dtype == torch.int32 else 8
    sizes = {"out": b * s * w, "labels": b * s * w, "lengths": b * s * 8, "record": 64, "metrics": 16}
    bufs = {k: _guarded(n) for k, n in sizes.items()}
    d_ids, d_table = torch.from_numpy(ids).to(dtype).to(DEV), torch.from_numpy(table).to(DEV)
    work = torch.empty(_lib.LABEL_WORKSPACE_BYTES, dtype=torch.uint8, device=DEV)
    P = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    rc = _lib.load().zett_op_label_batch(P(d_ids), w, s, b, s, (C.c_int32 * 5)(*special), 5, P(d_table), 8, v, v, 3, 1, _lib.LABEL_MLM, *kw["thresholds"], 2,
                                         P(bufs["out"][1]), s, P(bufs["labels"][1]), P(bufs["lengths"][1]), P(bufs["record"][1]), P(bufs["metrics"][1]), P(work),
                                         work.numel(), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert _guards_intact(bufs[k][0], n), k
    assert torch.equal(bufs["out"][1].view(dtype).cpu().reshape(b, s), torch.from_numpy(want["input_ids"]).to(dtype))
    assert torch.equal(bufs["record"][1].view(torch.int64).cpu(), torch.from_numpy(want["record"]))


@pytest.mark.parametrize("v,r,l", ((1, 8, 1), (8, 8, 7), (392, 520, 7), (300, 304, 3)))
def test_pad_vocabulary(v, r, l):
    rng = np.random.default_rng(v)
    sf, priors = rng.integers(0, 1000, (v, l)), rng.standard_normal(v) * 3
    for sf_dtype in INTS:
        for p_dtype in (torch.float32, torch.float64):
            for pad in (0, 3):
                wide = torch.full((v, l + pad), -7, dtype=sf_dtype, device=DEV)
                wide[:, :l] = torch.from_numpy(sf).to(sf_dtype).to(DEV)
                d_priors = torch.from_numpy(priors).to(p_dtype).to(DEV)
                got = pad_vocabulary(wide[:, :l], d_priors, r)
                want = cr.pad_vocabulary(sf, d_priors.cpu().numpy(), r)
                for key, dt in (("target_surface_forms", sf_dtype), ("target_priors", torch.float32), ("mask", torch.bool), ("ids_to_embed", torch.int64)):
                    g, w = getattr(got, key).cpu(), torch.from_numpy(want[key]).to(dt)
                    assert g.dtype == dt and g.shape == w.shape and torch.equal(g, w), (key, sf_dtype, p_dtype, pad)
                assert got.target_surface_forms.is_contiguous()
    with pytest.raises(ValueError, match="less than"):
        pad_vocabulary(wide[:, :l], d_priors, v - 1)


def test_pad_vocabulary_guards():
    v, r, l = 300, 304, 3
    rng = np.random.default_rng(1)
    sf, priors = torch.from_numpy(rng.integers(0, 1000, (v, l)).astype(np.int32)).to(DEV), torch.from_numpy(rng.standard_normal(v)).to(DEV)
    sizes = {"sf": r * l * 4, "priors": r * 4, "mask": r, "ids": r * 8}
    bufs = {k: _guarded(n) for k, n in sizes.items()}
    P = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    rc = _lib.load().zett_op_pad_vocabulary(P(sf), 4, l, l, v, r, P(priors), 8, P(bufs["sf"][1]), P(bufs["priors"][1]), P(bufs["mask"][1]), P(bufs["ids"][1]),
                                            C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    for k, n in sizes.items():
        assert _guards_intact(bufs[k][0], n), k
    want = cr.pad_vocabulary(sf.cpu().numpy(), priors.cpu().numpy(), r)
    assert torch.equal(bufs["sf"][1].view(torch.int32).cpu().reshape(r, l), torch.from_numpy(want["target_surface_forms"]))
    assert torch.equal(bufs["priors"][1].view(torch.float32).cpu(), torch.from_numpy(want["target_priors"]))
    assert torch.equal(bufs["mask"][1].cpu(), torch.from_numpy(want["mask"]).to(torch.uint8))
    assert torch.equal(bufs["ids"][1].view(torch.int64).cpu(), torch.from_numpy(want["ids_to_embed"]))


# ---- the reference's dicts through the device pieces -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cr.FIXTURES)
def test_fixtures_of_the_reference_through_the_pieces(name):
    """The fixtures hold prepared input_ids (the reference's tokenizer call was stood in for), so they enter behind the encoder:
    label_batch, then subsample_batch_vocabulary or pad_vocabulary, against the restatement that tests/test_collate_host.py holds to the
    reference's dict — and, where the reference does not list -100 as an id, against that dict itself."""
    inputs, ref = cr.load_fixture(name)
    want = cr.encode_fixture(inputs)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)          # noqa: E731
    v = len(inputs["priors"])
    lb = label_batch(up(inputs["input_ids"]), inputs["special_ids"], up(inputs["byte_lengths"]), vocab_len=v, loss=inputs["loss"], mask_token_id=inputs["mask_token_id"],
                     unk_token_id=inputs["unk_token_id"], seed=inputs["seed"], thresholds=mlm_thresholds(*inputs["probabilities"]))
    assert lb.metrics.cpu().numpy().tobytes() == ref["metrics"].tobytes() and torch.equal(lb.byte_lengths.cpu(), torch.from_numpy(ref["byte_lengths"]))
    if inputs["n_token_subsample"] is not None:
        order = up(inputs["negative_order"]) if inputs["subsample_mode"] == "random" else None
        got = subsample_batch_vocabulary(lb.input_ids, lb.labels, inputs["special_ids"], inputs["n_token_subsample"], up(inputs["surface_forms"]),
                                         up(inputs["priors"]).float(), mode=inputs["subsample_mode"], negative_order=order)
        input_ids, labels = got.input_ids, got.labels
        assert got.special_indices == want["special_indices"] == ref["special_indices"].tolist()
    else:
        got = pad_vocabulary(up(inputs["surface_forms"]), up(inputs["priors"]), padded_rows(v, inputs["pad_to_multiple_of"], inputs["tokenizer_sample_max"]))
        input_ids, labels = lb.input_ids, lb.labels
    exact = not (ref["ids_to_embed"] == -100).any()
    for key, tensor in (("input_ids", input_ids), ("labels", labels), ("ids_to_embed", got.ids_to_embed), ("target_surface_forms", got.target_surface_forms),
                        ("target_priors", got.target_priors), ("mask", got.mask)):
        assert torch.equal(tensor.cpu(), torch.from_numpy(np.asarray(want[key])).to(tensor.dtype)), (name, key)
        if exact:
            assert np.array_equal(tensor.cpu().numpy(), ref[key].astype(np.float32) if key == "target_priors" else ref[key]), (name, key, "reference")


# ---- DeviceCollator ----------------------------------------------------------------------------------------------------------------------------
BLOCK, MAXLEN = 24, 7


_bpe = cr.bpe_tokenizer


def _args(**kw):
    base = dict(do_tokenizer_sampling=False, n_token_subsample=None, pad_to_multiple_of=8, subsample_mode="random", block_size=BLOCK, use_passthrough_hypernet=False,
                add_prefix_space=False, hn_surface_maxlen=MAXLEN, sample_text_span=True, langs=["de", "en", "fr"], tokenizer_sample_max=1536, tokenizer_sample_min=1100,
                tokenizer_sample_mean=1200, tokenizer_sample_std=30, tokenizer_noise_mean=0.0, tokenizer_noise_std=0.0)
    return types.SimpleNamespace(**dict(base, **kw))


def _texts():
    rng = np.random.default_rng(3)
    words = "the quick brown fox jumps over the lazy dog , it's 12 345 times . we'll see".split(" ")
    texts = [" ".join(words[i] for i in rng.integers(0, len(words), size=20)) for _ in range(7)]
    return texts + [" ".join(words[i] for i in rng.integers(0, len(words), size=120))]          # one text longer than 16 * block_size characters: its span is drawn


@pytest.fixture(scope="module")
def fixed():
    """fixed(loss, **data_args) -> a DeviceCollator on the test tokenizer, built once per configuration for this module's tests"""
    built = {}

    def make(loss, hn=True, **kw):
        key = (loss, hn, tuple(sorted(kw.items())))
        if key not in built:
            built[key] = DeviceCollator(_bpe(), _bpe(False) if hn else None, _args(**kw), loss=loss, tokenizer=_bpe(), device=DEV)
        return built[key]

    yield make
    for c in built.values():
        c.encoder.close()


def _spans(texts, rng, block=BLOCK):
    out = []
    for text in texts:
        start = int(rng.integers(0, max(len(text) - 16 * block, 0) + 1))
        out.append(text[start:start + 16 * block])
    return out


def _same_dict(got, want, what=None):
    for key, dt in (("input_ids", torch.int64), ("labels", torch.int64), ("attention_mask", torch.int64), ("byte_lengths", torch.int64), ("ids_to_embed", torch.int64),
                    ("target_surface_forms", None), ("target_priors", torch.float32), ("mask", torch.bool)):
        g, w = got[key].cpu(), torch.from_numpy(np.asarray(want[key]))
        w = w.to(g.dtype if dt is None else dt)
        assert (dt is None or g.dtype == dt) and g.shape == w.shape and torch.equal(g, w), (what, key)
    assert got["special_indices"] == [int(x) for x in want["special_indices"]], what
    m = torch.stack([got["metrics"]["avg_byte_length"], got["metrics"]["unk_ratio"]]).cpu().numpy()
    assert m.dtype == np.float64 and m.tobytes() == want["metrics"].tobytes(), what
    assert torch.equal(got["label_record"].cpu(), torch.from_numpy(want["record"]))


@pytest.mark.parametrize("loss,n,mode", (("mlm", 256, "random"), ("mlm", 256, "positives_only"), ("clm", None, "random"), ("mlm", None, "random"), ("clm", 256, "random")))
def test_collator_with_a_fixed_tokenizer_equals_the_host_path(fixed, loss, n, mode):
    """The converted tokenizer's own call on the host, then the restatement, against one DeviceCollator call; 554 ids are no multiple of 8."""
    seed = 5
    c = fixed(loss, n_token_subsample=n, subsample_mode=mode)
    got = c([{"texts": _texts(), "lang_code": "en"}], seed=seed)
    texts = _spans(_texts(), np.random.default_rng(seed))
    assert len(texts[-1]) == 16 * BLOCK
    enc = c.tokenizer(texts, max_length=BLOCK, truncation=True, padding="max_length", return_tensors="np", add_special_tokens=True)
    v = len(c.tokenizer)
    assert v == 554 and c.original_length == 421 and c.special_ids == [0, 2, 3, 1, 420]
    order = c.negative_order(seed, v).cpu().numpy() if n is not None and mode == "random" else None
    want = cr.encode(enc["input_ids"], c.special_ids, c.byte_lengths.cpu().numpy(), c.surface_forms.cpu().numpy(), c.scores.cpu().numpy(), loss=loss, mask_token_id=420,
                     unk_token_id=3, seed=derived_seed(seed, 0), n_token_subsample=n, subsample_mode=mode, negative_order=order)
    want["attention_mask"] = enc["attention_mask"]
    _same_dict(got, want, (loss, n, mode))
    assert got["target_surface_forms"].dtype == torch.int32 and got["target_surface_forms"].shape[1] == MAXLEN
    assert got["special_indices_in_reference"] == [0, 2, 3, 1, 420] and got["lang_code"] == "en" and int(got["lang_index"]) == 1 and not got["lang_index"].is_cuda
    if loss == "mlm":
        assert int(got["label_record"][4]) > 0
    again = c([{"texts": _texts(), "lang_code": "en"}], seed=seed)          # the same (data, seed, rng state): the same bits
    for key in ("input_ids", "labels", "ids_to_embed", "target_surface_forms", "target_priors", "byte_lengths"):
        assert torch.equal(got[key], again[key]), key
    other = c([{"texts": _texts(), "lang_code": "en"}], seed=seed + 1)
    assert loss == "clm" or not torch.equal(got["labels"], other["labels"])


@pytest.mark.parametrize("name", cr.CALL_FIXTURES)
def test_collator_equals_the_reference_s_call_on_the_fixture_s_texts(name):
    """What the reference's ``Collator`` returned for these texts — its own ``__init__`` on a saved copy of the test tokenizer
    (``convert_to_byte_level``, the surface-form matrix, scores, byte lengths), its tokenizer call, ``encode`` — against one
    ``DeviceCollator`` call on the same texts; first the tables ``__init__`` prepared.  Padded branch: every array element for element.
    With n_token_subsample the reference shuffles with numpy's generator (other negatives) and under MLM lists -100 as an id (DESIGN.md
    section 7f): input_ids and labels are compared through ``ids_to_embed[.]``, the ids they stand for, and every row by its id."""
    inputs, ref, init = cr.load_call_fixture(name)
    n = inputs["n_token_subsample"]
    args = _args(n_token_subsample=n, subsample_mode=inputs["subsample_mode"], block_size=inputs["block_size"], hn_surface_maxlen=inputs["hn_surface_maxlen"],
                 pad_to_multiple_of=inputs["pad_to_multiple_of"], langs=inputs["langs"], sample_text_span=False)
    c = DeviceCollator(_bpe(), _bpe(False), args, loss=inputs["loss"], tokenizer=_bpe(), device=DEV)
    assert c.original_length == int(init["original_length"]) and c.special_ids == init["special_ids"].tolist()
    assert c.surface_forms.dtype == torch.int32 and np.array_equal(c.surface_forms.cpu().numpy(), init["surface_forms"])
    assert c.scores.cpu().numpy().tobytes() == init["scores"].tobytes() and np.array_equal(c.byte_lengths.cpu().numpy(), init["byte_lengths"])
    got = c([{"texts": inputs["texts"], "lang_code": inputs["lang_code"]}], seed=inputs["seed"])
    m = torch.stack([got["metrics"]["avg_byte_length"], got["metrics"]["unk_ratio"]]).cpu().numpy()
    assert m.tobytes() == ref["metrics"].tobytes()
    for key in ("attention_mask", "byte_lengths"):
        assert np.array_equal(got[key].cpu().numpy(), ref[key]), key
    assert got["special_indices"] == ref["special_indices"].tolist() and got["special_indices_in_reference"] == ref["special_indices_in_reference"].tolist()
    assert got["lang_code"] == inputs["lang_code"] and int(got["lang_index"]) == int(ref["lang_index"])
    ours = {k: got[k].cpu().numpy() for k in ("input_ids", "labels", "ids_to_embed", "target_surface_forms", "target_priors", "mask")}
    if n is None:
        for key, x in ours.items():
            assert np.array_equal(x, ref[key].astype(np.float32) if key == "target_priors" else ref[key]), key
        assert len(ours["mask"]) == 560 and ours["mask"].sum() == 554
        return
    assert len(ours["ids_to_embed"]) == len(ref["ids_to_embed"]) == n and ours["mask"].all() and ref["mask"].all()
    assert np.array_equal(ours["ids_to_embed"][ours["input_ids"]], ref["ids_to_embed"][ref["input_ids"]])
    on = ref["labels"] != -100
    assert on.any() and np.array_equal(on, ours["labels"] != -100)
    assert np.array_equal(ours["ids_to_embed"][ours["labels"][on]], ref["ids_to_embed"][ref["labels"][on]])
    in_batch = np.union1d(np.union1d(ref["ids_to_embed"][ref["input_ids"]], ref["ids_to_embed"][ref["labels"][on]]), init["special_ids"])
    assert np.isin(in_batch, ours["ids_to_embed"]).all() and len(np.unique(ours["ids_to_embed"])) == n          # the batch's ids and n - len(in_batch) distinct negatives
    rows = {int(i): r for r, i in enumerate(ours["ids_to_embed"])}
    shared = [(r, rows[int(i)]) for r, i in enumerate(ref["ids_to_embed"]) if int(i) in rows]
    assert len(shared) >= len(in_batch)
    for theirs, mine in shared:          # a row both lists hold carries the same surface form and the same prior
        assert np.array_equal(ref["target_surface_forms"][theirs], ours["target_surface_forms"][mine])
        assert np.float32(ref["target_priors"][theirs]) == ours["target_priors"][mine]
    c.encoder.close()


def test_collator_identity_batch(fixed):
    c = fixed("clm", n_token_subsample=256)
    a, b, other = c(None, True, seed=9), c(None, True, seed=9), c(None, True, seed=10)
    idx = a["ids_to_embed"].cpu()
    assert idx.shape == (256,) and len(set(idx.tolist())) == 256 and int(idx.min()) >= 0 and int(idx.max()) < c.original_length
    assert torch.equal(a["target_surface_forms"].cpu(), c.surface_forms.cpu()[idx]) and a["target_surface_forms"].dtype == c.surface_forms.dtype
    assert a["target_priors"].dtype == torch.float32 and not bool(a["target_priors"].any()) and a["target_priors"].shape == (256,)
    assert torch.equal(a["ids_to_embed"], b["ids_to_embed"]) and not torch.equal(a["ids_to_embed"], other["ids_to_embed"])
    assert a["lang_code"] is None and int(a["lang_index"]) == 0
    with pytest.raises(ValueError, match="n_token_subsample is None"):
        fixed("clm")(None, True, seed=9)


def test_collator_identity_batch_of_row_numbers(fixed):
    """No hn tokenizer: the surface forms are the int64 column arange(V), gathered through a [V, 2] float32 view — small integers are
    denormal bit patterns there, and the rows must come back as the same bits."""
    c = fixed("clm", hn=False, n_token_subsample=256)
    assert c.surface_forms.dtype == torch.int64 and c.surface_forms.shape == (554, 1)
    a = c(None, True, seed=3)
    assert a["target_surface_forms"].dtype == torch.int64 and a["target_surface_forms"].shape == (256, 1)
    assert torch.equal(a["target_surface_forms"][:, 0], a["ids_to_embed"]) and len(set(a["ids_to_embed"].tolist())) == 256


def test_collator_refusals_and_check_false(fixed):
    """check=False reads nothing back: a batch with more ids than n_token_subsample returns with the status bit set (the documented behaviour of
    subsample_batch_vocabulary(check=False)), where check=True raises."""
    with pytest.raises(NotImplementedError):
        DeviceCollator(_bpe(), None, _args(use_passthrough_hypernet=True), loss="clm", tokenizer=_bpe(), device=DEV)
    with pytest.raises(NotImplementedError):
        DeviceCollator(_bpe(), None, _args(n_token_subsample=64, subsample_mode="highest_scores"), loss="clm", tokenizer=_bpe(), device=DEV)
    with pytest.raises(ValueError, match="multiple"):
        DeviceCollator(_bpe(), None, _args(n_token_subsample=60), loss="clm", tokenizer=_bpe(), device=DEV)
    with pytest.raises(ValueError, match="mask token"):
        DeviceCollator(_bpe(False), None, _args(), loss="mlm", tokenizer=_bpe(False), device=DEV)
    with pytest.raises(ValueError, match="exactly when"):
        DeviceCollator(_bpe(), None, _args(), loss="clm", device=DEV)
    c = fixed("clm", n_token_subsample=8)
    data = [{"texts": _texts(), "lang_code": "fr"}]
    with pytest.raises(ValueError, match="more than n_token_subsample"):
        c(data, seed=1)
    got = c(data, seed=1, check=False)
    assert int(got["vocab_status"]) & BATCH_OVERFLOW and int(got["label_record"][7]) == 0 and int(got["lang_index"]) == 2
    torch.cuda.synchronize()


def test_collator_with_a_sampled_tokenizer_equals_the_host_path():
    """Tokenizer sampling (no noise), both vocabulary branches: the host-built path — sample_tokenizer, the library's tokenizer call, the
    restatement — against the device's, with n_total drawn from the same rng."""
    from zett_amd.tokenizer_sampling import DeviceTokenizerSampler, sample_tokenizer
    seed, reference, hn = 4, _bpe(), _bpe(False)
    texts = _texts()[:7]
    for n in (None, 256):
        args = _args(do_tokenizer_sampling=True, n_token_subsample=n, sample_text_span=False, add_prefix_space=True)
        host_sampler, sampler = (DeviceTokenizerSampler(table_capacity=1 << 14, max_depth=2, max_pieces=1 << 12) for _ in range(2))
        c = DeviceCollator(reference, hn, args, loss="mlm", samplers={"en": [sampler]}, device=DEV)
        got = c([{"texts": texts, "lang_code": "en"}], seed=seed)
        rng = np.random.default_rng(seed)
        assert int(rng.integers(0, 1)) == 0
        n_total = min(1536, max(1100, int(rng.normal(1200, 30))))
        tokenizer, special_ids_map, sf, priors, byte_lengths = sample_tokenizer(texts, host_sampler, reference, n_total=n_total, noise_std=0.0, add_prefix_space=True,
                                                                                 hn_tokenizer=hn, hn_surface_maxlen=MAXLEN)
        enc = tokenizer(texts, max_length=BLOCK, truncation=True, padding="max_length", return_tensors="np", add_special_tokens=True)
        ids = enc["input_ids"].copy()
        for k, v in special_ids_map.items():
            ids[ids == k] = v
        v = len(tokenizer)
        assert list(tokenizer.all_special_tokens) == list(reference.all_special_tokens)
        order = c.negative_order(seed, v).cpu().numpy() if n is not None else None
        want = cr.encode(ids, [int(i) for i in tokenizer.all_special_ids], np.asarray(byte_lengths), np.asarray(sf), np.asarray(priors, dtype=np.float64), loss="mlm",
                         mask_token_id=tokenizer.mask_token_id, unk_token_id=tokenizer.unk_token_id, seed=derived_seed(seed, 0), n_token_subsample=n, negative_order=order,
                         tokenizer_sample_max=1536)
        want["attention_mask"] = enc["attention_mask"]
        _same_dict(got, want, n)
        assert got["target_priors"].shape == ((1536 + 8,) if n is None else (256,))
        host_sampler.close()
        sampler.close()
        c.vocabulary.close()


def test_collator_in_front_of_an_mlm_step_of_the_tiny_hypernet(fixed):
    """collator -> hypernet -> splice -> lookup -> a toy backbone -> lm_head_loss(mode="mlm"): a finite loss, and gradients that reach the
    hypernetwork's outputs."""
    from zett_amd import synth
    from zett_amd.config import ZettHypernetConfig
    from zett_amd.hypernet import ZettHypernet
    from zett_amd.training import lm_head_loss, splice_special_rows, token_embeddings
    cfg, *_ = synth.workload("tiny")
    cfg = dict(cfg, original_vocab_size=420, vocab_size=425)          # the hn tokenizer's 420 ids
    e = cfg["n_embd"]
    model = ZettHypernet(ZettHypernetConfig(**cfg))
    model.load_state_dict({k: torch.from_numpy(x) for k, x in synth.make_weights(cfg, seed=83).items()})
    model = model.to(DEV).requires_grad_(True).train()
    src = torch.from_numpy(synth.make_source_embeddings(cfg, 83)).to(DEV)
    c = fixed("mlm", n_token_subsample=256)
    batch = c([{"texts": _texts(), "lang_code": "fr"}], seed=21)
    assert int(batch["label_record"][4]) > 0 and int(batch["vocab_status"]) == 0
    tap = {}
    pred_in, pred_out, _bias = model(batch["target_surface_forms"], source_embeddings=src, lang_index=batch["lang_index"])
    pred_in.register_hook(lambda g: tap.__setitem__("d pred_in", g.clone()))
    pred_out.register_hook(lambda g: tap.__setitem__("d pred_out", g.clone()))
    reference_rows = torch.cat([src, src[:8].flip(0)])          # (row 420: the reference's <mask>)
    pred_in, pred_out = splice_special_rows(pred_in, pred_out, reference_rows, batch["special_indices"], batch["special_indices_in_reference"], inplace=True)
    x = token_embeddings(pred_in, batch["input_ids"])
    mix = (torch.randn(e, e, generator=torch.Generator().manual_seed(1)) / e ** 0.5).to(DEV)
    hidden = x + torch.tanh(x @ mix)
    loss = lm_head_loss(hidden, pred_out, batch["labels"], batch["attention_mask"], mode="mlm", priors=batch["target_priors"], vocab_mask=batch["mask"], precision="f32")[0]
    loss.backward()
    assert bool(torch.isfinite(loss)) and set(tap) == {"d pred_in", "d pred_out"}
    for key, g in tap.items():
        assert bool(torch.isfinite(g).all()) and bool(g.any()), key
