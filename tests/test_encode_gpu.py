"""zett_amd.text_encode.DeviceTextEncoder on the GPU (csrc/text_encode.hip), everything through the C ABI: torch.equal against the
reference's own outputs (tests/golden/encode_*.json.gz) and against the restatement of tests/encode_ref.py — which
tests/test_encode_host.py holds to those outputs and to the installed library — with segmentation from oracle/retok_ref.py."""
import copy

import numpy as np
import pytest
import torch

from tests import encode_ref as er
from zett_amd import training
from zett_amd.text_encode import ENCODE_NO_UNK, DeviceTextEncoder

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INTS = (torch.int32, torch.int64)
UNIGRAM, BPE = "encode_unigram_prefix_bos_eos_t32", "encode_bpe_prefix_bos_eos_t32"
_ENCODERS = {}


def _encoder(name):
    enc = _ENCODERS.get(name)
    if enc is None:
        fx = er.load_fixture(name)
        enc = _ENCODERS[name] = DeviceTextEncoder.from_tokenizer_json(fx["tokenizer"], fx["pad_token_id"], fx["special_tokens"], fx["special_ids"], fx["padding_side"],
                                                                      fx["truncation_side"], device=DEV)
    return enc


def _same(got, ids, mask, dtype=torch.int64, what=None):
    for key, want in (("input_ids", ids), ("attention_mask", mask)):
        g, w = got[key].cpu(), torch.from_numpy(np.asarray(want)).to(dtype)
        assert g.dtype == dtype and g.shape == w.shape and torch.equal(g, w), (what, key, (g != w).nonzero()[:4].tolist() if g.shape == w.shape else (g.shape, w.shape))


@pytest.mark.parametrize("name", er.FIXTURES)
@pytest.mark.parametrize("dtype", INTS, ids=("i32", "i64"))
def test_fixtures_of_the_reference(name, dtype):
    """The reference's own rows; then into a row stride that rules the 16-byte stores out (T + 3) and one that allows them (T + 4): the
    padding columns keep their fill."""
    fx = er.load_fixture(name)
    enc, t = _encoder(name), fx["block_size"]
    _same(enc(fx["texts"], t, fx["map"], dtype=dtype), fx["input_ids"], fx["attention_mask"], dtype, name)
    for pad in (3, 4):
        wide = [torch.full((len(fx["texts"]), t + pad), -7, dtype=dtype, device=DEV) for _ in range(2)]
        got = enc(fx["texts"], t, fx["map"], dtype=dtype, out=(wide[0][:, :t], wide[1][:, :t]))
        _same(got, fx["input_ids"], fx["attention_mask"], dtype, (name, pad))
        assert got["input_ids"].data_ptr() == wide[0].data_ptr() and all(bool((w[:, t:] == -7).all()) for w in wide)


@pytest.mark.parametrize("name", (UNIGRAM, "encode_unigram_noprefix_bos_t8", BPE, "encode_bpe_noprefix_nopost_t8"))
@pytest.mark.parametrize("shape", ((1, 4), (7, 8), (300, 32)), ids=("1x4", "7x8", "300x32"))
def test_random_texts_against_the_restatement(name, shape):
    fx = er.load_fixture(name)
    b, t = shape
    rng = np.random.default_rng(20240)          # (the texts of tests/test_encode_host.py's split test)
    texts = [er.random_text(rng) for _ in range(300)][:b]
    ids, mask = er.encode_with(fx["spec"], fx["segment"], texts, t, fx["map"])
    got = _encoder(name)(texts, t, fx["map"])
    _same(got, ids, mask, what=(name, shape))
    if b == 300:          # the same bits on a second run
        again = _encoder(name)(texts, t, fx["map"])
        assert torch.equal(again["input_ids"], got["input_ids"]) and torch.equal(again["attention_mask"], got["attention_mask"])


@pytest.mark.parametrize("name", (UNIGRAM, BPE))
def test_long_word_and_many_words(name):
    """One word of 5 000 bytes (its state does not fit LDS: the global scratch) and 5 000 words of one byte (a text across several
    segments of the scan), both whole in a row of 8 192."""
    fx = er.load_fixture(name)
    texts = ["then" * 1250, "a1" * 2500, "x"]
    assert max(len(w) for w in er.split_words(texts[0], True)) == 5000 and len(er.split_words(texts[1], True)) == 5000
    ids, mask = er.encode_with(fx["spec"], fx["segment"], texts, 8192)
    assert mask[0].sum() > 1000 and mask[1].sum() > 5000 and mask[:2].sum(1).max() < 8192
    _same(_encoder(name)(texts, 8192), ids, mask, what=name)
    ids, mask = er.encode_with(fx["spec"], fx["segment"], texts, 32)
    _same(_encoder(name)(texts, 32, dtype=torch.int32), ids, mask, torch.int32, what=(name, 32))


def test_more_than_1024_scan_segments():
    """2^20 + 1500 texts, all empty but four: 1026 segments of 1024 positions, so the workgroup that scans the segment counts takes a
    second round, whose offsets start from the first round's total (the carry).  Every empty text is one dead word whatever the carry;
    the words of the two texts behind position 2^20 come out right only if it is.  The rows of the four distinct texts come from the
    restatement and are placed with numpy.  The call's workspace is 188 MB (zett_encode_workspace_bytes(31, 2^20 + 1500) = 187 977 744)."""
    fx = er.load_fixture(UNIGRAM)
    b, t = (1 << 20) + 1500, 8
    distinct = ["", "hello world", "it's 12", " x"]
    which = np.zeros(b, dtype=np.int64)
    which[[0, (1 << 20) - 1, (1 << 20) + 3, b - 1]] = [1, 2, 3, 1]
    texts = [distinct[k] for k in which.tolist()]
    assert sum(map(len, texts)) + b > (1 << 20) + 1024
    ids, mask = er.encode_with(fx["spec"], fx["segment"], distinct, t)
    assert len({tuple(r) for r in ids.tolist()}) == 4 and (mask.sum(1)[1:] > mask.sum(1)[0]).all()
    _same(_encoder(UNIGRAM)(texts, t, dtype=torch.int32), ids[which], mask[which], torch.int32, "2^20 + 1500 texts")


def test_no_texts_and_empty_texts():
    enc, fx = _encoder(UNIGRAM), er.load_fixture(UNIGRAM)
    got = enc([], 8)
    assert got["input_ids"].shape == (0, 8) and got["attention_mask"].shape == (0, 8) and got["input_ids"].dtype == torch.int64
    for texts in ([""], [""] * 70):
        ids, mask = er.encode_with(fx["spec"], fx["segment"], texts, 8)
        assert mask.sum() == 2 * len(texts)
        _same(enc(texts, 8), ids, mask, what=len(texts))
    fx = er.load_fixture("encode_bpe_noprefix_nopost_t8")
    _same(_encoder("encode_bpe_noprefix_nopost_t8")(["", ""], 5), np.full((2, 5), fx["pad_token_id"]), np.zeros((2, 5)), what="all pads")


def test_one_id_of_room():
    """n_prefix + n_suffix = T - 1"""
    enc, fx = _encoder(UNIGRAM), er.load_fixture(UNIGRAM)
    texts = ["", "hello world", " ", "it's"]
    ids, mask = er.encode_with(fx["spec"], fx["segment"], texts, 3)
    assert mask.sum(1).tolist() == [2, 3, 3, 3]
    _same(enc(texts, 3), ids, mask)
    with pytest.raises(ValueError):
        enc(texts, 2)


def test_missing_unk_sets_the_status_bit():
    """A Unigram model without unk_id and without the piece of a byte the text holds: the library raises; here the status bit is set,
    check=True raises, check=False does not wait and does not raise."""
    fx = er.load_fixture(UNIGRAM)
    data = copy.deepcopy(fx["tokenizer"])
    assert data["model"]["unk_id"] is None
    data["model"]["vocab"] = [p for p in data["model"]["vocab"] if p[0] != "q"]
    enc = DeviceTextEncoder.from_tokenizer_json(data, fx["pad_token_id"], fx["special_tokens"], fx["special_ids"], device=DEV)
    fine = enc(["a b c"], 8)
    assert int(enc.last_status.item()) == 0 and int(fine["attention_mask"].sum()) > 2
    with pytest.raises(Exception, match="unk_id"):
        enc(["a b c", "a q c"], 8)
    got = enc(["a b c", "a q c"], 8, check=False)
    assert got["input_ids"].shape == (2, 8)
    assert int(enc.last_status.item()) & ENCODE_NO_UNK
    enc.close()


def test_chain_into_the_batch_vocabulary():
    """encode_texts -> subsample_batch_vocabulary gives the bits of the same call fed from the fixture's ids."""
    fx = er.load_fixture(UNIGRAM)
    v = len(fx["tokenizer"]["model"]["vocab"])
    rng = np.random.default_rng(3)
    sf = torch.from_numpy(rng.integers(0, 1000, (v, 5))).to(DEV)
    priors = torch.from_numpy(rng.standard_normal(v).astype(np.float32)).to(DEV)
    order = torch.from_numpy(rng.permutation(v)).to(DEV)
    batch = training.encode_texts(_encoder(UNIGRAM), fx["texts"], fx["block_size"], fx["map"], check=False)
    want_ids = torch.tensor(fx["input_ids"], device=DEV)
    n = 256
    assert n <= v and len(np.unique(fx["input_ids"])) + len(fx["special_ids"]) <= n
    got = training.subsample_batch_vocabulary(batch["input_ids"], batch["input_ids"], fx["special_ids"], n, sf, priors, negative_order=order)
    want = training.subsample_batch_vocabulary(want_ids, want_ids, fx["special_ids"], n, sf, priors, negative_order=order)
    for key in ("input_ids", "labels", "ids_to_embed", "target_surface_forms", "target_priors", "mask", "n_positive", "status"):
        assert torch.equal(getattr(got, key), getattr(want, key)), key
    assert got.special_indices == want.special_indices
    assert training.DeviceTextEncoder is DeviceTextEncoder


def _texts_of_bytes(n_text):
    """three ASCII texts of n_text bytes together"""
    src = "the quick brown fox it's 12 345 times, we'll see. " * (n_text // 50 + 1)
    a, b = n_text // 3, n_text // 2
    return [src[:a], src[a:a + b], src[a + b:n_text]]


@pytest.mark.parametrize("positions", (15, 16, 17, 1023, 1024, 1025, "empty"))
def test_c_abi_stays_inside_a_framed_workspace(positions):
    """Straight through the C ABI with a workspace of exactly zett_encode_workspace_bytes between two 4096-byte guards: n_text + n_texts
    at the rounding edges of the workspace's arrays and of one scan segment.  The guards keep their fill, the status word is 0 and the
    outputs are the wrapper's."""
    import ctypes as C
    enc, fx = _encoder(UNIGRAM), er.load_fixture(UNIGRAM)
    texts = [""] if positions == "empty" else _texts_of_bytes(positions - 3)
    blob = "".join(texts).encode()
    b, t, guard = len(texts), 8, 4096
    assert positions == "empty" or len(blob) + b == positions
    want = enc(texts, t, fx["map"])
    off = torch.tensor(np.cumsum([0] + [len(x.encode()) for x in texts]), dtype=torch.int64, device=DEV)
    text = torch.tensor(list(blob or b"\0"), dtype=torch.uint8, device=DEV)
    need = enc.workspace_bytes(len(blob), b)
    frame = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=DEV)
    assert frame.data_ptr() % 16 == 0 and need % 16 == 0
    ids = torch.full((b, t), -7, dtype=torch.int64, device=DEV)
    mask = torch.full((b, t), -7, dtype=torch.int64, device=DEV)
    status = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    pairs = [(int(k), int(v)) for k, v in (fx["map"] or {}).items()]
    m_from, m_to = (C.c_int32 * max(len(pairs), 1))(*[p[0] for p in pairs]), (C.c_int32 * max(len(pairs), 1))(*[p[1] for p in pairs])
    P = lambda x: C.c_void_p(x.data_ptr())          # noqa: E731
    rc = enc.lib.zett_encode_texts(enc.retok.handle, P(text), P(off), b, len(blob), P(enc._d_table), len(enc.table), enc.spec.flags, enc.spec.prefix_mode, t,
                                   enc._prefix, len(enc.spec.prefix_ids), enc._suffix, len(enc.spec.suffix_ids), m_from, m_to, len(pairs), enc.spec.pad_id, P(ids), P(mask), 8, t,
                                   C.c_void_p(frame.data_ptr() + guard), need, P(status), C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    assert rc == 0, enc.lib.zett_last_error()
    torch.cuda.synchronize()
    assert bool((frame[:guard] == 0xA5).all()) and bool((frame[guard + need:] == 0xA5).all())
    assert int(status.item()) == 0
    assert torch.equal(ids, want["input_ids"]) and torch.equal(mask, want["attention_mask"])
