"""``DeviceTextEncoder(split_added_tokens=True)`` on the GPU (the cut step of csrc/text_words.hip.h, zett_encode_texts_added):
torch.equal against the restatement of tests/encode_added_ref.py and against rows built from the installed library's ids, at the
smallest shapes where the cut can go wrong.  tests/test_encode_added_host.py holds the restatement to the library on the host."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import encode_added_ref as ar
from tests import encode_ref as er
from zett_amd import _lib, training
from zett_amd.text_encode import ENCODE_BAD_TABLE, MAX_ADDED_TOKEN_BYTES, MAX_ADDED_TOKENS, DeviceTextEncoder

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
INTS = (torch.int32, torch.int64)
ALWAYS, NONE_U, UNLESS, NONE_B = "encode_unigram_prefix_bos_eos_t32", "encode_unigram_noprefix_bos_t8", "encode_bpe_prefix_bos_eos_t32", "encode_bpe_noprefix_nopost_t8"
NAMES = (ALWAYS, NONE_U, UNLESS, NONE_B)
_MADE = {}


def _vocab(name):
    return len(er.load_fixture(name)["tokenizer"]["model"]["vocab"])


def _tokens(name, kind="few"):
    v = _vocab(name)
    if kind == "few":          # </s> at its own row of the vocabulary, the overlap set, a multi-byte token
        return [("</s>", 2), ("<x>", v), ("<x><y>", v + 1), ("x><", v + 2), ("<é中>", v + 3)]
    if kind == "shared_prefix":
        return [("<|%d|>" % k, v + k) for k in range(256)]
    if kind == "cap":
        return [("<|%d|>" % k, v + k) for k in range(MAX_ADDED_TOKENS - 1)] + [("<" + "a" * (MAX_ADDED_TOKEN_BYTES - 2) + ">", v + MAX_ADDED_TOKENS - 1)]
    raise KeyError(kind)


def _made(name, kind="few"):
    """(encoder, the library's tokenizer, fixture), once per (fixture, token list)"""
    got = _MADE.get((name, kind))
    if got is None:
        fx = er.load_fixture(name)
        data = ar.with_added_tokens(fx["tokenizer"], _tokens(name, kind))
        enc = DeviceTextEncoder.from_tokenizer_json(data, fx["pad_token_id"], fx["special_tokens"], fx["special_ids"], fx["padding_side"], fx["truncation_side"], device=DEV,
                                                    split_added_tokens=True)
        got = _MADE[(name, kind)] = (enc, ar.library(data), fx)
    return got


def _library_rows(tk, spec, texts, t, id_map):
    cap = t - len(spec.prefix_ids) - len(spec.suffix_ids)
    ids = np.full((len(texts), t), spec.pad_id, dtype=np.int64)
    mask = np.zeros((len(texts), t), dtype=np.int64)
    for r, text in enumerate(texts):
        row = list(spec.prefix_ids) + tk.encode(text, add_special_tokens=False).ids[:cap] + list(spec.suffix_ids)
        ids[r, :len(row)] = row
        mask[r, :len(row)] = 1
    for key, value in (id_map or {}).items():
        ids[ids == key] = value
    return ids, mask


def _same(got, ids, mask, dtype=torch.int64, what=None):
    for key, want in (("input_ids", ids), ("attention_mask", mask)):
        g, w = got[key].cpu(), torch.from_numpy(np.asarray(want)).to(dtype)
        assert g.dtype == dtype and g.shape == w.shape and torch.equal(g, w), (what, key, (g != w).nonzero()[:4].tolist() if g.shape == w.shape else (g.shape, w.shape))


def _check(name, texts, t, id_map=None, dtype=torch.int64, kind="few", library=True):
    """the device against the restatement and against the library; returns the restatement's rows"""
    enc, tk, fx = _made(name, kind)
    ids, mask = ar.encode_with(enc.spec, fx["segment"], texts, t, id_map)
    if library:
        lib_ids, lib_mask = _library_rows(tk, enc.spec, texts, t, id_map)
        assert np.array_equal(ids, lib_ids) and np.array_equal(mask, lib_mask), (name, "the restatement is not the library")
    _same(enc(texts, t, id_map, dtype=dtype), ids, mask, dtype, (name, t))
    return ids, mask


EDGES = [
    "</s>",                                                   # a text that is one match
    "</s>a b", "a b</s>",                                     # a match at the start, at the end
    "</s></s>", "a</s></s></s>b", "</s></s>a",                # two and three adjacent matches
    "a<x><y>b", "<x><x><y>", "a<x><", "<<x>>", "x><x>", "<x><y><x>x><",          # the overlap set
    "ends <", "/s> starts",                                   # a token string across the boundary of two texts: in neither
    "ends </", "", "s> starts",                               # and across an empty text
    "<x", "", "", ">",
    "a</s> b", "a</s>b", "a</s>", " </s>", "</s> ", "</s> </s>", " </s> ", "</s>  b",          # sections that start with U+0020, that do not, that are empty
    "a  </s>  b", "a\n\n</s>\t\tb", "a </s>",                 # a whitespace run in front of a match
    "a</s>'s", "x</s>'ll do", "</s>'re'd",                    # a contraction straight behind a match
    "中</s>é", "é</s>\U0001F600", "\u0301</s>\u0301",          # a multi-byte character on both sides
    "a<é中>b", "<é中>", "<é中", "é中>", "中<é中>中",              # a token whose own content is multi-byte
    "", " ", "plain text, it's 12",
]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("dtype", INTS, ids=("i32", "i64"))
def test_edges_of_the_cut(name, dtype):
    ids, _ = _check(name, EDGES, 16, dtype=dtype)
    v = _vocab(name)
    spec = _made(name)[0].spec
    n_pre = len(spec.prefix_ids)
    assert ids[0, n_pre] == 2 and (ids[6] == v + 1).sum() == 1 and not (ids[6] == v).any()
    for r in (12, 13, 14, 15, 16, 17, 18, 19, 20):          # no match in a string that spans texts
        assert not (ids[r] >= v).any() and (ids[r] == 2).sum() == spec.suffix_ids.count(2)
    _check(name, EDGES[::-1], 16, dtype=dtype)
    for text in EDGES[:12]:          # every text alone: one text, one block
        _check(name, [text], 16, dtype=dtype)


@pytest.mark.parametrize("name", NAMES)
def test_truncation_at_the_match(name):
    """the match is the last id that fits, then the first id cut"""
    enc, tk, fx = _made(name)
    v, spec = _vocab(name), enc.spec
    text = "ab 12<x>cd"
    seq = ar.text_ids(text, {c: i for c, i in _tokens(name)}, spec.prefix_mode, spec.marks_are_letters, fx["segment"], spec.resplit)
    k = seq.index(v)
    assert 0 < k < len(seq) - 1
    room = len(spec.prefix_ids) + len(spec.suffix_ids)
    fits, _ = _check(name, [text, "<x>", "a"], room + k + 1)
    assert fits[0, len(spec.prefix_ids) + k] == v
    cut, _ = _check(name, [text, "<x>", "a"], room + k)
    assert v not in cut[0] and v in cut[1]


@pytest.mark.parametrize("name", (ALWAYS, NONE_B))
def test_special_ids_map_hits_a_split_out_id(name):
    v = _vocab(name)
    ids, _ = _check(name, ["a<x>b</s>", "<x><y>"], 12, {v: 7, 7: 9, 2: 5})
    assert not (ids == v).any() and not (ids == 7).any() and (ids[0] == 9).sum() >= 1 and (ids == v + 1).sum() == 1 and not (ids == 2).any()


FILL = "the quick brown fox it's 12 345 times, we'll see. "


@pytest.mark.parametrize("name", (ALWAYS, NONE_B))
@pytest.mark.parametrize("positions", (1023, 1024, 1025, 1027))
def test_match_at_the_edge_of_a_scan_segment(name, positions):
    """n_text + n_texts at the edges of a scan segment of 1024 positions, the text's last four bytes a match; 1027: a match on positions
    1022 .. 1025 with text behind it"""
    if positions == 1027:
        texts = [(FILL * 21)[:1021] + "</s>b"]
        assert len(texts[0]) + 1 == positions
    else:
        n = positions - 3 - 8
        texts = [(FILL * 21)[:n // 2] + "</s>", "", (FILL * 21)[:n - n // 2] + "</s>"]
    assert sum(len(x) for x in texts) + len(texts) == positions
    _check(name, texts, 512, dtype=torch.int32)


@pytest.mark.parametrize("name", (NONE_U, NONE_B))
def test_match_at_the_staging_edge_of_the_words_kernel(name):
    """64 words — the dead slot, a word of k bytes, 61 of 64 bytes and the match's 3 positions — are 3908 + k bytes: the wave stages
    them in LDS up to 4096 and reads global memory beyond, and the match is the wave's last word either way"""
    for k in range(185, 192):
        text = "y" * k + (" " + "y" * 63) * 61 + "</s> z z"
        _check(name, [text], 4096, library=(k == 188))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("shape", ((1, 4), (7, 8), (300, 32)), ids=("1x4", "7x8", "300x32"))
def test_random_texts(name, shape):
    enc, tk, fx = _made(name)
    b, t = shape
    rng = np.random.default_rng(20241)          # (the texts of tests/test_encode_added_host.py)
    strings = [c for c, _ in _tokens(name)]
    texts = [ar.random_text(rng, strings) for _ in range(300)][:b] if b > 1 else ["a<x></s>'s\n"]
    _check(name, texts, t, fx["map"])
    if b == 300:          # the same bits on a second run
        one, two = enc(texts, t, fx["map"]), enc(texts, t, fx["map"])
        assert torch.equal(one["input_ids"], two["input_ids"]) and torch.equal(one["attention_mask"], two["attention_mask"])


@pytest.mark.parametrize("kind", ("shared_prefix", "cap"))
def test_large_tables(kind):
    """256 tokens behind ``<|``; a table at the cap, its longest token at the byte cap"""
    name = UNLESS
    strings = [c for c, _ in _tokens(name, kind)]
    rng = np.random.default_rng(11)
    picks = [strings[i] for i in rng.integers(0, len(strings), size=40)] + [strings[0], strings[-1], strings[-1][:-1], "<|", "<|12", "<|12|", "|>"]
    texts = [ar.random_text(rng, picks, 12) for _ in range(60)] + ["<|1|><|11|><|111|>", strings[-1] * 2, strings[-1][:-1] + "<|7|>"]
    ids, _ = _check(name, texts, 48, kind=kind)
    v = _vocab(name)
    assert (ids[-3, 1:4] == np.array([v + 1, v + 11, v + 111])).all() and (ids >= v).sum() > 20


def _abi_call(enc, texts, t, table, frame_guard=4096, n_added=None, pairs=()):
    """zett_encode_texts_added straight through the C ABI inside a framed workspace of exactly its queried size; table: (bytes, offsets,
    ids) as numpy arrays or None"""
    blob = "".join(texts).encode()
    b = len(texts)
    off = torch.tensor(np.cumsum([0] + [len(x.encode()) for x in texts]), dtype=torch.int64, device=DEV)
    text = torch.tensor(list(blob or b"\0"), dtype=torch.uint8, device=DEV)
    n = (len(table[2]) if table else 0) if n_added is None else n_added
    need = C.c_int64(0)
    rc = enc.lib.zett_encode_added_workspace_bytes(len(blob), b, n, C.byref(need))
    if rc != 0:
        return rc, None
    need = need.value
    frame = torch.full((need + 2 * frame_guard,), 0xA5, dtype=torch.uint8, device=DEV)
    ids = torch.full((b, t), -7, dtype=torch.int64, device=DEV)
    mask = torch.full((b, t), -7, dtype=torch.int64, device=DEV)
    status = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    m_from, m_to = (C.c_int32 * max(len(pairs), 1))(*[p[0] for p in pairs]), (C.c_int32 * max(len(pairs), 1))(*[p[1] for p in pairs])
    P = lambda x: C.c_void_p(0 if x is None else x.data_ptr())          # noqa: E731
    dev = [torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV) for a in table] if table else [None, None, None]
    n_bytes = int(len(table[0])) if table else 0
    rc = enc.lib.zett_encode_texts_added(enc.retok.handle, P(text), P(off), b, len(blob), P(enc._d_table), len(enc.table), enc.spec.flags, enc.spec.prefix_mode, t,
                                         enc._prefix, len(enc.spec.prefix_ids), enc._suffix, len(enc.spec.suffix_ids), m_from, m_to, len(pairs), enc.spec.pad_id, P(ids), P(mask), 8, t,
                                         P(dev[0]), P(dev[1]), P(dev[2]), n, n_bytes, C.c_void_p(frame.data_ptr() + frame_guard), need, P(status),
                                         C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc, dict(ids=ids, mask=mask, status=int(status.item()) if rc == 0 else None, need=need,
                    guards=bool((frame[:frame_guard] == 0xA5).all()) and bool((frame[frame_guard + need:] == 0xA5).all()))


def _table(enc):
    raw, offsets, ids = enc.spec.added_table()
    return np.frombuffer(raw, dtype=np.uint8), offsets, ids


@pytest.mark.parametrize("positions", (15, 16, 17, 1023, 1024, 1025, "empty"))
def test_c_abi_stays_inside_a_framed_workspace(positions):
    enc, tk, fx = _made(ALWAYS)
    if positions == "empty":
        texts = [""]
    else:
        n = positions - 3 - 4
        src = ("it's </s>12<x><y> we'll<x>see. " * (n // 30 + 2))
        texts = [src[:n // 3], src[n // 3:n // 3 + n // 2], src[n // 3 + n // 2:n] + "</s>"]
        assert sum(len(x) for x in texts) + 3 == positions
    want = enc(texts, 8, fx["map"])
    pairs = [(int(k), int(v)) for k, v in (fx["map"] or {}).items()]
    rc, got = _abi_call(enc, texts, 8, _table(enc), pairs=pairs)
    assert rc == 0, enc.lib.zett_last_error()
    assert got["guards"] and got["status"] == 0 and got["need"] % 16 == 0
    assert torch.equal(got["ids"], want["input_ids"]) and torch.equal(got["mask"], want["attention_mask"])
    ids, mask = ar.encode_with(enc.spec, fx["segment"], texts, 8, fx["map"])
    _same(want, ids, mask)


@pytest.mark.parametrize("name", (ALWAYS, UNLESS))
def test_count_zero_gives_the_bits_of_zett_encode_texts(name):
    """with no table the new entry point is the old one: same workspace size, same rows — also through an encoder whose tokenizer has
    no added token, where the strings of the special tokens are text"""
    fx = er.load_fixture(name)
    plain = DeviceTextEncoder.from_tokenizer_json(fx["tokenizer"], fx["pad_token_id"], fx["special_tokens"], fx["special_ids"], device=DEV)
    rng = np.random.default_rng(20240)
    texts = [er.random_text(rng) for _ in range(70)]
    want = plain(texts, 16, fx["map"])
    pairs = [(int(k), int(v)) for k, v in (fx["map"] or {}).items()]
    rc, got = _abi_call(plain, texts, 16, None, pairs=pairs)
    assert rc == 0, plain.lib.zett_last_error()
    assert got["guards"] and got["status"] == 0 and got["need"] == plain.workspace_bytes(sum(len(x.encode()) for x in texts), len(texts))
    assert torch.equal(got["ids"], want["input_ids"]) and torch.equal(got["mask"], want["attention_mask"])
    bare = DeviceTextEncoder.from_tokenizer_json(ar.with_added_tokens(fx["tokenizer"], []), fx["pad_token_id"], fx["special_tokens"], fx["special_ids"], device=DEV,
                                                 split_added_tokens=True)
    again = bare(texts + ["a</s>b"], 16, fx["map"])
    assert torch.equal(again["input_ids"][:-1], want["input_ids"]) and torch.equal(again["attention_mask"][:-1], want["attention_mask"])
    ids, mask = er.encode_with(fx["spec"], fx["segment"], ["a</s>b"], 16, fx["map"])          # the eos string as text
    _same({k: x[-1:] for k, x in again.items()}, ids, mask)
    with pytest.raises(NotImplementedError):
        plain(["a</s>b"], 16)          # the default mode refuses as before
    plain.close()
    bare.close()


def test_refusals_before_any_launch():
    enc, tk, fx = _made(UNLESS)
    table = _table(enc)
    texts = ["a</s>b"]
    assert _abi_call(enc, texts, 8, table)[0] == 0
    over = C.c_int64(0)
    assert enc.lib.zett_encode_added_workspace_bytes(8, 1, MAX_ADDED_TOKENS + 1, C.byref(over)) != 0
    assert enc.lib.zett_encode_added_workspace_bytes(8, 1, MAX_ADDED_TOKENS, C.byref(over)) == 0
    assert enc.lib.zett_encode_added_workspace_bytes(8, 1, 1, None) != 0

    def call(table, n, n_bytes=None, work_short=0):
        blob = texts[0].encode()
        off = torch.tensor([0, len(blob)], dtype=torch.int64, device=DEV)
        text = torch.tensor(list(blob), dtype=torch.uint8, device=DEV)
        need = C.c_int64(0)
        assert enc.lib.zett_encode_added_workspace_bytes(len(blob), 1, min(max(n, 0), MAX_ADDED_TOKENS), C.byref(need)) == 0
        work = torch.zeros(need.value, dtype=torch.uint8, device=DEV)
        ids = torch.full((1, 8), -7, dtype=torch.int64, device=DEV)
        mask = torch.full((1, 8), -7, dtype=torch.int64, device=DEV)
        status = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        P = lambda x: C.c_void_p(0 if x is None else x.data_ptr())          # noqa: E731
        one = (C.c_int32 * 1)(0)
        rc = enc.lib.zett_encode_texts_added(enc.retok.handle, P(text), P(off), 1, len(blob), P(enc._d_table), len(enc.table), enc.spec.flags, enc.spec.prefix_mode, 8,
                                             enc._prefix, len(enc.spec.prefix_ids), enc._suffix, len(enc.spec.suffix_ids), one, one, 0, enc.spec.pad_id, P(ids), P(mask), 8, 8,
                                             P(table[0]), P(table[1]), P(table[2]), n, len(dev[0]) if n_bytes is None else n_bytes, P(work), need.value - work_short, P(status),
                                             C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
        torch.cuda.synchronize()
        return rc, ids, int(status.item())
    dev = [torch.from_numpy(np.ascontiguousarray(a).copy()).to(DEV) for a in table]
    n = len(table[2])
    assert call(dev, n)[0] == 0
    for bad in ([None, dev[1], dev[2]], [dev[0], None, dev[2]], [dev[0], dev[1], None]):          # null arguments
        rc, ids, status = call(bad, n)
        assert rc != 0 and bool((ids == -7).all()) and status == -1
    for kw in (dict(n=MAX_ADDED_TOKENS + 1), dict(n=-1), dict(n=n, n_bytes=2 * n - 1), dict(n=n, n_bytes=MAX_ADDED_TOKEN_BYTES * n + 1), dict(n=n, work_short=16)):
        rc, ids, status = call(dev, **kw)
        assert rc != 0 and bool((ids == -7).all()) and status == -1, kw
    # a table that is not sorted, or holds a one-byte token: the status bit, every write inside the outputs
    raw, offsets, tids = table
    order = np.arange(n)[::-1]
    keys = [bytes(raw[offsets[k]:offsets[k + 1]]) for k in order]
    rev = (np.frombuffer(b"".join(keys), dtype=np.uint8), np.concatenate([[0], np.cumsum([len(k) for k in keys])]).astype(np.int32), tids[order].copy())
    rc, got = _abi_call(enc, texts, 8, rev)
    assert rc == 0 and got["status"] & ENCODE_BAD_TABLE and got["guards"]
    short = (np.frombuffer(b"<<x>", dtype=np.uint8), np.array([0, 1, 4], dtype=np.int32), np.array([5, 6], dtype=np.int32))
    rc, got = _abi_call(enc, texts, 8, short)
    assert rc == 0 and got["status"] & ENCODE_BAD_TABLE and got["guards"]
    # and on the host: one entry over the cap
    v = _vocab(UNLESS)
    with pytest.raises(NotImplementedError):
        DeviceTextEncoder.from_tokenizer_json(ar.with_added_tokens(fx["tokenizer"], _tokens(UNLESS, "cap") + [("<|over|>", v + MAX_ADDED_TOKENS)]), fx["pad_token_id"],
                                              fx["special_tokens"], fx["special_ids"], device=DEV, split_added_tokens=True)


def test_training_encode_texts_passes_the_switch():
    enc, tk, fx = _made(UNLESS)
    got = training.encode_texts(enc, ["a</s>b"], 8)
    ids, mask = ar.encode_with(enc.spec, fx["segment"], ["a</s>b"], 8)
    _same(got, ids, mask)
    import inspect
    assert "split_added_tokens" in inspect.signature(training.encode_texts).parameters
    assert _lib.ENCODE_BAD_TABLE == 4
