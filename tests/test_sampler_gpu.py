"""DeviceTokenizerSampler (csrc/tokenizer_sample.hip through the C ABI) against tests/sampler_ref.py, the plain-Python definition."""
import math

import numpy as np
import pytest

from tests import sampler_ref as R

pytestmark = pytest.mark.gpu

ULP_BOUND = 4          # two correctly rounded logs of about 1 ulp each and one rounding of the quotient


def _sampler(**kw):
    from zett_amd.tokenizer_sampling import DeviceTokenizerSampler
    kw.setdefault("table_capacity", 1 << 12)
    kw.setdefault("max_depth", 4)
    kw.setdefault("max_pieces", 1 << 10)
    kw.setdefault("list_capacity", kw["table_capacity"] + 256)          # whatever the table holds fits the batch's list
    return DeviceTokenizerSampler(**kw)


def _table(sampler):
    keys, counts, z = sampler.merged_table()
    assert len(set(keys)) == len(keys), "a key sits in two slots"
    return {k: int(c) for k, c in zip(keys, counts)}, {k: float(x) for k, x in zip(keys, z)}


def _ulps(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return np.abs(got - want) / np.spacing(np.abs(want))


def _check_list(got, want):
    """pieces equal in order; scores within ULP_BOUND (exact where the definition gives a constant)"""
    assert [p for p, _ in got] == [R.byte_level(k) for k, _ in want]
    g, w = np.array([s for _, s in got]), np.array([s for _, s in want])
    const = (w == 0.0) | (w == R.FLOOR)
    assert np.array_equal(g[const], w[const])
    if (~const).any():
        worst = float(_ulps(g[~const], w[~const]).max())
        print("largest ulp distance of a score:", worst)
        assert worst <= ULP_BOUND


# ---- the merged table --------------------------------------------------------------------------------------------------------------------
WORDS = ["x" * 14, "y" * 15, "z" * 16]          # with the prefix space: words of 15, 16 and 17 bytes
TABLE_CASES = {
    "empty_text": ([""], 16, 1),
    "stride4": (["abcdefghij"], 16, 4),
    "duplicate_multibyte": (["é日x", "é日x"], 16, 1),
    "len15": ([WORDS[0]], 16, 1),
    "len16": ([WORDS[1]], 16, 1),
    "len17": ([WORDS[2]], 16, 1),
    "one_char": (["a"], 16, 1),
    "duplicates": (["ab ab", "cd", "ab ab", "it's  \n é 12"], 16, 1),
    "repeated_words": (["go go go go é é é go", "go go", "é é"] + ["the the 12 the 12"] * 1 + ["so " * 150], 16, 1),
    "maxlen2_stride1": (None, 2, 1),
    "maxlen2_stride4": (None, 2, 4),
    "maxlen16_stride1": (None, 16, 1),
    "maxlen16_stride4": (None, 16, 4),
}


def _small_texts():
    rng = np.random.default_rng(11)
    return [R.random_text(rng) for _ in range(12)]


@pytest.mark.parametrize("name", sorted(TABLE_CASES))
def test_table_equals_the_definition(name):
    texts, max_length, stride = TABLE_CASES[name]
    texts = _small_texts() if texts is None else texts
    ref = R.SamplerRef()
    ref.sample(texts, 1000, max_length, stride)
    s = _sampler()
    s.sample_tokenizer(texts, 1000, max_length, stride)
    got, _ = _table(s)
    assert got == ref.merged
    s.close()


def test_hand_computed_empty_text():
    s = _sampler()
    out = s.sample_tokenizer([""], 0, as_list=True)
    assert _table(s)[0] == {b" ": 4}          # the start list of a first pre-token holds 0 twice: 2 * len("Ġ".encode())
    assert len(out) == R.N_ALPHABET + 135 and all(score == 0.0 for _, score in out)          # no key of two bytes; min == sum: log(1) = 0
    s.close()


def test_probe_chains_wrap_round_the_end_of_the_table():
    texts = _small_texts()
    ref = R.SamplerRef()
    ref.sample(texts, 1000, 16, 1)
    s = _sampler(table_capacity=len(ref.merged) + 3)          # about 99 % full: chains run over the end
    s.sample_tokenizer(texts, 1000, 16, 1)
    assert _table(s)[0] == ref.merged
    s.close()


def test_a_table_too_small_sets_the_status_bit_and_stays_in_bounds():
    """Bounded probe loops: the call returns, the bit is set, and what is in the table is a part of the truth."""
    import torch
    from zett_amd import tokenizer_sampling as ts
    texts = _small_texts()
    ref = R.SamplerRef()
    ref.sample(texts, 1000, 16, 1)
    cap = len(ref.merged) // 3
    s = _sampler(table_capacity=cap)
    out = s.sample_tokenizer(texts, 1000, 16, 1, check=False)
    torch.cuda.synchronize()
    assert int(out.status.item()) & ts.SAMPLE_TABLE_FULL
    assert 0 <= int(out.n.item()) <= out.pieces.shape[0]
    got, _ = _table(s)
    assert len(got) <= cap and all(k in ref.merged and v <= ref.merged[k] for k, v in got.items())
    with pytest.raises(RuntimeError, match="table is full"):
        s.sample_tokenizer(texts, 1000, 16, 1)
    s.close()


# ---- 300 texts in three pushes, then two pops ----------------------------------------------------------------------------------------------
def _batches():
    rng = np.random.default_rng(5)
    texts = [R.random_prose(rng) if i % 2 else R.random_text(rng, 160) for i in range(340)]
    return [texts[0:100], texts[100:200], texts[200:300], texts[300:320], texts[320:340]]


SEED_SIZE = 391 + 25000          # the cut falls inside a class of equal p: with noise inside the keys with p <= 0


def _run_device(noise_std, seed):
    s = _sampler(table_capacity=1 << 19, max_depth=4, max_pieces=1 << 16)
    b = _batches()
    for texts in b[:3]:
        s.sample_tokenizer(texts, 30000, 16, 1, 0.0, False)
    first = s.sample_tokenizer(b[3], 2000, 16, 1, 0.0, True)
    last = s.sample_tokenizer(b[4], SEED_SIZE, 16, 1, noise_std, True, seed=seed)
    return s, first, last


def _run_ref(noise_std, z):
    ref = R.SamplerRef()
    b = _batches()
    for texts in b[:3]:
        assert ref.sample(texts, 30000, 16, 1, 0.0, False) == []
    first = ref.sample(b[3], 2000, 16, 1, 0.0, True)
    last = ref.sample(b[4], SEED_SIZE, 16, 1, noise_std, True, noise=(lambda k: z[k]) if z is not None else None)
    return ref, first, last


@pytest.fixture(scope="module")
def plain():
    s, first, last = _run_device(0.0, 0)
    table, _ = _table(s)
    out = {"table": table, "first": first.to_list(), "last": last.to_list(), "tensors": (first, last), "ref": _run_ref(0.0, None)}
    s.close()
    return out


@pytest.fixture(scope="module")
def noised():
    s, _, last = _run_device(0.05, 1234)
    table, z = _table(s)
    out = {"table": table, "z": z, "last": last.to_list()}
    s.close()
    return out


def test_sequence_table(plain):
    ref, _, _ = plain["ref"]
    assert plain["table"] == ref.merged
    assert len(ref.merged) >= 20000


def test_sequence_without_noise(plain):
    _, first, last = plain["ref"]
    assert len(plain["first"]) == 2000
    _check_list(plain["first"], first)
    _check_list(plain["last"], last)


def test_sequence_with_noise(noised):
    _, _, last = _run_ref(0.05, noised["z"])
    assert len(noised["last"]) == len(last)
    _check_list(noised["last"], last)
    floor = [p for p, s in noised["last"][391:] if s == R.FLOOR]
    assert len(floor) > 100, "the case must reach into the keys with p <= 0"
    keys = [R.from_byte_level(p) for p in floor]
    assert keys == sorted(keys, key=lambda k: (len(k), k))


def test_noise_is_a_function_of_seed_and_key(noised):
    s, _, _ = _run_device(0.05, 1234)
    _, again = _table(s)
    s.close()
    s, _, _ = _run_device(0.0, 99)          # the read-out gives z of the call's seed whatever noise_std was
    _, other = _table(s)
    s.close()
    z = noised["z"]
    assert again.keys() == z.keys() == other.keys()
    assert all(np.float64(again[k]).tobytes() == np.float64(z[k]).tobytes() for k in z)
    assert sum(other[k] != z[k] for k in z) > 0.99 * len(z)
    # the same key in another table (a single text) gets the same z
    one = _sampler()
    one.sample_tokenizer(["the"], 1000, seed=1234)
    _, z1 = _table(one)
    one.close()
    assert all(np.float64(z1[k]).tobytes() == np.float64(z[k]).tobytes() for k in z1 if k in z) and any(k in z for k in z1)


def test_noise_is_standard_normal(noised):
    z = np.array(list(noised["z"].values()))
    n = len(z)
    assert n >= 20000 and np.isfinite(z).all()
    print("n =", n, "mean z =", z.mean(), "var z =", z.var())
    assert abs(z.mean()) <= 5 / math.sqrt(n)
    assert abs(z.var() - 1) <= 5 * math.sqrt(2 / n)


def test_sequence_is_deterministic(plain):
    import torch
    s, first, last = _run_device(0.0, 0)
    for a, b in zip((first, last), plain["tensors"]):
        assert torch.equal(a.n, b.n) and torch.equal(a.pieces, b.pieces) and torch.equal(a.lengths, b.lengths) and torch.equal(a.scores, b.scores)
    s.close()


# ---- the queue and the edges of seed_size, as tests/test_sampler_host.py checks them on the definition -------------------------------------
@pytest.mark.parametrize("pop_prev", [False, True])
@pytest.mark.parametrize("push_current", [False, True])
def test_queue_behaviour(pop_prev, push_current):
    texts = [["a b"], ["c d"], ["e f"], ["g h"]]
    ref, s = R.SamplerRef(), _sampler()
    for t in texts[:2]:
        ref.sample(t, 0, pop_prev=False)
        s.sample_tokenizer(t, 0, pop_prev=False)
    for t in texts:
        want = ref.sample(t, 500, 16, 1, 0.0, pop_prev, push_current)
        got = s.sample_tokenizer(t, 500, 16, 1, 0.0, pop_prev, push_current, as_list=True)
        assert [p for p, _ in got] == [R.byte_level(k) for k, _ in want]
        assert s.depth == len(ref.queue)
        if pop_prev:
            assert _table(s)[0] == ref.merged
        if s.depth == s.max_depth and not pop_prev and push_current:
            break
    s.close()


@pytest.mark.parametrize("seed_size", [0, 391, 392, 393, 100000])
def test_seed_size_edges(seed_size):
    texts = ["hello world, it's me"]
    want = R.SamplerRef().sample(texts, seed_size)
    s = _sampler(max_pieces=1 << 17)
    got = s.sample_tokenizer(texts, seed_size, as_list=True)
    _check_list(got, want)
    assert len(got) == (392 if seed_size <= 392 else (393 if seed_size == 393 else len(want)))
    s.close()


def test_refusals_of_the_c_abi():
    import ctypes as C

    from zett_amd import _lib
    lib = _lib.load()
    h = C.c_void_p()
    for args in ((0, 0, 16, 16, 16), (0, 2, 0, 16, 16), (0, 2, 16, 0, 16), (0, 2, 1 << 20, 16, 16), (0, 2, 16, 16, 0)):
        assert lib.zett_sampler_create(*args, C.byref(h)) < 0 and not h.value
    s = _sampler(max_depth=1, max_pieces=4)
    with pytest.raises(ValueError):
        s.sample_tokenizer(["a"], 10000)          # more pieces than max_pieces
    with pytest.raises(ValueError):
        s.sample_tokenizer(["a"], 10, max_length=17)
    with pytest.raises(ValueError):
        s.sample_tokenizer(["a"], 10, stride=0)
    with pytest.raises(RuntimeError):
        s.merged_table()                           # no call with pop_prev yet
    s.sample_tokenizer(["a"], 10, pop_prev=False)
    with pytest.raises(RuntimeError):
        s.sample_tokenizer(["b"], 10, pop_prev=False)          # the queue is full
    n = C.c_int64(0)
    assert lib.zett_sampler_workspace_bytes(-1, 0, C.byref(n)) < 0
    s.close()


def test_outputs_stay_inside_a_small_capacity():
    """Straight through the C ABI: 300 rows for 391 fixed pieces and more.  The bit is set, n is the capacity, the rows behind are untouched."""
    import ctypes as C

    import torch

    from zett_amd import _lib
    s = _sampler()
    blob = "hello world".encode()
    dev = s.device
    text = torch.tensor(list(blob), dtype=torch.uint8, device=dev)
    off = torch.tensor([0, len(blob)], dtype=torch.int64, device=dev)
    cap, guard = 300, 8
    pieces = torch.full((cap + guard, 16), 0xAB, dtype=torch.uint8, device=dev)
    lengths = torch.full((cap + guard,), 0xAB, dtype=torch.uint8, device=dev)
    scores = torch.full((cap + guard,), 7.0, dtype=torch.float64, device=dev)
    n = torch.zeros(1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    need = C.c_int64(0)
    assert s.lib.zett_sampler_workspace_bytes(len(blob), 1, C.byref(need)) == 0
    work = torch.empty(need.value, dtype=torch.uint8, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    rc = s.lib.zett_sampler_sample(s.handle, P(text), P(off), 1, len(blob), P(s._d_table), len(s.table), 1000, 16, 1, 0.0, 0, 1, 1, P(pieces), P(lengths), P(scores), cap,
                                   P(n), P(work), work.numel(), P(status), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert int(status.item()) == _lib.SAMPLE_OUT_FULL and int(n.item()) == cap
    assert bool((pieces[cap:] == 0xAB).all()) and bool((lengths[cap:] == 0xAB).all()) and bool((scores[cap:] == 7.0).all())
    assert bool((lengths[:cap] >= 1).all())
    # too small a workspace, a null status: refused before any launch
    assert s.lib.zett_sampler_sample(s.handle, P(text), P(off), 1, len(blob), P(s._d_table), len(s.table), 1000, 16, 1, 0.0, 0, 1, 1, P(pieces), P(lengths), P(scores), cap,
                                     P(n), P(work), 16, P(status), None) < 0
    assert s.lib.zett_sampler_sample(s.handle, P(text), P(off), 1, len(blob), P(s._d_table), len(s.table), 1000, 16, 1, 0.0, 0, 1, 1, P(pieces), P(lengths), P(scores), cap,
                                     P(n), P(work), work.numel(), None, None) < 0
    s.close()


# ---- the host half's surface forms: the one element of the 5-tuple that needs the device -----------------------------------------------------
@pytest.mark.parametrize("name", R.FIXTURES)
def test_host_half_surface_forms_equal_the_reference(name):
    from zett_amd.tokenizer_sampling import sample_tokenizer
    fx = R.load_fixture(name)
    call = fx["sampler_call"]
    tokenizer, special_ids_map, surface_forms, priors, byte_lengths = sample_tokenizer(
        fx["texts"], R.StandInSampler(fx["prepared"]), R.tokenizer_of(fx["reference"]), n_total=call["n_total"], noise_std=call["noise_std"],
        add_prefix_space=fx["add_prefix_space"], hn_tokenizer=R.tokenizer_of(fx["hn_tokenizer"]), hn_surface_maxlen=fx["hn_surface_maxlen"])
    assert np.array_equal(np.asarray(surface_forms), np.array(fx["surface_forms"]))
    assert priors.tolist() == fx["scores"] and byte_lengths.tolist() == fx["byte_lengths"]
    assert [[k, v] for k, v in special_ids_map.items()] == fx["special_ids_map"]


# ---- end to end -------------------------------------------------------------------------------------------------------------------------------
def _reference_tokenizer():
    from tokenizers import Tokenizer, models, processors
    from transformers import PreTrainedTokenizerFast
    specials = {"<s>": 0, "<pad>": 1, "</s>": 2, "<unk>": 3}
    tk = Tokenizer(models.WordLevel(dict(specials), unk_token="<unk>"))
    tk.post_processor = processors.TemplateProcessing(single="<s> $A </s>", special_tokens=[("<s>", 0), ("</s>", 2)])
    return PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>", clean_up_tokenization_spaces=False)


def test_end_to_end_sample_then_encode():
    from zett_amd.training import DeviceTextEncoder, DeviceTokenizerSampler, sample_tokenizer
    rng = np.random.default_rng(3)
    words = "the quick brown fox jumps over the lazy dog , it's 12 345 times . we'll see".split(" ")
    texts = [" ".join(words[i] for i in rng.integers(0, len(words), size=20)) for _ in range(8)]
    sampler = DeviceTokenizerSampler(table_capacity=1 << 14, max_depth=2, max_pieces=1 << 12)
    tokenizer, special_ids_map, surface_forms, priors, byte_lengths = sample_tokenizer(texts, sampler, _reference_tokenizer(), n_total=1200, noise_std=0.0,
                                                                                       add_prefix_space=True)
    assert special_ids_map == {} and surface_forms is None and len(priors) == len(tokenizer) == len(byte_lengths)
    enc = DeviceTextEncoder.from_tokenizer(tokenizer)
    got = enc(texts, 32, special_ids_map)
    want = tokenizer(texts, max_length=32, truncation=True, padding="max_length", return_tensors="np", add_special_tokens=True)
    assert np.array_equal(got["input_ids"].cpu().numpy(), want["input_ids"])
    assert np.array_equal(got["attention_mask"].cpu().numpy(), want["attention_mask"])
    enc.close()
    sampler.close()


# ---- the word stage's workspace, framed ----------------------------------------------------------------------------------------------------------
def _texts_of_bytes(n_text):
    """three distinct ASCII texts of n_text bytes together"""
    src = "the quick brown fox it's 12 345 times, we'll see. " * (n_text // 50 + 1)
    a, b = n_text // 3, n_text // 2
    return [src[:a], src[a:a + b], src[a + b:n_text]]


@pytest.mark.parametrize("positions", (15, 16, 17, 1023, 1024, 1025, "empty"))
def test_c_abi_stays_inside_a_framed_workspace(positions):
    """Straight through the C ABI with a workspace of exactly zett_sampler_workspace_bytes between two 4096-byte guards: n_text + n_texts
    at the rounding edges of the workspace's arrays and of one scan segment.  The guards keep their fill, the status word is 0 and the
    outputs are the wrapper's (both calls pop and do not push, so the queue is the same for both: empty)."""
    import ctypes as C

    import torch
    s = _sampler()
    dev = s.device
    texts = [""] if positions == "empty" else _texts_of_bytes(positions - 3)
    assert len(set(texts)) == len(texts)
    blob = "".join(texts).encode()
    b, guard, seed_size, max_length, stride = len(texts), 4096, 1000, 16, 1
    assert positions == "empty" or len(blob) + b == positions
    want = s.sample_tokenizer(texts, seed_size, max_length, stride, push_current=False)
    cap = int(want.pieces.shape[0])
    off = torch.tensor(np.cumsum([0] + [len(x.encode()) for x in texts]), dtype=torch.int64, device=dev)
    text = torch.tensor(list(blob or b"\0"), dtype=torch.uint8, device=dev)
    need = C.c_int64(0)
    assert s.lib.zett_sampler_workspace_bytes(len(blob), b, C.byref(need)) == 0
    need = need.value
    frame = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device=dev)
    assert frame.data_ptr() % 16 == 0 and need % 16 == 0
    pieces = torch.zeros((cap, 16), dtype=torch.uint8, device=dev)
    lengths = torch.zeros(cap, dtype=torch.uint8, device=dev)
    scores = torch.zeros(cap, dtype=torch.float64, device=dev)
    n = torch.full((1,), -1, dtype=torch.int32, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    P = lambda t: C.c_void_p(t.data_ptr())          # noqa: E731
    rc = s.lib.zett_sampler_sample(s.handle, P(text), P(off), b, len(blob), P(s._d_table), len(s.table), seed_size, max_length, stride, 0.0, 0, 1, 0, P(pieces), P(lengths),
                                   P(scores), cap, P(n), C.c_void_p(frame.data_ptr() + guard), need, P(status), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    assert rc == 0, s.lib.zett_last_error()
    torch.cuda.synchronize()
    assert bool((frame[:guard] == 0xA5).all()) and bool((frame[guard + need:] == 0xA5).all())
    assert int(status.item()) == 0
    assert torch.equal(pieces, want.pieces) and torch.equal(lengths, want.lengths) and torch.equal(scores, want.scores) and torch.equal(n, want.n)
    assert int(n.item()) > 391 or positions == "empty"
    s.close()
