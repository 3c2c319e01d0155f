"""DeviceSampledVocabulary (csrc/sampled_vocab.hip through the C ABI) against the host-built path: ``build_sampled_tokenizer`` ->
``HnTokenizerSpec`` / ``DeviceTextEncoder.from_tokenizer`` / the library's own tokenizer call, and against the reference's recorded
surface forms.  Every comparison is integer or bit equality."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sampler_ref as R
from tests.sampled_vocab_cases import CASES, hand_made, stand_in_reference, texts_for
from zett_amd import _lib
from zett_amd import sampled_vocab as sv
from zett_amd.surface_forms import DeviceRetokenizer, HnTokenizerSpec
from zett_amd.text_encode import DeviceTextEncoder
from zett_amd.tokenizer_sampling import DeviceTokenizerSampler, SampledPieces, build_sampled_tokenizer, sample_tokenizer

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MAX_VOCAB = 2048
_VOCABULARIES = {}


def _vocabulary(name):
    v = _VOCABULARIES.get(name)
    if v is None:
        v = _VOCABULARIES[name] = sv.DeviceSampledVocabulary(stand_in_reference(CASES[name]["specials"]), True, max_vocab=MAX_VOCAB, device=DEV)
    return v


def _upload(pieces_and_scores, capacity=None, n=None):
    """A list as the sampler would leave it on the device."""
    raws = [R.from_byte_level(p) for p, _ in pieces_and_scores]
    assert all(1 <= len(r) <= 16 for r in raws)
    cap = len(raws) if capacity is None else capacity
    pieces = np.zeros((cap, 16), dtype=np.uint8)
    lengths = np.zeros(cap, dtype=np.uint8)
    scores = np.zeros(cap, dtype=np.float64)
    for i, raw in enumerate(raws):
        pieces[i, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
        lengths[i] = len(raw)
        scores[i] = pieces_and_scores[i][1]
    up = lambda a: torch.from_numpy(a).to(DEV)          # noqa: E731
    return SampledPieces(up(pieces), up(lengths), up(scores), torch.tensor([len(raws) if n is None else n], dtype=torch.int32, device=DEV),
                         torch.zeros(1, dtype=torch.int32, device=DEV))


def _host_model(tokenizer):
    """(set of (bytes, id, score bits), single_id) of the model the host-built path puts on the device"""
    spec = HnTokenizerSpec.from_tokenizer(tokenizer)
    o = spec.piece_offsets
    keys = [bytes(spec.piece_bytes[o[i]:o[i + 1]]) for i in range(len(spec.piece_ids))]
    entries = {(k, int(i), np.float64(s).tobytes()) for k, i, s in zip(keys, spec.piece_ids, spec.piece_scores)}
    assert len(entries) == len(keys)
    single = np.full(256, -1, dtype=np.int32)
    for k, i in zip(keys, spec.piece_ids):
        if len(k) == 1:
            single[k[0]] = i
    return entries, single


def _device_model(vocabulary):
    keys, ids, scores, single = vocabulary.piece_table()
    entries = {(k, int(i), np.float64(s).tobytes()) for k, i, s in zip(keys, ids, scores)}
    assert len(entries) == len(keys), "an entry sits in two slots"
    return entries, single


def _library_rows(tokenizer, texts, t, special_ids_map):
    want = tokenizer(texts, max_length=t, truncation=True, padding="max_length", return_tensors="np", add_special_tokens=True)
    ids = want["input_ids"].copy()
    for k, v in special_ids_map.items():          # zett/collator.py:177-178
        ids[ids == k] = v
    return ids, want["attention_mask"]


def _usable(texts, tokenizer):
    """the texts without the special tokens' strings (the library would split them out; the encoder refuses such a text)"""
    for s in tokenizer.all_special_tokens:
        texts = [x.replace(s, "") for x in texts]
    return texts


def _check_against_host(vocabulary, built, pieces_and_scores, reference):
    """The table as a set of (bytes, id, score bits) and single_id against the host-built tokenizer's model; priors, byte lengths, map,
    n_vocab, min_score and pad id against the host half; the unknown score's base against the model's."""
    tokenizer, special_ids_map, scores = build_sampled_tokenizer(pieces_and_scores, reference, True)
    want_entries, want_single = _host_model(tokenizer)
    got_entries, got_single = _device_model(vocabulary)
    assert got_entries == want_entries
    assert np.array_equal(got_single, want_single)
    assert np.float64(built.table_min_score).tobytes() == np.float64(HnTokenizerSpec.from_tokenizer(tokenizer).unigram_min_score).tobytes()
    assert built.n_vocab == len(tokenizer) == len(scores) and built.status == 0
    assert torch.equal(built.priors.view(torch.int64).cpu(), torch.from_numpy(np.asarray(scores, dtype=np.float64)).view(torch.int64))
    tokens = tokenizer.convert_ids_to_tokens(range(len(tokenizer)))
    assert built.byte_lengths.dtype == torch.int64 and built.byte_lengths.cpu().tolist() == [len(x) for x in tokens]
    assert list(built.special_ids_map.items()) == list(special_ids_map.items())
    assert np.float64(built.min_score).tobytes() == np.float64(scores.min()).tobytes()
    assert built.encoder.spec.pad_id == tokenizer.pad_token_id
    return tokenizer, special_ids_map


@pytest.mark.parametrize("extra", (1, 9, 600))
@pytest.mark.parametrize("name", sorted(CASES))
def test_vocabulary(name, extra):
    pieces = hand_made(extra)
    vocabulary = _vocabulary(name)
    built = vocabulary.build(_upload(pieces), len(pieces))
    _check_against_host(vocabulary, built, pieces, stand_in_reference(CASES[name]["specials"]))
    assert built.n_removed == CASES[name]["removed"] and bool(built.special_ids_map) == CASES[name]["map"]
    if name == "special_is_a_table_piece" and extra == 1:          # the one table piece is the removed special: m = 391
        assert built.n_vocab == 391 + 4 and built.n_removed == 1


@pytest.mark.parametrize("extra", (1, 9, 600))
@pytest.mark.parametrize("name", sorted(CASES))
def test_table_equals_the_host_built_tokenizer_s(name, extra):
    """The read-out as a set of (bytes, id, score bits) against ``HnTokenizerSpec.from_tokenizer(host-built tokenizer)``.  With the
    installed transformers 5 that model holds the scores as the library's JSON round trip leaves them (35 of 995 entries of the
    600-piece lists one ulp from the sampler's): the table holds the same values, priors the sampler's."""
    pieces = hand_made(extra)
    vocabulary = _vocabulary(name)
    vocabulary.build(_upload(pieces), len(pieces))
    tokenizer = build_sampled_tokenizer(pieces, stand_in_reference(CASES[name]["specials"]), True)[0]
    want_entries, want_single = _host_model(tokenizer)
    got_entries, got_single = _device_model(vocabulary)
    print("entries:", len(want_entries), "only on the device:", len(got_entries - want_entries), "only on the host:", len(want_entries - got_entries))
    assert np.array_equal(got_single, want_single)
    assert got_entries == want_entries
    scores = {i: s for _, i, s in got_entries}
    differ = sum(scores[i] != np.float64(x).tobytes() for i, x in enumerate(vocabulary.build(_upload(pieces), len(pieces)).priors.cpu().tolist()) if i in scores)
    assert vocabulary.scores_through_json == (differ > 0) or extra < 600          # (the 600-piece lists hold scores the round trip moves)


@pytest.mark.parametrize("name", sorted(CASES))
def test_encode(name):
    pieces = hand_made(600)
    vocabulary = _vocabulary(name)
    built = vocabulary.build(_upload(pieces), len(pieces))
    tokenizer, special_ids_map = _check_against_host(vocabulary, built, pieces, stand_in_reference(CASES[name]["specials"]))
    texts = _usable(texts_for(600, n=300), tokenizer)
    assert len(texts) == 300 and sum(map(len, texts)) > 5000
    host = DeviceTextEncoder.from_tokenizer(tokenizer, device=DEV)
    for t in (8, 32):
        ids, mask = _library_rows(tokenizer, texts, t, special_ids_map)
        for dtype in (torch.int32, torch.int64):
            got = built.encoder(texts, t, special_ids_map, dtype=dtype)
            want = host(texts, t, special_ids_map, dtype=dtype)
            assert got["input_ids"].dtype == dtype
            assert torch.equal(got["input_ids"], want["input_ids"]) and torch.equal(got["attention_mask"], want["attention_mask"])
            assert np.array_equal(got["input_ids"].cpu().numpy(), ids) and np.array_equal(got["attention_mask"].cpu().numpy(), mask)
    host.close()


# ---- surface forms: the reference's own output -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.FIXTURES)
def test_surface_forms_equal_the_reference(name):
    """Every special token of the fixtures' reference is a special token of their hn tokenizer: four patched rows."""
    fx = R.load_fixture(name)
    pieces = sv.prepend_unknown_chars([(p, s) for p, s in fx["prepared"]])          # (the fixtures' lists are not a sampler's: zett/collator.py:373-376 on the host)
    vocabulary = sv.DeviceSampledVocabulary(R.tokenizer_of(fx["reference"]), fx["add_prefix_space"], hn_tokenizer=R.tokenizer_of(fx["hn_tokenizer"]),
                                            hn_surface_maxlen=fx["hn_surface_maxlen"], max_vocab=MAX_VOCAB, device=DEV)
    assert all(i >= 0 for i in vocabulary.special_hn_ids)
    built = vocabulary.build(_upload(pieces), len(pieces))
    assert built.surface_forms.dtype == torch.int32 and np.array_equal(built.surface_forms.cpu().numpy(), np.array(fx["surface_forms"]))
    assert built.priors.cpu().tolist() == fx["scores"] and built.byte_lengths.cpu().tolist() == fx["byte_lengths"]
    assert [[k, v] for k, v in built.special_ids_map.items()] == fx["special_ids_map"] and built.n_vocab == len(fx["pieces"])
    assert built.encoder.spec.pad_id == fx["pad_token_id"]
    got = built.encoder(fx["texts"], 16, built.special_ids_map)
    tokenizer = build_sampled_tokenizer(pieces, R.tokenizer_of(fx["reference"]), fx["add_prefix_space"])[0]
    ids, mask = _library_rows(tokenizer, fx["texts"], 16, built.special_ids_map)
    assert np.array_equal(got["input_ids"].cpu().numpy(), ids) and np.array_equal(got["attention_mask"].cpu().numpy(), mask)
    vocabulary.close()


def test_surface_forms_with_a_special_the_hn_tokenizer_does_not_know():
    """<mask> goes through the hn model like a piece (its text is emitted); <s>, </s> and <pad> are patched rows.  Yardstick: the host half."""
    fx = R.load_fixture(R.FIXTURES[0])
    hn = R.tokenizer_of(fx["hn_tokenizer"])
    reference = stand_in_reference({"<s>": 0, "</s>": 2, "<pad>": 1, "<mask>": 397})
    pieces = hand_made(9)
    tokenizer, special_ids_map, want_sf, priors, byte_lengths = sample_tokenizer(["x"], R.StandInSampler(pieces), reference, n_total=400, noise_std=0.0,
                                                                                 add_prefix_space=True, hn_tokenizer=hn, hn_surface_maxlen=5)
    vocabulary = sv.DeviceSampledVocabulary(reference, True, hn_tokenizer=hn, hn_surface_maxlen=5, max_vocab=MAX_VOCAB, device=DEV)
    assert sorted(vocabulary.special_hn_ids) == sorted([-1] + [hn.convert_tokens_to_ids(x) for x in ("<s>", "</s>", "<pad>")])
    built = vocabulary.build(_upload(pieces), len(pieces))
    assert np.array_equal(built.surface_forms.cpu().numpy(), np.asarray(want_sf))
    assert built.priors.cpu().numpy().tobytes() == np.asarray(priors, dtype=np.float64).tobytes() and built.byte_lengths.cpu().tolist() == byte_lengths.tolist()
    assert built.special_ids_map == special_ids_map
    vocabulary.close()


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
def _e2e_texts():
    rng = np.random.default_rng(3)          # (the texts of tests/test_sampler_gpu.py::test_end_to_end_sample_then_encode)
    words = "the quick brown fox jumps over the lazy dog , it's 12 345 times . we'll see".split(" ")
    return [" ".join(words[i] for i in rng.integers(0, len(words), size=20)) for _ in range(8)]


def _sampler():
    return DeviceTokenizerSampler(table_capacity=1 << 14, max_depth=2, max_pieces=1 << 12)


def test_end_to_end_equals_the_host_path():
    texts, reference = _e2e_texts(), stand_in_reference(CASES["ids_0123"]["specials"])
    host_sampler, sampler = _sampler(), _sampler()
    tokenizer, special_ids_map, _, priors, byte_lengths = sample_tokenizer(texts, host_sampler, reference, n_total=1200, noise_std=0.0, add_prefix_space=True)
    vocabulary = _vocabulary("ids_0123")
    encoder, got_map, surface_forms, got_priors, got_lengths = sv.sample_tokenizer_device(texts, sampler, vocabulary, n_total=1200, noise_std=0.0)
    assert got_map == special_ids_map == {} and surface_forms is None
    assert got_priors.cpu().numpy().tobytes() == np.asarray(priors, dtype=np.float64).tobytes() and got_lengths.cpu().tolist() == byte_lengths.tolist()
    got = encoder(texts, 32, got_map)
    ids, mask = _library_rows(tokenizer, texts, 32, special_ids_map)
    assert np.array_equal(got["input_ids"].cpu().numpy(), ids) and np.array_equal(got["attention_mask"].cpu().numpy(), mask)
    assert sampler.depth == host_sampler.depth == 1
    host_sampler.close()
    sampler.close()


def test_rebuilding_one_handle_leaves_nothing_behind():
    """seed_size 392, 1 200, 392 into the same handle: after each build the table is the new model's and the rows are the library's; the
    same sample built twice gives the same bits in every output."""
    texts, reference = _e2e_texts(), stand_in_reference(CASES["one_beyond_the_end"]["specials"])
    vocabulary = _vocabulary("one_beyond_the_end")
    sampler = _sampler()
    sizes = []
    for seed_size in (392, 1200, 392):
        sampled = sampler.sample_tokenizer(texts, seed_size, 16, 4, 0.0, True, False)
        built = vocabulary.build(sampled, seed_size)
        tokenizer, special_ids_map = _check_against_host(vocabulary, built, sampled.to_list(), reference)
        assert special_ids_map and built.n_vocab == int(sampled.n.item()) + 4
        got = built.encoder(texts, 32, special_ids_map)
        ids, mask = _library_rows(tokenizer, texts, 32, special_ids_map)
        assert np.array_equal(got["input_ids"].cpu().numpy(), ids) and np.array_equal(got["attention_mask"].cpu().numpy(), mask)
        sizes.append(built.n_vocab)
    assert sizes[0] == sizes[2] == 396 and sizes[1] > 420
    entries = _device_model(vocabulary)
    again = vocabulary.build(sampled, 392)
    assert _device_model(vocabulary)[0] == entries[0] and np.array_equal(_device_model(vocabulary)[1], entries[1])
    assert torch.equal(again.priors.view(torch.int64), built.priors.view(torch.int64)) and torch.equal(again.byte_lengths, built.byte_lengths)
    assert again.special_ids_map == built.special_ids_map and (again.n_vocab, again.n_removed, again.status) == (built.n_vocab, built.n_removed, built.status)
    assert torch.equal(again.encoder(texts, 32, special_ids_map)["input_ids"], got["input_ids"])
    sampler.close()


# ---- edges -------------------------------------------------------------------------------------------------------------------------------
def test_status_bits():
    vocabulary = _vocabulary("ids_0123")
    pieces = hand_made(9)
    built = vocabulary.build(_upload(pieces, n=255), len(pieces), check=False)          # an n below 256, uploaded by hand
    assert built.status & sv.VOCAB_NOT_A_SAMPLE and built.n_vocab == 255 + 4
    with pytest.raises(NotImplementedError, match="alphabet"):
        vocabulary.build(_upload(pieces, n=255), len(pieces))
    twice = pieces[:395] + [pieces[393]] + pieces[395:]          # one piece written twice
    built = vocabulary.build(_upload(twice), len(twice), check=False)
    assert built.status == sv.VOCAB_DUPLICATE and built.n_vocab == len(twice) + 4
    with pytest.raises(ValueError, match="twice"):
        vocabulary.build(_upload(twice), len(twice))
    built = vocabulary.build(_upload(pieces, capacity=500, n=450), 420, check=False)          # more pieces than the bound the host gave
    assert built.status & sv.VOCAB_OUT_FULL and built.n_vocab == 420 + 4
    with pytest.raises(ValueError, match="max_vocab"):
        vocabulary.build(_upload(pieces), MAX_VOCAB)


def _raw_build(vocabulary, sampled, bound, v_cap, text_cap, guard=64, work_bytes=None, handle=None):
    """zett_sampled_vocab_build straight through the C ABI, every output with a guard region of 0xAB behind it"""
    s = vocabulary.n_special
    out = {"priors": torch.full((v_cap + guard,), 0xAB, dtype=torch.uint8, device=DEV).repeat_interleave(8).view(torch.float64),
           "byte_lengths": torch.full(((v_cap + guard) * 8,), 0xAB, dtype=torch.uint8, device=DEV).view(torch.int64),
           "text_offsets": torch.full(((v_cap + 1 + guard) * 4,), 0xAB, dtype=torch.uint8, device=DEV).view(torch.int32),
           "text": torch.full((text_cap + guard,), 0xAB, dtype=torch.uint8, device=DEV),
           "record": torch.full((32 + guard,), 0xAB, dtype=torch.uint8, device=DEV)}
    P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None          # noqa: E731
    work = vocabulary._work
    rc = vocabulary.lib.zett_sampled_vocab_build(handle or vocabulary.retok.handle, P(sampled.pieces), P(sampled.lengths), P(sampled.scores), P(sampled.n), sampled.pieces.shape[0],
                                                 bound, P(vocabulary._d_ids), P(vocabulary._d_raw_off), P(vocabulary._d_raw), P(vocabulary._d_chars), P(vocabulary._d_hn), s,
                                                 vocabulary._raw_bytes, vocabulary._max_raw, P(out["priors"]), P(out["byte_lengths"]), P(out["text_offsets"]), v_cap,
                                                 P(out["text"]), text_cap, P(out["record"]), _lib.VOCAB_SCORES_THROUGH_JSON if vocabulary.scores_through_json else 0, P(work), work.numel() if work_bytes is None else work_bytes,
                                                 C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    return rc, out


def _record(out):
    return _lib.ZettSampledVocabRecord.from_buffer_copy(out["record"][:32].cpu().numpy().tobytes())


def test_outputs_stay_inside_capacities_one_short():
    vocabulary = _vocabulary("ids_0123")
    pieces = hand_made(9)
    sampled = _upload(pieces)
    v = len(pieces) + 4
    rc, full = _raw_build(vocabulary, sampled, len(pieces), v, 40 * v)
    assert rc == 0
    rec = _record(full)
    assert rec.status == 0 and rec.n_vocab == v and 0 < rec.n_text < 40 * v
    offsets = full["text_offsets"][:v + 1].cpu().numpy()
    assert offsets[0] == 0 and offsets[-1] == rec.n_text and (np.diff(offsets) >= 0).all()
    text = bytes(full["text"][:rec.n_text].cpu().numpy())
    tokens = build_sampled_tokenizer(pieces, stand_in_reference(CASES["ids_0123"]["specials"]), True)[0].convert_ids_to_tokens(range(v))
    assert [text[offsets[i]:offsets[i + 1]].decode("utf-8") for i in range(v)] == tokens          # the byte-level text of every id
    for v_cap, text_cap in ((v - 1, 40 * v), (v, rec.n_text - 1), (v - 1, rec.n_text - 1)):
        rc, out = _raw_build(vocabulary, sampled, len(pieces), v_cap, text_cap)
        assert rc == 0
        short = _record(out)
        assert short.status == sv.VOCAB_OUT_FULL and short.n_vocab == v and short.n_text <= text_cap
        assert bool((out["priors"].view(torch.uint8)[8 * v_cap:] == 0xAB).all()) and bool((out["byte_lengths"].view(torch.uint8)[8 * v_cap:] == 0xAB).all())
        assert bool((out["text_offsets"].view(torch.uint8)[4 * (v_cap + 1):] == 0xAB).all()) and bool((out["text"][text_cap:] == 0xAB).all())
        assert bool((out["record"][32:] == 0xAB).all())
        assert torch.equal(out["priors"][:v_cap].view(torch.int64), full["priors"][:v_cap].view(torch.int64))
        got = out["text_offsets"][:v_cap + 1].cpu().numpy()
        assert (np.diff(got) >= 0).all() and got[-1] <= text_cap
    vocabulary.build(sampled, len(pieces))          # (the shared handle is left committed)


def test_an_uncommitted_handle_refuses_to_encode_and_bad_arguments_are_refused():
    vocabulary = _vocabulary("ids_0123")
    pieces = hand_made(9)
    sampled = _upload(pieces)
    v = len(pieces) + 4
    fresh = DeviceRetokenizer.unigram_on_device(DEV, MAX_VOCAB)
    encoder = DeviceTextEncoder.from_handle(fresh, vocabulary.encode_spec, vocabulary.table, vocabulary._d_table)
    with pytest.raises(RuntimeError, match="zett_sampled_vocab_commit"):
        encoder(["a b"], 8)                                             # created, never built
    rc, out = _raw_build(vocabulary, sampled, len(pieces), v, 40 * v, handle=fresh.handle)
    assert rc == 0
    with pytest.raises(RuntimeError, match="zett_sampled_vocab_commit"):
        encoder(["a b"], 8)                                             # built, not committed
    rec = _record(out)
    big = _lib.ZettSampledVocabRecord.from_buffer_copy(bytes(rec))
    big.n_vocab = v + 1
    assert vocabulary.lib.zett_sampled_vocab_commit(fresh.handle, C.byref(big)) == _lib.E_INVALID          # beyond the build's bound
    assert vocabulary.lib.zett_sampled_vocab_commit(fresh.handle, C.byref(rec)) == 0
    want = vocabulary.build(sampled, len(pieces)).encoder(["a b", "it's 12"], 8)
    got = encoder(["a b", "it's 12"], 8)
    assert torch.equal(got["input_ids"], want["input_ids"])
    # refused before any launch: a short workspace, null arguments, a handle of another kind, too large a seed_size
    assert _raw_build(vocabulary, sampled, len(pieces), v, 40 * v, work_bytes=64, handle=fresh.handle)[0] == _lib.E_INVALID
    assert _raw_build(vocabulary, sampled._replace(n=None), len(pieces), v, 40 * v, handle=fresh.handle)[0] == _lib.E_INVALID
    assert _raw_build(vocabulary, sampled, MAX_VOCAB, v, 40 * v, handle=fresh.handle)[0] == _lib.E_INVALID
    assert got["input_ids"].shape == (2, 8) and torch.equal(encoder(["a b", "it's 12"], 8)["input_ids"], want["input_ids"])          # (a refused call changes no state)
    host = DeviceTextEncoder.from_tokenizer(build_sampled_tokenizer(pieces, stand_in_reference(CASES["ids_0123"]["specials"]), True)[0], device=DEV)
    assert _raw_build(vocabulary, sampled, len(pieces), v, 40 * v, handle=host.retok.handle)[0] == _lib.E_INVALID
    host.close()
    fresh.close()
