"""The device path of the lexical transfer (zett_amd/lexical.py -> zett_lexical_*) against what the reference script produced
(tests/golden/lexical_*) and against the CPU restatement (tests/lexical_ref.py).

Rows with n <= 16 constituents are bit-identical to the reference; rows with n > 16 are bit-identical to the restatement (the
product adds in ids order, torch's CPU mean cascades beyond 16) and inside the derived reordering bound of the reference
(tests/lexical_cases.py assert_rows_match)."""
import random

import numpy as np
import pytest
import torch

from tests import lexical_cases as lc
from tests import lexical_ref, retok_random

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _transfer(case):
    from zett_amd.lexical import LexicalTransfer
    from zett_amd.surface_forms import HnTokenizerSpec
    spec = HnTokenizerSpec.from_model_json(case["model"], (), (), -1)
    return LexicalTransfer(spec, DEV, vocab=case["vocab"], unk_token_id=case["unk_token_id"])


def _id_lists(plan):
    ids, count = plan.ids.cpu().numpy(), plan.count.cpu().numpy()
    return [ids[r, :count[r]].tolist() for r in range(len(count))]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def cases():
    return {name: lc.load(name) for name in lc.CASES}


@pytest.mark.parametrize("mode", lc.MODES)
@pytest.mark.parametrize("name", lc.CASES)
def test_goldens(cases, name, mode):
    """All three modes, tied (unigram) and untied (bpe): every row against the reference script's output, the overlap count
    against the line it printed, the plan against the restatement's."""
    case = cases[name]
    lt = _transfer(case)
    plan = lt.plan(case["tokens"], case["n_source_rows"], mode)
    assert plan.overlap == case["overlap"][mode]
    want_lists = lexical_ref.plan(lexical_ref.bare_model(case["model"]), case["vocab"], case["tokens"], case["n_source_rows"], mode)
    assert _id_lists(plan) == want_lists
    assert plan.n_ids == sum(map(len, want_lists))
    src_in = torch.from_numpy(case["source_in"]).to(DEV)
    src_out = None if case["source_out"] is None else torch.from_numpy(case["source_out"]).to(DEV)
    out_in = torch.full((len(case["tokens"]), src_in.shape[1]), float("nan"), device=DEV)
    out_out = None if src_out is None else torch.full_like(out_in, float("nan"))
    lt.rows_into(plan, src_in, src_out, "unk", dest_in=out_in, dest_out=out_out)
    torch.cuda.synchronize()
    e_in, e_out = lc.expected(name, mode)
    E = src_in.shape[1]
    lc.assert_rows_match(out_in.cpu().numpy(), e_in, want_lists, case["S"][:, :E], f"{name} {mode} in")
    if e_out is not None:
        lc.assert_rows_match(out_out.cpu().numpy(), e_out, want_lists, case["S"][:, E:], f"{name} {mode} out")
    lt.close()


def test_one_call_interface(cases):
    from zett_amd.lexical import lexical_embeddings
    from zett_amd.surface_forms import HnTokenizerSpec
    case = cases["bpe"]
    src_in, src_out = torch.from_numpy(case["source_in"]).to(DEV), torch.from_numpy(case["source_out"]).to(DEV)
    out_in, out_out, overlap = lexical_embeddings(HnTokenizerSpec.from_model_json(case["model"], (), (), -1), case["tokens"], src_in, src_out, "bfvt",
                                                  vocab=case["vocab"], unk_token_id=case["unk_token_id"])
    assert overlap == case["overlap"]["bfvt"] and out_in.dtype == torch.float32 and out_out.dtype == torch.float32
    e_in, e_out = lc.expected("bpe", "bfvt")
    assert np.array_equal(_bits(out_in.cpu().numpy()), _bits(e_in)) and np.array_equal(_bits(out_out.cpu().numpy()), _bits(e_out))


def test_random_fallback_golden(cases):
    """fallback_mode="random" with numpy's global generator seeded as the reference run was: the same draws land in the same rows."""
    case = cases["unigram"]
    lt = _transfer(case)
    plan = lt.plan(case["tokens"], case["n_source_rows"], "fvt")
    assert plan.overlap == case["overlap"]["fvt_random"] < plan.n_tokens
    src_in = torch.from_numpy(case["source_in"]).to(DEV)
    out = torch.full((plan.n_tokens, 32), float("nan"), device=DEV)
    np.random.seed(case["random_seed"])
    lt.rows_into(plan, src_in, None, "random", dest_in=out)
    torch.cuda.synchronize()
    lc.assert_rows_match(out.cpu().numpy(), lc.expected("unigram", "fvt_random")[0], _id_lists(plan), case["S"], "unigram fvt random")
    lt.close()


@pytest.mark.parametrize("kind", ["bpe", "unigram", "wordpiece"])
@pytest.mark.parametrize("mode", lc.MODES)
def test_plan_on_random_models(kind, mode):
    """ids / counts against the restatement on random BPE, Unigram and WordPiece models, R below and above the vocabulary."""
    from zett_amd.lexical import LexicalTransfer
    from zett_amd.surface_forms import HnTokenizerSpec
    make = {"bpe": retok_random.random_bpe, "unigram": retok_random.random_unigram, "wordpiece": retok_random.random_wordpiece}[kind]
    checked = 0
    for seed in range(12):
        rng = random.Random(1000 * seed + len(kind))
        model = make(rng)
        entries = model["vocab"]
        vocab = dict(entries) if isinstance(entries, dict) else {p: i for i, (p, _) in enumerate(entries)}
        vocab["<extra>"] = len(vocab)                      # an added token: part of get_vocab(), not of the model
        tokens = retok_random.random_tokens(rng, n=150) + list(vocab)[:20] + [""]
        tokens = [t for t in tokens if all(ch in retok_random.BYTES_TO_CHARS for ch in t)]
        ref_model = lexical_ref.bare_model(model)
        for R in (max(2, len(vocab) // 2), len(vocab) + 5):
            try:
                want = lexical_ref.plan(ref_model, vocab, tokens, R, mode)
            except Exception:
                continue                                       # (a model without unk that meets an unknown byte: tokenizers raises)
            lt = LexicalTransfer(HnTokenizerSpec.from_model_json(model, (), (), -1), DEV, vocab=vocab, unk_token_id=None)
            plan = lt.plan(tokens, R, mode, width=4)
            assert _id_lists(plan) == want, (kind, seed, R, mode)
            assert plan.overlap == sum(1 for w in want if w)
            lt.close()
            checked += 1
    assert checked >= 6


def _long_case(cases):
    """The bpe fixture with tokens whose decomposition is longer than 16 ids, and longer than the first plan's width."""
    case = cases["bpe"]
    tokens = list(case["tokens"][:200]) + ["ĠhelloĠworld" * 6, "".join(case["tokens"][300:340]), "a1b2c3d4" * 9, ""]
    return case, tokens


def test_replan_of_wide_rows_equals_the_wide_plan(cases):
    case, tokens = _long_case(cases)
    lt = _transfer(case)
    R = case["n_source_rows"]
    want = lexical_ref.plan(lexical_ref.bare_model(case["model"]), case["vocab"], tokens, R, "fvt")
    longest = max(map(len, want))
    assert longest > 16
    narrow = lt.plan(tokens, R, "fvt", width=3)
    wide = lt.plan(tokens, R, "fvt", width=longest)
    assert narrow.n_replanned > 0 and wide.n_replanned == 0 and narrow.width == longest
    assert _id_lists(narrow) == _id_lists(wide) == want
    assert torch.equal(narrow.count, wide.count)
    # rows with n > 16: bit-identical to the restatement (the in-order sum)
    src_in, src_out = torch.from_numpy(case["source_in"]).to(DEV), torch.from_numpy(case["source_out"]).to(DEV)
    out_in = torch.empty((len(tokens), 32), device=DEV)
    out_out = torch.empty_like(out_in)
    lt.rows_into(narrow, src_in, src_out, dest_in=out_in, dest_out=out_out)
    ref, _ = lexical_ref.rows(case["S"], want, case["unk_token_id"])
    got = np.concatenate([out_in.cpu().numpy(), out_out.cpu().numpy()], axis=1)
    assert np.array_equal(_bits(got), _bits(ref))
    # ... and inside the reordering bound of torch's cascaded mean, the reference's arithmetic
    S = torch.from_numpy(case["S"])
    torch_rows = np.stack([S[ids].mean(0).numpy() if ids else case["S"][case["unk_token_id"]] for ids in want])
    lc.assert_rows_match(got, torch_rows, want, case["S"], "long tokens vs torch mean")
    lt.close()


def test_source_rows_below_and_above_the_tokenizer_and_a_special_token_beyond(cases):
    """R smaller than the tokenizer: a special token whose id is >= R is NOT matched by string but tokenized like any text."""
    case = cases["unigram"]
    specials = [s for s in case["special_tokens"] if s in case["vocab"]]
    assert specials
    tokens = specials + list(case["tokens"][:300])
    lt = _transfer(case)
    ref_model = lexical_ref.bare_model(case["model"])
    for R in (min(case["vocab"][s] for s in specials), case["n_source_rows"], case["tokenizer_length"] + 7):
        R = max(R, 1)
        for mode in ("fvt", "bfvt"):
            want = lexical_ref.plan(ref_model, case["vocab"], tokens, R, mode)
            assert _id_lists(lt.plan(tokens, R, mode)) == want, (R, mode)
    R = max(1, min(case["vocab"][s] for s in specials))
    beyond = [s for s in specials if case["vocab"][s] >= R]
    assert beyond
    plan = lt.plan(beyond, R, "bfvt")
    want = lexical_ref.plan(ref_model, case["vocab"], beyond, R, "bfvt")
    assert _id_lists(plan) == want and all(w != [case["vocab"][s]] for w, s in zip(want, beyond))
    lt.close()


def test_empty_token_is_a_fallback_row(cases):
    case = cases["bpe"]
    lt = _transfer(case)
    plan = lt.plan(["", "Ġthe", ""], case["n_source_rows"], "bfvt")
    assert plan.count.cpu().tolist()[0] == 0 and plan.count.cpu().tolist()[2] == 0 and plan.overlap == 1
    only = lt.plan([""], case["n_source_rows"], "fvt")
    assert only.count.cpu().tolist() == [0] and only.overlap == 0
    lt.close()


@pytest.mark.parametrize("src_dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("dst_dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_dtypes(cases, src_dtype, dst_dtype):
    """16-bit sources are upcast on load; a 16-bit destination holds fp32_result.to(dtype)."""
    case = cases["bpe"]
    lt = _transfer(case)
    plan = lt.plan(case["tokens"], case["n_source_rows"], "fvt")
    src_in = torch.from_numpy(case["source_in"]).to(DEV).to(src_dtype)
    src_out = torch.from_numpy(case["source_out"]).to(DEV).to(src_dtype)
    ref32_in = torch.empty((plan.n_tokens, 32), device=DEV)
    ref32_out = torch.empty_like(ref32_in)
    lt.rows_into(plan, src_in.float(), src_out.float(), dest_in=ref32_in, dest_out=ref32_out)
    out_in = torch.empty((plan.n_tokens, 32), device=DEV, dtype=dst_dtype)
    out_out = torch.empty_like(out_in)
    lt.rows_into(plan, src_in, src_out, dest_in=out_in, dest_out=out_out)
    torch.cuda.synchronize()
    assert torch.equal(out_in, ref32_in.to(dst_dtype)) and torch.equal(out_out, ref32_out.to(dst_dtype))
    if src_dtype == torch.float32:
        want, _ = lexical_ref.rows(case["S"], _id_lists(plan), case["unk_token_id"])
        assert np.array_equal(_bits(ref32_in.cpu().numpy()), _bits(want[:, :32]))
    lt.close()


def test_row_map_skips_and_strided_unaligned_destination(cases):
    """rows < 0 are left untouched; a destination with a leading dimension larger than E at an odd element offset, and widths
    that are not a multiple of a lane's columns, take the element path and give the same values — fp32 and 16-bit sources."""
    case = cases["unigram"]
    lt = _transfer(case)
    n = 500
    tokens = case["tokens"][:n]
    plan = lt.plan(tokens, case["n_source_rows"], "bfvt")
    lists = _id_lists(plan)
    combos = [(32, torch.float32, torch.float32), (30, torch.float32, torch.bfloat16), (29, torch.bfloat16, torch.float32),
              (24, torch.bfloat16, torch.bfloat16), (29, torch.float16, torch.float16), (32, torch.float16, torch.float32)]
    for E, src_dtype, dtype in combos:
        src = torch.from_numpy(np.ascontiguousarray(case["source_in"][:, :E])).to(DEV).to(src_dtype)
        want, _ = lexical_ref.rows(src.float().cpu().numpy(), lists, case["unk_token_id"])
        g = torch.Generator().manual_seed(E)
        perm = torch.randperm(n + 40, generator=g)[:n].to(torch.int64)
        perm[::7] = -1
        backing = torch.full((n + 40, 45), -7.0, device=DEV, dtype=dtype)
        flat = backing.view(-1)[3:3 + (n + 39) * 45 + E]
        dest = flat.as_strided((n + 40, E), (45, 1))          # odd element offset, ld 45
        lt.rows_into(plan, src, None, dest_in=dest, rows=perm.to(DEV))
        torch.cuda.synchronize()
        expect = torch.full((n + 40, 45), -7.0, dtype=dtype)
        e_view = expect.view(-1)[3:3 + (n + 39) * 45 + E].as_strided((n + 40, E), (45, 1))
        keep = perm >= 0
        e_view[perm[keep]] = torch.from_numpy(want)[keep].to(dtype)
        assert torch.equal(backing.cpu(), expect), (E, src_dtype, dtype)
        # the same rows through the vector path (aligned, contiguous) where the width allows it
        aligned = torch.full((n + 40, E), -7.0, device=DEV, dtype=dtype)
        lt.rows_into(plan, src, None, dest_in=aligned, rows=perm.to(DEV))
        torch.cuda.synchronize()
        assert torch.equal(aligned.cpu(), expect.view(-1)[3:3 + (n + 39) * 45 + E].as_strided((n + 40, E), (45, 1))), (E, src_dtype, dtype, "aligned")
    lt.close()


def test_bad_indices_are_reported_and_nothing_is_written(cases):
    from zett_amd.lexical import LexicalPlan
    case = cases["bpe"]
    lt = _transfer(case)
    R = case["n_source_rows"]
    src_in, src_out = torch.from_numpy(case["source_in"]).to(DEV), torch.from_numpy(case["source_out"]).to(DEV)
    ids = torch.tensor([[0, 1], [2, R], [3, 4]], dtype=torch.int32, device=DEV)
    count = torch.tensor([2, 2, 1], dtype=torch.int32, device=DEV)
    bad_plan = LexicalPlan(ids, count, 3, 5, R, "fvt")
    out_in = torch.full((3, 32), 5.0, device=DEV)
    out_out = torch.full((3, 32), 5.0, device=DEV)
    with pytest.raises(IndexError):
        lt.rows_into(bad_plan, src_in, src_out, dest_in=out_in, dest_out=out_out)
    ok_plan = LexicalPlan(torch.tensor([[0, 1], [2, R - 1], [3, 4]], dtype=torch.int32, device=DEV), count, 3, 5, R, "fvt")
    with pytest.raises(IndexError):
        lt.rows_into(ok_plan, src_in, src_out, dest_in=out_in, dest_out=out_out, rows=torch.tensor([0, 3, 1], device=DEV))
    with pytest.raises(IndexError):
        lt.rows_into(ok_plan, src_in, src_out, dest_in=out_in, dest_out=out_out, unk_token_id=R)
    with pytest.raises(ValueError):          # a count beyond the width: a row that was not planned again
        lt.rows_into(LexicalPlan(ok_plan.ids, torch.tensor([2, 3, 1], dtype=torch.int32, device=DEV), 3, 6, R, "fvt"), src_in, src_out,
                     dest_in=out_in, dest_out=out_out)
    torch.cuda.synchronize()
    assert bool((out_in == 5.0).all()) and bool((out_out == 5.0).all())
    lt.rows_into(ok_plan, src_in, src_out, dest_in=out_in, dest_out=out_out)          # the handle still works
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out_in[2].cpu().numpy()), _bits(case["source_in"][3]))
    lt.close()


def test_character_outside_the_byte_table_is_a_key_error(cases):
    case = cases["bpe"]
    lt = _transfer(case)
    with pytest.raises(KeyError, match="token 2"):
        lt.plan(["Ġthe", "abc", "sp ace", "x"], case["n_source_rows"], "fvt")
    assert lt.plan(["Ġthe"], case["n_source_rows"], "fvt").overlap == 1          # the handle still works
    lt.close()


def test_unk_fallback_needs_an_unk_id(cases):
    from zett_amd.lexical import LexicalTransfer
    from zett_amd.surface_forms import HnTokenizerSpec
    case = cases["bpe"]
    lt = LexicalTransfer(HnTokenizerSpec.from_model_json(case["model"], (), (), -1), DEV, vocab=case["vocab"], unk_token_id=None)
    plan = lt.plan(["Ġthe"], case["n_source_rows"], "no")
    src = torch.from_numpy(case["source_in"]).to(DEV)
    with pytest.raises(ValueError, match="unk_token_id"):
        lt.rows_into(plan, src, dest_in=torch.empty((1, 32), device=DEV))
    lt.close()
