"""zett_amd.training.splice_special_rows / token_embeddings on the GPU (csrc/train_embed.hip), against torch / numpy on the CPU: the lookup
equal to indexing + ``.to(dtype)``, its backward bit-identical to the restatement of tests/embed_lookup_ref.py, the splice equal to
``index_copy``, and the whole input side inside a training step of the tiny hypernetwork."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.embed_lookup_ref import CASES, counts, embed_bwd_ref, recipe
from zett_amd import synth
from zett_amd.training import splice_special_rows, token_embeddings

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = (torch.float32, torch.float16, torch.bfloat16)
GRAD_LIMIT_F32 = 2e-4          # tests/test_lm_loss_gpu.py


def _bits(a):
    return a.detach().cpu().contiguous().view(torch.int32)


def _table(v, e, seed=7):
    return torch.randn(v, e, generator=torch.Generator().manual_seed(seed))


def _shape2(t):
    return next((b, t // b) for b in (30, 15, 1) if t % b == 0)          # [B, S] of a case


# ---- the lookup --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_lookup_equals_indexing_and_to_dtype(case):
    t, v, e = case
    ids = recipe(*case)[0]
    variants = (ids.to(DEV), ids.to(torch.int32).to(DEV), ids.view(_shape2(t)).to(DEV), ids.to(torch.int32).view(_shape2(t)).to(DEV))
    for in_dtype in DTYPES:
        table = _table(v, e).to(in_dtype)
        wide = torch.zeros(v, e + 8, dtype=in_dtype, device=DEV)
        wide[:, :e] = table.to(DEV)
        for tab in (table.to(DEV), wide[:, :e]):          # contiguous, and a view with row stride E + 8
            for out_dtype in DTYPES:
                want = table[ids].to(out_dtype)
                for x in variants:
                    got = token_embeddings(tab, x, dtype=out_dtype)
                    assert got.dtype == out_dtype and got.shape == tuple(x.shape) + (e,)
                    assert torch.equal(got.cpu().view(t, e), want), (case, in_dtype, out_dtype, x.dtype, tuple(x.shape))
        assert token_embeddings(table.to(DEV), variants[0]).dtype == in_dtype          # dtype=None: pred_in's


@pytest.mark.parametrize("case", [(257, 300, 29), (3000, 97, 64)])
def test_lookup_tail_path_at_an_odd_base_offset(case):
    t, v, e = case
    ids = recipe(*case)[0]
    for in_dtype in DTYPES:
        table = _table(v, e).to(in_dtype)
        flat = torch.zeros(v * e + 1, dtype=in_dtype, device=DEV)
        flat[1:] = table.to(DEV).view(-1)
        odd = flat[1:].view(v, e)          # one element off the allocation: no 16-byte access is possible
        for out_dtype in DTYPES:
            assert torch.equal(token_embeddings(odd, ids.to(DEV), dtype=out_dtype).cpu(), table[ids].to(out_dtype)), (case, in_dtype, out_dtype)


def test_lookup_four_wide_where_eight_do_not_divide():
    """E = 36 is a multiple of 4 and not of 8: between two 16-bit dtypes the lookup moves 4 elements per access, and the backward of a
    16-bit upstream 4 columns per lane, instead of dropping to one element (E = 29) — the same results."""
    case = (257, 300, 36)
    t, v, e = case
    ids, g = recipe(*case)
    for in_dtype in DTYPES:
        table = _table(v, e).to(in_dtype)
        for out_dtype in DTYPES:
            assert torch.equal(token_embeddings(table.to(DEV), ids.to(DEV), dtype=out_dtype).cpu(), table[ids].to(out_dtype)), (in_dtype, out_dtype)
    for dtype in DTYPES:
        up = g.to(dtype)
        want = torch.from_numpy(embed_bwd_ref(ids.numpy(), up.float().numpy(), v))
        assert torch.equal(_bits(_backward(ids.to(DEV), v, e, up.to(DEV))), _bits(want)), dtype


def _backward(ids_dev, v, e, upstream_dev, **kw):
    pred = torch.zeros(v, e, device=DEV, requires_grad=True)
    out = token_embeddings(pred, ids_dev, dtype=upstream_dev.dtype, **kw)
    out.backward(upstream_dev.view(out.shape))
    return pred.grad


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "f16", "bf16"))
def test_lookup_backward_is_the_restatement_bit_for_bit(case, dtype):
    t, v, e = case
    ids, g = recipe(*case)
    up = g.to(dtype)
    want = torch.from_numpy(embed_bwd_ref(ids.numpy(), up.float().numpy(), v))
    got = _backward(ids.to(DEV), v, e, up.to(DEV))
    assert got.dtype == torch.float32 and got.shape == (v, e)
    assert torch.equal(_bits(got), _bits(want)), (case, dtype, int((_bits(got) != _bits(want)).any(1).sum()))
    unused = torch.from_numpy(counts(*case) == 0)
    assert not _bits(got)[unused].any()          # exact (positive) zeros
    assert torch.equal(_bits(_backward(ids.to(DEV), v, e, up.to(DEV))), _bits(got))          # a second run
    assert torch.equal(_bits(_backward(ids.view(_shape2(t)).to(DEV), v, e, up.to(DEV))), _bits(got))          # the same ids as [B, S]
    assert torch.equal(_bits(_backward(ids.to(torch.int32).to(DEV), v, e, up.to(DEV))), _bits(got))


def test_lookup_backward_accumulates_like_autograd():
    case = (3000, 97, 64)
    t, v, e = case
    ids, g = recipe(*case)
    want = torch.from_numpy(embed_bwd_ref(ids.numpy(), g.numpy(), v))
    pred = _table(v, e).to(DEV).requires_grad_(True)
    out = token_embeddings(pred, ids.to(DEV))
    assert torch.equal(out.detach().cpu(), pred.detach().cpu()[ids])
    out.backward(g.to(DEV), retain_graph=True)
    assert torch.equal(_bits(pred.grad), _bits(want))
    out.backward(g.to(DEV))
    assert torch.equal(_bits(pred.grad), _bits(want + want))
    with pytest.raises(ValueError, match="fp32 pred_in"):
        token_embeddings(pred.detach().half().requires_grad_(True), ids.to(DEV))


@pytest.mark.parametrize("ids_dtype", (torch.int64, torch.int32))
def test_ids_outside_the_table(ids_dtype):
    """Planted on purpose; none of them is ever an address."""
    case = (3000, 97, 64)
    t, v, e = case
    ids, g = recipe(*case)
    ids = ids.clone()
    planted = {5: -1, 700: -100, 1500: v, 2999: v + 1000}
    if ids_dtype == torch.int64:
        planted[64] = 2 ** 31 + 5
        planted[65] = -(2 ** 31) - 7
    for p, x in planted.items():
        ids[p] = x
    bad = torch.zeros(t, dtype=torch.bool)
    bad[list(planted)] = True
    ids_dev = ids.to(ids_dtype).to(DEV)
    table = _table(v, e)
    for dtype in (torch.float32, torch.bfloat16):
        with pytest.raises(IndexError):
            token_embeddings(table.to(DEV), ids_dev, dtype=dtype)
        got = token_embeddings(table.to(DEV), ids_dev, dtype=dtype, check_ids=False).cpu()
        assert not _bits(got.float())[bad].any()
        assert torch.equal(got[~bad], table[ids[~bad]].to(dtype))
        want = torch.from_numpy(embed_bwd_ref(ids.numpy(), g.to(dtype).float().numpy(), v))          # (the restatement skips ids outside [0, V))
        assert torch.equal(_bits(_backward(ids_dev, v, e, g.to(dtype).to(DEV), check_ids=False)), _bits(want))
    with pytest.raises(IndexError):
        token_embeddings(table.to(DEV).requires_grad_(True), ids_dev)


# ---- the splice ----------------------------------------------------------------------------------------------------------------------
V, R = 50, 40
SPECIAL, IN_REFERENCE = [0, V - 1, 17, 5], [R - 1, 0, 3, 9]


def _splice_inputs(e, src_dtype, extra=3):
    """The source has 2E + extra columns.  extra = 3: an odd leading dimension, so the source rows take the element path at every E;
    extra = 0 (the shape production has) or 4: 16-byte reads of the source wherever E is a multiple of 4."""
    gen = torch.Generator().manual_seed(e)
    pred_in, pred_out = torch.randn(V, e, generator=gen), torch.randn(V, e, generator=gen)
    src = torch.randn(R, 2 * e + extra, generator=gen).to(src_dtype)
    idx, ref = torch.tensor(SPECIAL), torch.tensor(IN_REFERENCE)
    want_in = pred_in.clone().index_copy_(0, idx, src[ref, :e].float())
    want_out = pred_out.clone().index_copy_(0, idx, src[ref, e:2 * e].float())
    return pred_in, pred_out, src, want_in, want_out


@pytest.mark.parametrize("e", (29, 64, 200))
@pytest.mark.parametrize("src_dtype", DTYPES, ids=("f32", "f16", "bf16"))
@pytest.mark.parametrize("extra", (0, 4, 3), ids=("ld2E", "ld2E+4", "ld2E+3"))
def test_splice_equals_index_copy(e, src_dtype, extra):
    """Out of place and in place, every source dtype.  With a source of 2E or 2E + 4 columns, E = 64 and E = 200 read the source 16 bytes
    per lane (4 fp32, or 4 16-bit elements converted) and copy the other rows the same way; E = 29 and the odd 2E + 3 take the element path."""
    pred_in, pred_out, src, want_in, want_out = _splice_inputs(e, src_dtype, extra)
    a, b, s = pred_in.to(DEV), pred_out.to(DEV), src.to(DEV)
    for lists in ((SPECIAL, IN_REFERENCE), (np.array(SPECIAL), np.array(IN_REFERENCE, dtype=np.int32)), (torch.tensor(SPECIAL, device=DEV), torch.tensor(IN_REFERENCE))):
        got_in, got_out = splice_special_rows(a, b, s, *lists)
        assert torch.equal(_bits(got_in), _bits(want_in)) and torch.equal(_bits(got_out), _bits(want_out))
        assert got_in.data_ptr() != a.data_ptr() and torch.equal(a.cpu(), pred_in) and torch.equal(b.cpu(), pred_out)          # fresh matrices
    got_in, none = splice_special_rows(a, None, s[:, :e], SPECIAL, IN_REFERENCE)          # tied embeddings: E columns are enough
    assert none is None and torch.equal(_bits(got_in), _bits(want_in))
    with pytest.raises(ValueError, match="output half"):
        splice_special_rows(a, b, s[:, :e], SPECIAL, IN_REFERENCE)
    # in place: the same storage, no other element changes (a view with row stride E + 4 keeps its padding)
    wide = torch.full((V, e + 4), 7.0, device=DEV)
    wide[:, :e] = a
    a2, b2 = wide[:, :e], b.clone()
    got_in, got_out = splice_special_rows(a2, b2, s, SPECIAL, IN_REFERENCE, inplace=True)
    assert got_in.data_ptr() == a2.data_ptr() and got_out.data_ptr() == b2.data_ptr()
    assert torch.equal(_bits(a2), _bits(want_in)) and torch.equal(_bits(b2), _bits(want_out)) and bool((wide[:, e:] == 7.0).all())
    # no special indices: the inputs themselves
    same_in, same_out = splice_special_rows(a, b, s, [], [])
    assert same_in is a and same_out is b


@pytest.mark.parametrize("inplace", (False, True))
def test_splice_gradients_are_the_upstream_with_the_rows_zero(inplace):
    e = 64
    pred_in, pred_out, src, want_in, want_out = _splice_inputs(e, torch.float32)
    gen = torch.Generator().manual_seed(3)
    up_in, up_out = torch.randn(V, e, generator=gen).to(DEV), torch.randn(V, e, generator=gen).to(DEV)
    keep_in, keep_out = up_in.clone(), up_out.clone()
    a, b = pred_in.to(DEV).requires_grad_(True), pred_out.to(DEV).requires_grad_(True)
    s = src.to(DEV).requires_grad_(True)
    x, y = (a * 1.0, b * 1.0) if inplace else (a, b)          # in place needs a non-leaf, as the hypernetwork's outputs are
    got_in, got_out = splice_special_rows(x, y, s, SPECIAL, IN_REFERENCE, inplace=inplace)
    assert torch.equal(_bits(got_in), _bits(want_in)) and torch.equal(_bits(got_out), _bits(want_out))
    torch.autograd.backward([got_in, got_out], [up_in, up_out])
    for grad, up, keep in ((a.grad, up_in, keep_in), (b.grad, up_out, keep_out)):
        want = keep.clone()
        want[SPECIAL] = 0.0
        assert torch.equal(_bits(grad), _bits(want))
        assert torch.equal(_bits(up), _bits(keep))          # the incoming gradient is never modified
    assert s.grad is None          # the source is a frozen target
    if inplace:
        with pytest.raises(RuntimeError):          # torch refuses an in-place write to a leaf that requires grad
            splice_special_rows(a, b, s, SPECIAL, IN_REFERENCE, inplace=True)


@pytest.mark.parametrize("case", [(257, 300, 29), (257, 300, 64)])
def test_no_grad_runs_the_gather_and_the_splice_only(case):
    t, v, e = case
    ids = recipe(*case)[0].to(DEV)
    pred = _table(v, e).to(DEV).requires_grad_(True)
    src = _table(R, 2 * e, seed=9).to(DEV)
    sp, ref = [0, v - 1, 100], [R - 1, 0, 7]
    with_grad_in, _ = splice_special_rows(pred, None, src, sp, ref)
    with_grad = token_embeddings(with_grad_in, ids, dtype=torch.bfloat16)
    assert with_grad_in.grad_fn is not None and with_grad.grad_fn is not None
    with torch.no_grad():
        quiet_in, _ = splice_special_rows(pred, None, src, sp, ref)
        quiet = token_embeddings(quiet_in, ids, dtype=torch.bfloat16)
    assert quiet_in.grad_fn is None and quiet.grad_fn is None and not quiet.requires_grad
    assert torch.equal(quiet_in, with_grad_in.detach()) and torch.equal(quiet, with_grad.detach())
    plain = token_embeddings(pred.detach(), ids, dtype=torch.bfloat16)          # nothing requires grad: no Function, no plan
    assert plain.grad_fn is None and not plain.requires_grad


# ---- the whole input side in a training step -------------------------------------------------------------------------------------------
def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-300))


def _tiny(seed, rows=64):          # (the case of tests/test_lm_loss_gpu.py)
    from zett_amd.config import ZettHypernetConfig
    from zett_amd.hypernet import ZettHypernet
    cfg, *_ = synth.workload("tiny")
    w = synth.make_weights(cfg, seed=seed)
    src = synth.make_source_embeddings(cfg, seed)
    ids = synth.make_surface_forms(cfg, rows, seed=seed, n_special=1)
    ids[::3, 1:] = cfg["pad_token_id"]                                  # single-token rows for the lexical loss
    models = []
    for _ in range(2):
        model = ZettHypernet(ZettHypernetConfig(**cfg))
        model.load_state_dict({k: torch.from_numpy(x) for k, x in w.items()})
        models.append(model.to(DEV).requires_grad_(True).train())
    return cfg, models, torch.from_numpy(src).to(DEV), torch.from_numpy(ids).to(DEV)


def test_training_a_tiny_hypernet_through_splice_and_lookup():
    """hypernet -> splice (in place) -> lookup -> a toy causal backbone -> lm_head_loss + 0.5 lexical_loss on the spliced matrices -> backward ->
    HypernetAdamW.step.  The first step's parameter gradients equal those of torch's index_copy / F.embedding / F.cross_entropy in the same
    places; ours twice from the same state gives the same bits.

    `ours` runs the hypernetwork's dense schedule (``train_packed = False``): everything from the hypernetwork's outputs to the loss and
    back is fixed-order, and so is the dense backward, so EVERY parameter gradient is compared bit for bit.  The default packed schedule adds
    the uses of a distinct id with float atomics in its own backward (zett_amd/autograd.py backward_packed), which moves
    the last bits of the embedding-side parameter gradients from run to run whatever sits behind the hypernetwork (measured: 3 to 12 of
    86 parameters, with or without this feature in the graph); under it the gradients that ARRIVE at the hypernetwork's outputs — all that
    the splice, the lookup, the backbone and the losses produce — are held to the same bits instead."""
    from zett_amd.training import HypernetAdamW, lexical_loss, lm_head_loss
    rows, batch, seq, pad_id = 64, 4, 24, 3
    cfg, (ours, theirs), src, sfm = _tiny(seed=83, rows=rows)
    pad, e = cfg["pad_token_id"], cfg["n_embd"]
    gen = torch.Generator().manual_seed(1234)
    input_ids = torch.randint(0, rows, (batch, seq), generator=gen)
    input_ids[:, 5] = input_ids[:, 2]          # repeats within a sequence, besides those chance gives
    input_ids[1, 15:] = pad_id
    input_ids[3, 20:] = pad_id                 # the pad id fills the tail of two sequences
    labels = torch.randint(0, rows, (batch, seq), generator=gen).to(DEV)
    mix = (torch.randn(e, e, generator=gen) / e ** 0.5).to(DEV)
    input_ids = input_ids.to(DEV)
    special, in_reference = [pad_id, 40], [1, 7]
    lang = torch.tensor(2)
    steps = torch.arange(1, seq + 1, device=DEV, dtype=torch.float32)[:, None]

    def backbone(x):
        return x + torch.tanh(torch.cumsum(x, 1) / steps @ mix)

    def total(model, use_torch, tap=None):
        pred_in, pred_out, _bias = model(sfm, source_embeddings=src, lang_index=lang)
        if tap is not None:          # the gradients arriving at the hypernetwork's outputs
            pred_in.register_hook(lambda g: tap.__setitem__("d pred_in", g.clone()))
            pred_out.register_hook(lambda g: tap.__setitem__("d pred_out", g.clone()))
        if use_torch:
            idx, ref = torch.tensor(special, device=DEV), torch.tensor(in_reference, device=DEV)
            pred_in = pred_in.index_copy(0, idx, src[ref, :e].float())
            pred_out = pred_out.index_copy(0, idx, src[ref, e:2 * e].float())
            hidden = backbone(F.embedding(input_ids, pred_in))
            lm = F.cross_entropy((hidden @ pred_out.T).view(-1, rows), labels.view(-1))
        else:
            pred_in, pred_out = splice_special_rows(pred_in, pred_out, src, special, in_reference, inplace=True)
            hidden = backbone(token_embeddings(pred_in, input_ids))
            lm = lm_head_loss(hidden, pred_out, labels, precision="f32")[0]
        return lm + 0.5 * lexical_loss(pred_in, pred_out, src, sfm, pad)[0]

    def grads(model):
        return {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    total(theirs, True).backward()
    arrived = ({}, {})
    for tap in arrived:          # the default packed schedule: what this side of the hypernetwork hands back, twice
        total(ours, False, tap).backward()
        ours.zero_grad(set_to_none=True)
    assert set(arrived[0]) == {"d pred_in", "d pred_out"} and all(torch.equal(_bits(arrived[0][k]), _bits(arrived[1][k])) for k in arrived[0])
    assert not _bits(arrived[0]["d pred_in"])[special].any() and not _bits(arrived[0]["d pred_out"])[special].any()          # spliced rows: no gradient
    ours.train_packed = False          # the dense schedule: no float atomics anywhere in the step (see the docstring)
    total(ours, False).backward()
    first = grads(ours)
    ours.zero_grad(set_to_none=True)
    total(ours, False).backward()
    again = grads(ours)
    assert first.keys() == again.keys() and all(torch.equal(_bits(first[n]), _bits(again[n])) for n in first)          # two runs, the same bits
    ours.zero_grad(set_to_none=True)
    ours.train_packed = True          # the default schedule again, as `theirs` runs: the comparison with torch and the five steps

    opt = HypernetAdamW(ours, lr=1e-3)
    losses = []
    for step in range(5):
        loss = total(ours, False)
        loss.backward()
        if step == 0:
            # (the rule of tests/test_lm_loss_gpu.py: a gradient that is zero in exact arithmetic is round-off on both sides, and is held to
            # "negligible next to the largest gradient" instead of to a relative error between two noises)
            want, worst = dict(theirs.named_parameters()), {}
            floor = 1e-6 * max(float(q.grad.double().norm()) for q in want.values() if q.grad is not None)
            for name, p in ours.named_parameters():
                if p.grad is None and want[name].grad is None:
                    continue
                ref = want[name].grad.double()
                if float(ref.norm()) < floor:
                    assert float(p.grad.double().norm()) < floor, (name, float(p.grad.double().norm()), floor)
                else:
                    worst[name] = _rel(p.grad, ref)
            print("worst relative gradient error:", max(worst.values()), "over", len(worst), "parameters")
            bad = {k: x for k, x in worst.items() if x > GRAD_LIMIT_F32}
            assert not bad and len(worst) >= 40, bad
        opt.step(zero_grad=True)
        losses.append(loss.detach())
    losses = [float(x) for x in torch.stack(losses).cpu()]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    assert opt.last_step_stats()["step"] == 5
