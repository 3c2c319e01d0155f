"""zett_amd.training.HypernetAdafactor on the GPU, on the tiny hypernetwork of the existing training tests: five steps of
lm_head_loss + 0.5 lexical_loss -> backward -> step, every parameter and statistic of every step against the float64 definition
(tests/adafactor_ref.py through tests/adafactor_check.tensor_step and its bounds) applied to the same gradients; the frozen Rescalers,
the shapes of the state, the state_dict round trip, the refreshed engine, the swap with HypernetAdamW through make_optimizer and the
run-to-run bits under train_deterministic."""
import pytest
import torch

from tests import adafactor_check as ac
from tests import adafactor_ref as ref
from tests import train_ops_check as tc
from zett_amd import synth
from zett_amd.training import (HypernetAdafactor, HypernetAdamW, adafactor_state_shapes, lexical_loss, lm_head_loss, make_optimizer, param_labels,
                               splice_special_rows, token_embeddings)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LR, WD, MAX_NORM = 1e-2, 0.01, 0.1


def _bits(a):
    return a.detach().cpu().contiguous().view(torch.int32)


def _model(seed, rows=64):
    from zett_amd.config import ZettHypernetConfig
    from zett_amd.hypernet import ZettHypernet
    cfg, *_ = synth.workload("tiny")
    w = synth.make_weights(cfg, seed=seed)
    src = synth.make_source_embeddings(cfg, seed)
    ids = synth.make_surface_forms(cfg, rows, seed=seed, n_special=1)
    ids[::3, 1:] = cfg["pad_token_id"]                                  # single-token rows for the lexical loss
    model = ZettHypernet(ZettHypernetConfig(**cfg))
    model.load_state_dict({k: torch.from_numpy(x) for k, x in w.items()})
    return cfg, model.to(DEV).requires_grad_(True).train(), torch.from_numpy(src).to(DEV), torch.from_numpy(ids).to(DEV)


class _Step:
    """the training step of tests/test_embed_lookup_gpu.py: hypernet -> splice -> lookup -> a toy causal backbone -> the two losses"""

    def __init__(self, seed=83, rows=64, deterministic=False):
        self.cfg, self.model, self.src, self.sfm = _model(seed, rows)
        if deterministic:
            self.model.train_deterministic = True
        batch, seq, pad_id = 4, 24, 3
        e = self.cfg["n_embd"]
        gen = torch.Generator().manual_seed(1234)
        self.input_ids = torch.randint(0, rows, (batch, seq), generator=gen).to(DEV)
        self.labels = torch.randint(0, rows, (batch, seq), generator=gen).to(DEV)
        self.mix = (torch.randn(e, e, generator=gen) / e ** 0.5).to(DEV)
        self.steps = torch.arange(1, seq + 1, device=DEV, dtype=torch.float32)[:, None]
        self.special, self.in_reference = [pad_id, 40], [1, 7]

    def loss(self):
        pred_in, pred_out, _bias = self.model(self.sfm, source_embeddings=self.src, lang_index=torch.tensor(2))
        pred_in, pred_out = splice_special_rows(pred_in, pred_out, self.src, self.special, self.in_reference, inplace=True)
        x = token_embeddings(pred_in, self.input_ids)
        hidden = x + torch.tanh(torch.cumsum(x, 1) / self.steps @ self.mix)
        lm = lm_head_loss(hidden, pred_out, self.labels, precision="f32")[0]
        return lm + 0.5 * lexical_loss(pred_in, pred_out, self.src, self.sfm, self.cfg["pad_token_id"])[0]

    def backward(self):
        loss = self.loss()
        loss.backward()
        return loss.detach()


def _snapshot(model, opt):
    return ({n: p.detach().cpu().clone() for n, p in model.named_parameters()}, {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters() if p.grad is not None},
            {n: {k: t.cpu().clone() for k, t in st.items()} for n, st in opt.state.items()})


def test_five_steps_against_the_definition():
    s = _Step()
    model = s.model
    labels = param_labels(model)
    opt = HypernetAdafactor(model, lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
    init = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    with torch.no_grad():
        before = s.model(s.sfm, source_embeddings=s.src, lang_index=torch.tensor(2))[0].clone()
    losses = []
    for t in range(5):
        losses.append(s.backward())
        params, grads, states = _snapshot(model, opt)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                  # the step never waits for the host
        try:
            opt.step(zero_grad=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        stats = opt.last_step_stats()
        words = opt.record.cpu()
        want = ac.record_ref(list(grads.values()), MAX_NORM, t)
        assert stats["step"] == t + 1 and stats["skipped"] == 0
        tc.check(torch.stack([words[0], words[1], words[4], words[5]]), torch.stack([want[k][0] for k in ("norm", "coef", "beta", "omb")]),
                 torch.stack([torch.as_tensor(want[k][1], dtype=torch.float64) for k in ("norm", "coef", "beta", "omb")]), f"step {t}: norm, coef, beta, 1 - beta")
        assert stats["grad_norm"] == float(words[0]) and stats["clip_coef"] == float(words[1])
        coef, beta, omb = float(words[1]), float(words[4]), float(words[5])
        for n, p in model.named_parameters():
            if n not in grads:
                assert torch.equal(_bits(p), _bits(init[n])) and n not in opt.state, n          # no gradient: not in the step
                continue
            assert not p.grad.any(), n                            # zero_grad cleared it in the same pass
            if labels[n] == "frozen":
                assert torch.equal(_bits(p), _bits(init[n])) and n not in opt.state, n          # Rescalers: bit-unchanged, no state
                continue
            st0 = states.get(n) or {k: torch.zeros(shape) for k, shape in ref.state_shapes(tuple(p.shape)).items()}
            assert {k: tuple(v.shape) for k, v in opt.state[n].items()} == adafactor_state_shapes(p.shape) == ref.state_shapes(tuple(p.shape)), n
            flags = ac.DECAY if labels[n] == "decay" else 0
            r = ac.tensor_step(params[n], grads[n], st0, flags, coef, beta, omb, LR, WD)
            tc.check(p.detach().cpu(), r["p"], r["b_p"], f"step {t} {n}")
            for k in r["state"]:
                tc.check(opt.state[n][k].cpu(), r["state"][k], r["b_state"][k], f"step {t} {n} {k}")
    assert sum(1 for l in labels.values() if l == "frozen") == 4 and stats["clip_coef"] < 1.0
    assert float(losses[-1]) < float(losses[0]) and all(bool(torch.isfinite(l)) for l in losses)
    assert sum(t.numel() for st in opt.state.values() for t in st.values()) < 0.2 * sum(p.numel() for n, p in model.named_parameters() if labels[n] != "frozen")
    with torch.no_grad():                                         # the engine was refreshed: a no_grad forward sees the new weights
        after = s.model(s.sfm, source_embeddings=s.src, lang_index=torch.tensor(2))[0]
    assert not after.requires_grad and not torch.equal(before, after)


def test_state_dict_round_trip_gives_the_same_sixth_step():
    a, b = _Step(seed=13), _Step(seed=13)
    oa, ob = HypernetAdafactor(a.model, lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM), HypernetAdafactor(b.model, lr=5.0, weight_decay=0.5, max_grad_norm=None)
    for _ in range(5):
        a.backward()
        oa.step(zero_grad=True)
    sd = oa.state_dict()
    assert sd["step"] == 5 and sd["hyper"] == {"lr": LR, "weight_decay": WD, "max_grad_norm": MAX_NORM}
    with torch.no_grad():
        for p, q in zip(a.model.parameters(), b.model.parameters()):
            q.copy_(p)
    b.model.refresh_weights()
    ob.load_state_dict(sd)
    a.backward()
    grads = {n: p.grad.clone() for n, p in a.model.named_parameters() if p.grad is not None}
    for n, q in b.model.named_parameters():                       # the same gradients: what is compared is the optimizer, not the backward's atomics
        q.grad = grads[n].clone() if n in grads else None
    oa.step()
    ob.step()
    assert oa.last_step_stats() == ob.last_step_stats() and oa.last_step_stats()["step"] == 6
    for (n, p), q in zip(a.model.named_parameters(), b.model.parameters()):
        assert torch.equal(_bits(p), _bits(q)), n
    for n in oa.state:
        assert all(torch.equal(_bits(oa.state[n][k]), _bits(ob.state[n][k])) for k in oa.state[n]), n


def test_a_non_finite_gradient_skips_the_step():
    s = _Step(seed=21)
    opt = HypernetAdafactor(s.model, lr=LR)
    s.backward()
    opt.step(zero_grad=True)
    s.backward()
    big = next(n for n, p in s.model.named_parameters() if p.grad is not None and p.dim() == 2 and min(p.shape) >= 128)
    dict(s.model.named_parameters())[big].grad[3, 5] = float("nan")
    params, grads, states = _snapshot(s.model, opt)
    opt.step()
    stats = opt.last_step_stats()
    assert stats["skipped"] == 1 and stats["step"] == 1 and stats["clip_coef"] == 0.0
    for n, p in s.model.named_parameters():
        assert torch.equal(_bits(p), _bits(params[n])), n
        assert p.grad is None or torch.equal(_bits(p.grad), _bits(grads[n])), n          # without zero_grad nothing is cleared
    for n, st in opt.state.items():
        assert all(torch.equal(_bits(st[k]), _bits(states[n][k])) for k in st), n
    opt.step(zero_grad=True)
    assert opt.last_step_stats()["skipped"] == 1 and all(not p.grad.any() for p in s.model.parameters() if p.grad is not None)


def test_make_optimizer_swaps_the_two_and_adamw_is_unchanged():
    """the same gradients through make_optimizer(use_adafactor=False) and through HypernetAdamW built by hand: the same bits; through
    make_optimizer(use_adafactor=True): a HypernetAdafactor with the same interface, which moves the parameters too"""
    args = dict(learning_rate=[1e-3, 1e-5], weight_decay=0.01, max_grad_norm=0.1, adam_beta1=0.9, adam_beta2=0.95, adam_epsilon=1e-8)
    runs = {}
    for name in ("by hand", "adamw", "adafactor"):
        s = _Step(seed=5)
        if name == "by hand":
            opt = HypernetAdamW(s.model, lr=1e-3, betas=(0.9, 0.95), eps=1e-8, weight_decay=0.01, max_grad_norm=0.1)
        else:
            opt = make_optimizer(s.model, dict(args, use_adafactor=name == "adafactor"))
        gen = torch.Generator(device=DEV).manual_seed(23)
        init = {n: p.detach().clone() for n, p in s.model.named_parameters()}
        for _ in range(2):
            for n, p in s.model.named_parameters():
                p.grad = torch.randn(p.shape, device=DEV, generator=gen) * 1e-2
            opt.step(lr=2e-3, zero_grad=True)
        assert set(opt.last_step_stats()) == {"grad_norm", "clip_coef", "skipped", "step"} and opt.last_step_stats()["step"] == 2
        assert set(opt.state_dict()) == {"step", "state", "hyper", "labels"}
        runs[name] = (type(opt), {n: p.detach().clone() for n, p in s.model.named_parameters()}, init)
    assert runs["adamw"][0] is HypernetAdamW and runs["adafactor"][0] is HypernetAdafactor
    assert all(torch.equal(_bits(runs["adamw"][1][n]), _bits(runs["by hand"][1][n])) for n in runs["adamw"][1])
    moved = [n for n, p in runs["adafactor"][1].items() if not torch.equal(p, runs["adafactor"][2][n])]
    assert len(moved) == 83 and any(not torch.equal(runs["adafactor"][1][n], runs["adamw"][1][n]) for n in moved)


def test_two_deterministic_runs_end_in_the_same_bits():
    ends = []
    for _ in range(2):
        s = _Step(seed=31, deterministic=True)
        opt = HypernetAdafactor(s.model, lr=LR, weight_decay=WD, max_grad_norm=MAX_NORM)
        for _ in range(3):
            s.backward()
            opt.step(zero_grad=True)
        ends.append(({n: _bits(p) for n, p in s.model.named_parameters()}, {n: {k: _bits(t) for k, t in st.items()} for n, st in opt.state.items()}, opt.last_step_stats()))
    assert ends[0][2] == ends[1][2] and ends[0][2]["step"] == 3
    assert all(torch.equal(ends[0][0][n], ends[1][0][n]) for n in ends[0][0])
    assert all(torch.equal(ends[0][1][n][k], ends[1][1][n][k]) for n in ends[0][1] for k in ends[0][1][n])
