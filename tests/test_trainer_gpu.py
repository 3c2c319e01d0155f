"""zett_amd.trainer on the GPU: a few steps of the tiny hypernetwork in front of a toy backbone (one fixed mixing matrix).  With
``train_precision="f32"``, ``train_deterministic=True`` and ``lm_precision="f32"`` a step is a pure function of its inputs, so the trainer is
held to the same steps written out by hand from the public functions bit for bit (``torch.equal``), with no tolerance anywhere."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import collate_ref as cr
from zett_amd import synth
from zett_amd.collate import DeviceCollator
from zett_amd.config import ZettHypernetConfig
from zett_amd.hypernet import ZettHypernet
from zett_amd.trainer import HypernetTrainer, device_loader, learning_rate_schedule, loader_draw
from zett_amd.training import identity_loss, lexical_loss, lm_head_loss, make_optimizer, splice_special_rows, token_embeddings

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOCK, N_SUB, LANGS = 32, 256, ["de", "en", "fr"]
WORDS = "the quick brown fox jumps over the lazy dog , it's 12 345 times . we'll see".split(" ")


def _args(**kw):
    import types
    base = dict(do_tokenizer_sampling=False, n_token_subsample=None, pad_to_multiple_of=8, subsample_mode="random", block_size=BLOCK, use_passthrough_hypernet=False,
                add_prefix_space=False, hn_surface_maxlen=7, sample_text_span=True, langs=LANGS, tokenizer_sample_max=1536, tokenizer_sample_min=1100,
                tokenizer_sample_mean=1200, tokenizer_sample_std=30, tokenizer_noise_mean=0.0, tokenizer_noise_std=0.0)
    return types.SimpleNamespace(**dict(base, **kw))


def _texts(seed, n=4):
    rng = np.random.default_rng(seed)
    return [" ".join(WORDS[i] for i in rng.integers(0, len(WORDS), size=int(rng.integers(8, 30)))) for _ in range(n)]


def _training_args(**kw):
    base = dict(loss="clm", steps=20, warmup_steps=3, learning_rate=1e-3, learning_rate_alpha=0.1, lexical_loss_weight=0.5, max_grad_norm=0.1, weight_decay=0.01,
                adam_beta2=0.95, logging_steps=2, save_steps=1000, eval_steps=1000, seed=11, output_dir=None)
    return dict(base, **kw)


class Setup:
    """What every test shares, built once: the configuration, the source matrix, collators and batches.  Nothing in it is written after
    construction; models and optimizers are built per test."""

    def __init__(self):
        cfg, *_ = synth.workload("tiny")
        self.cfg = dict(cfg, original_vocab_size=420, vocab_size=425)          # the hn tokenizer's 420 ids
        self.e = self.cfg["n_embd"]
        self.weights = {k: torch.from_numpy(x) for k, x in synth.make_weights(self.cfg, seed=83).items()}
        src = torch.from_numpy(synth.make_source_embeddings(self.cfg, 83)).to(DEV)
        self.src = torch.cat([src, src[:8].flip(0)]).contiguous()          # (row 420: the reference's <mask>)
        self.hn = cr.bpe_tokenizer(False)
        self.pad = self.hn.pad_token_id
        self.collators = {}
        mix = (torch.randn(self.e, self.e, generator=torch.Generator().manual_seed(1)) / self.e ** 0.5).to(DEV)
        self.backbone = lambda x, attention_mask=None: x + torch.tanh(x @ mix)
        c = self.collator("clm", N_SUB)
        self.data = {lang: [{"texts": _texts(10 * j + i), "lang_code": lang} for i in range(3)] for j, lang in enumerate(LANGS)}
        self.batches = [c([self.data[lang][i]], seed=100 + 7 * i + j, check=False) for i in range(2) for j, lang in enumerate(LANGS)]          # de en fr de en fr
        self.identity = [c(None, True, seed=s) for s in (9, 10)]

    def collator(self, loss, n):
        if (loss, n) not in self.collators:
            self.collators[loss, n] = DeviceCollator(cr.bpe_tokenizer(), self.hn, _args(n_token_subsample=n), loss=loss,
                                                     tokenizer=cr.bpe_tokenizer(), device=DEV)
        return self.collators[loss, n]

    def model(self):
        model = ZettHypernet(ZettHypernetConfig(**self.cfg))
        model.load_state_dict(self.weights)
        model = model.to(DEV).requires_grad_(True).train()
        model.train_precision, model.train_deterministic = "f32", True
        return model

    def trainer(self, model=None, **kw):
        return HypernetTrainer(self.model() if model is None else model, self.backbone, self.src, _training_args(**kw), hn_pad_token_id=self.pad, lm_precision="f32",
                               langs=LANGS)

    # ---- the steps by hand, from the public functions ----
    def lm(self, batch, pred_in, pred_out, loss="clm"):
        hidden = self.backbone(token_embeddings(pred_in, batch["input_ids"]))
        return lm_head_loss(hidden, pred_out, batch["labels"], batch["attention_mask"], mode=loss, priors=batch["target_priors"], vocab_mask=batch["mask"], precision="f32")

    def backward(self, model, batch, k=1):
        pred_in, pred_out, _ = model(batch["target_surface_forms"], source_embeddings=self.src, lang_index=batch["lang_index"])
        pred_in, pred_out = splice_special_rows(pred_in, pred_out, self.src, batch["special_indices"], batch["special_indices_in_reference"], inplace=True)
        lm, _ = self.lm(batch, pred_in, pred_out)
        lex, overlap = lexical_loss(pred_in, pred_out, self.src, batch["target_surface_forms"], self.pad, kind="mse")
        loss = lm + 0.5 * lex
        (loss / k).backward()
        return {"loss": loss.detach(), "lexical_loss": lex.detach(), "mean_lexical_overlap": overlap.detach()}

    def identity_backward(self, model, batch, k=1):
        pred_in, pred_out, _ = model(batch["target_surface_forms"], source_embeddings=self.src, lang_index=batch["lang_index"])
        loss = identity_loss(pred_in, pred_out, self.src, batch["ids_to_embed"])
        (loss / k).backward()
        return {"identity_loss": loss.detach()}


@pytest.fixture(scope="module")
def setup():
    s = Setup()
    yield s
    for c in s.collators.values():
        c.encoder.close()


def _same_state(a, b, opt_a, opt_b):
    pa, pb = dict(a.named_parameters()), dict(b.named_parameters())
    assert pa.keys() == pb.keys()
    for n in pa:
        assert torch.equal(pa[n], pb[n]), ("parameter", n)
    assert opt_a.state.keys() == opt_b.state.keys() and len(opt_a.state) > 0
    for n, st in opt_a.state.items():
        assert st.keys() == opt_b.state[n].keys()
        for k in st:
            assert torch.equal(st[k], opt_b.state[n][k]), ("moment", n, k)
    assert opt_a.last_step_stats()["step"] == opt_b.last_step_stats()["step"]


def _equal_metrics(got, want):
    for key, value in want.items():
        assert torch.equal(got[key], value), (key, float(got[key]), float(value))


# 1 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("use_adafactor", (False, True), ids=("adamw", "adafactor"))
def test_three_micro_steps_equal_the_steps_by_hand(setup, use_adafactor):
    trainer = setup.trainer(use_adafactor=use_adafactor)
    assert type(trainer.optimizer).__name__ == ("HypernetAdafactor" if use_adafactor else "HypernetAdamW")
    model = setup.model()
    opt = make_optimizer(model, _training_args(use_adafactor=use_adafactor))
    schedule = learning_rate_schedule(_training_args())
    for step, batch in enumerate(setup.batches[:3]):
        got = trainer.train_micro_step(batch)
        want = setup.backward(model, batch)
        opt.step(lr=schedule(step), zero_grad=True)
        _equal_metrics(got, want)
        assert got["learning_rate"] == schedule(step) and set(got) == {"loss", "lexical_loss", "mean_lexical_overlap", "learning_rate", "grad_norm", "skipped"}
        assert float(got["grad_norm"]) == opt.last_step_stats()["grad_norm"] > 0 and int(got["skipped"]) == 0
    assert trainer.micro_step == 3 and schedule(2) > schedule(1) > 0
    _same_state(trainer.hypernet, model, trainer.optimizer, opt)
    assert any(not torch.equal(p.detach().cpu(), setup.weights[n]) for n, p in model.named_parameters())          # and the steps moved the parameters


# 2 ----------------------------------------------------------------------------------------------------------------------------------------
def test_accumulation_over_two_micro_steps(setup):
    trainer = setup.trainer(gradient_accumulation_steps=2)
    model = setup.model()
    opt = make_optimizer(model, _training_args())
    schedule = learning_rate_schedule(_training_args())
    for m, batch in enumerate(setup.batches[:4]):
        got = trainer.train_micro_step(batch)
        _equal_metrics(got, setup.backward(model, batch, k=2))
        assert got["learning_rate"] == schedule(m // 2)
        if m % 2 == 1:
            opt.step(lr=schedule(m // 2), zero_grad=True)
        assert ("grad_norm" in got) == (m % 2 == 1)
    assert opt.last_step_stats()["step"] == 2
    _same_state(trainer.hypernet, model, trainer.optimizer, opt)


# 3 ----------------------------------------------------------------------------------------------------------------------------------------
class Counted:
    """a re-iterable that counts its restarts and the items it handed out"""

    def __init__(self, items):
        self.items, self.starts, self.taken = list(items), 0, 0

    def __iter__(self):
        self.starts += 1
        for item in self.items:
            self.taken += 1
            yield item


def test_fit_identity_then_training_with_windows_and_restarts(setup):
    args = dict(identity_steps=2, steps=5, logging_steps=2)
    trainer = setup.trainer(**args)
    identity, train = Counted(setup.identity[:1]), Counted(setup.batches[1:3])          # both shorter than their phase: en, fr
    logged = []
    trainer.fit([train], [1.0], identity_loader=identity, log=lambda metrics, step: logged.append((step, metrics)))
    assert (identity.starts, identity.taken) == (2, 2) and (train.starts, train.taken) == (2, 3) and trainer.micro_step == 5
    model = setup.model()
    opt = make_optimizer(model, _training_args(**args))
    schedule = learning_rate_schedule(_training_args(**args))
    records = []
    for step, (batch, identity_step) in enumerate([(setup.identity[0], True)] * 2 + [(setup.batches[1], False), (setup.batches[2], False), (setup.batches[1], False)]):
        records.append(setup.identity_backward(model, batch) if identity_step else setup.backward(model, batch))
        opt.step(lr=schedule(step), zero_grad=True)
    _same_state(trainer.hypernet, model, trainer.optimizer, opt)
    assert [step for step, _ in logged] == [2, 4]          # (the fifth update ends no window)
    first, second = logged[0][1], logged[1][1]
    assert first["train/identity_loss"] == np.mean([float(r["identity_loss"]) for r in records[:2]]) and "train/loss" not in first and "train/en_loss" not in first
    assert first["train/learning_rate"] == np.mean([schedule(0), schedule(1)]) and first["train/skipped"] == 0.0 and first["train/grad_norm"] > 0
    for key in ("loss", "lexical_loss", "mean_lexical_overlap"):
        assert second["train/" + key] == np.mean([float(r[key]) for r in records[2:4]]), key
    assert second["train/en_loss"] == float(records[2]["loss"]) and second["train/fr_loss"] == float(records[3]["loss"]) and math.isnan(second["train/de_loss"])
    assert "train/identity_loss" not in second and second["train/time"] >= first["train/time"] > 0
    for lang, batch in (("en", setup.batches[1]), ("fr", setup.batches[2])):
        assert second[f"train/{lang}_avg_byte_length"] == float(batch["metrics"]["avg_byte_length"]) and second[f"train/{lang}_std_byte_length"] == 0.0
        assert second[f"train/{lang}_unk_ratio"] == float(batch["metrics"]["unk_ratio"])
        assert second[f"train/{lang}_pad_ratio"] == float((batch["attention_mask"] == 0).double().mean())
    assert "train/de_avg_byte_length" not in second


# 4 ----------------------------------------------------------------------------------------------------------------------------------------
def test_a_non_finite_batch_is_skipped(setup):
    good, after = setup.batches[0], setup.batches[1]
    priors = good["target_priors"].clone()
    priors[int(good["labels"][0, 1])] = math.inf          # +inf on a logit: the softmax of that column is inf - inf
    bad = dict(good, target_priors=priors)
    trainer = setup.trainer()
    trainer.train_micro_step(good)
    before = {n: p.detach().clone() for n, p in trainer.hypernet.named_parameters()}
    moments = {n: {k: t.clone() for k, t in st.items()} for n, st in trainer.optimizer.state.items()}
    got = trainer.train_micro_step(bad)
    assert not math.isfinite(float(got["loss"])) and int(got["skipped"]) == 1 and not math.isfinite(float(got["grad_norm"]))
    assert all(torch.equal(p, before[n]) for n, p in trainer.hypernet.named_parameters())
    assert all(torch.equal(t, moments[n][k]) for n, st in trainer.optimizer.state.items() for k, t in st.items())
    got = trainer.train_micro_step(after)
    assert int(got["skipped"]) == 0 and math.isfinite(float(got["loss"])) and math.isfinite(float(got["grad_norm"]))
    model = setup.model()
    opt = make_optimizer(model, _training_args())
    schedule = learning_rate_schedule(_training_args())
    for step, batch in ((0, good), (2, after)):          # the skipped update still spends its place in the schedule
        setup.backward(model, batch)
        opt.step(lr=schedule(step), zero_grad=True)
    assert all(torch.equal(p, q) for p, q in zip(trainer.hypernet.parameters(), model.parameters())) and trainer.optimizer.last_step_stats()["step"] == 2
    logged = []
    setup.trainer(steps=3, warmup_steps=1, logging_steps=3).fit([[good, bad, after]], [1.0], log=lambda metrics, step: logged.append(metrics))
    assert len(logged) == 1 and logged[0]["train/skipped"] == 1.0 / 3.0 and not math.isfinite(logged[0]["train/loss"])


# 5 ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ("clm", "mlm"))
def test_evaluate_caches_for_a_fixed_tokenizer_and_restores_the_mode(setup, loss):
    c = setup.collator(loss, None)          # the whole vocabulary, padded: every batch of the set has the same rows
    batches = [c([setup.data[lang][2]], seed=300 + j, check=False) for j, lang in enumerate(("en", "en", "fr"))]
    trainer = setup.trainer(loss=loss)
    model = trainer.hypernet
    calls = []
    model.register_forward_pre_hook(lambda *a: calls.append(model.training))
    got = trainer.evaluate({"fixed": batches, "sampled": (batches, True)}, LANGS)
    assert calls == [False] * 4 and model.training          # once for the fixed set, once per batch of the set flagged as sampling; eval() inside, train() after
    second = "bpb" if loss == "clm" else "acc"
    want = {name: {"loss": [], second: []} for name in ("fixed", "sampled")}
    model.eval()
    with torch.no_grad():
        cache = None
        for batch in batches:
            pred_in, pred_out, _ = model(batch["target_surface_forms"], source_embeddings=setup.src, lang_index=batch["lang_index"])
            pred_in, pred_out = splice_special_rows(pred_in, pred_out, setup.src, batch["special_indices"], batch["special_indices_in_reference"], inplace=True)
            cache = (pred_in, pred_out) if cache is None else cache          # the first batch's (language "en"), as eval_loop keeps them: for the "fr" batch too
            for name, (p_in, p_out) in (("fixed", cache), ("sampled", (pred_in, pred_out))):
                value, stats = setup.lm(batch, p_in, p_out, loss)
                want[name]["loss"].append(float(value))
                if loss == "clm":
                    want[name][second].append(float((stats["row_loss"].view(len(batch["labels"]), BLOCK).sum(-1) / batch["byte_lengths"].sum(-1)).mean()))
                else:
                    assert int(stats["n_counted"]) > 0
                    want[name][second].append(float(stats["n_correct"] / stats["n_counted"]))
    model.train()
    assert want["fixed"]["loss"][:2] == want["sampled"]["loss"][:2] and want["fixed"]["loss"][2] != want["sampled"]["loss"][2]          # (the language id is embedded)
    for name in ("fixed", "sampled"):
        for key, values in want[name].items():
            assert got[f"eval/{name}_en_{key}"] == np.mean(values[:2]) and got[f"eval/{name}_fr_{key}"] == values[2], (name, key)
        assert f"eval/{name}_de_loss" not in got
        lengths = [float(b["metrics"]["avg_byte_length"]) for b in batches]
        assert got[f"eval/{name}_en_avg_byte_length"] == np.mean(lengths[:2]) and got[f"eval/{name}_en_std_byte_length"] == np.std(lengths[:2])
        assert got[f"eval/{name}_fr_unk_ratio"] == float(batches[2]["metrics"]["unk_ratio"])
    metrics, cache = trainer.eval_step(batches[0])
    again, same = trainer.eval_step(batches[1], cache)
    assert same is cache and float(again["loss"]) == want["fixed"]["loss"][1] and set(metrics) == {"loss", second}


# 6 ----------------------------------------------------------------------------------------------------------------------------------------
def _loaders(setup, sampled, opened):
    """fresh loaders for one run: with a fixed tokenizer the shared collator (a pure function of its seed); with a sampled one a collator and
    one DeviceTokenizerSampler of its own, whose queue moves with every batch"""
    if not sampled:
        c = setup.collator("clm", N_SUB)
    else:
        from zett_amd.tokenizer_sampling import DeviceTokenizerSampler
        sampler = DeviceTokenizerSampler(table_capacity=1 << 14, max_depth=2, max_pieces=1 << 12)
        c = DeviceCollator(cr.bpe_tokenizer(), setup.hn, _args(do_tokenizer_sampling=True, n_token_subsample=N_SUB, sample_text_span=False, add_prefix_space=True),
                           loss="clm", samplers={"en": [sampler], "fr": [sampler]}, device=DEV)
        opened += [sampler, c.vocabulary]
    return [device_loader(setup.data[lang], c, seed=5 + j) for j, lang in enumerate(("en", "fr"))]


@pytest.mark.parametrize("sampled", (False, True), ids=("fixed", "sampled"))
def test_resume_replays_the_data_and_continues_bit_for_bit(setup, tmp_path, sampled):
    opened = []
    try:
        _resume(setup, tmp_path, sampled, opened)
    finally:
        for x in opened:
            x.close()


def _resume(setup, tmp_path, sampled, opened):
    args = dict(steps=6, logging_steps=3, save_steps=3, output_dir=str(tmp_path / "run"))
    draws = [loader_draw(11, m, [0.5, 0.5]) for m in range(6)]
    assert len(set(draws[:3])) == 2 and max(draws.count(0), draws.count(1)) > 3          # both loaders before the checkpoint; one of them restarts (3 items each)
    whole, whole_log = setup.trainer(**args), []
    whole.fit(_loaders(setup, sampled, opened), [0.5, 0.5], log=lambda metrics, step: whole_log.append((step, metrics)))
    first = setup.trainer(**args)
    first.fit(_loaders(setup, sampled, opened), [0.5, 0.5], log=lambda *a: None, stop_after=3)
    assert first.micro_step == 3 and os.path.exists(os.path.join(args["output_dir"], "trainer_state.pt"))
    resumed, resumed_log = setup.trainer(**args), []
    resumed.resume(args["output_dir"])
    assert resumed.micro_step == 3
    _same_state(resumed.hypernet, first.hypernet, resumed.optimizer, first.optimizer)
    resumed.fit(_loaders(setup, sampled, opened), [0.5, 0.5], log=lambda metrics, step: resumed_log.append((step, metrics)))
    _same_state(resumed.hypernet, whole.hypernet, resumed.optimizer, whole.optimizer)
    assert [s for s, _ in whole_log] == [3, 6] and [s for s, _ in resumed_log] == [6]
    a, b = whole_log[-1][1], resumed_log[-1][1]
    assert a.keys() == b.keys() and "train/loss" in a
    for key in a:
        assert key == "train/time" or a[key] == b[key] or (math.isnan(a[key]) and math.isnan(b[key])), key
    # reset: the loaded parameters and moments (the directory holds the checkpoint of update 6 by now), the count and the schedule from 0
    reset = setup.trainer(resume_from_checkpoint_reset_steps=True, **args)
    reset.resume(args["output_dir"])
    assert reset.micro_step == 0
    _same_state(reset.hypernet, whole.hypernet, reset.optimizer, whole.optimizer)
    schedule = learning_rate_schedule(_training_args(**args))
    assert [reset.train_micro_step(setup.batches[0])["learning_rate"] for _ in range(2)] == [schedule(0), schedule(1)] and schedule(1) > 0
    assert reset.optimizer.last_step_stats()["step"] == 8          # the optimizer's own count goes on from the checkpoint's 6


# 7 ----------------------------------------------------------------------------------------------------------------------------------------
def _cli_config(tmp_path):
    """a 1-layer GPT-2 with its tokenizer, two tiny parquet tables and the config of a three-update run, all under tmp_path"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from transformers import GPT2Config, GPT2LMHeadModel
    tokenizer = cr.bpe_tokenizer(False)
    torch.manual_seed(0)
    GPT2LMHeadModel(GPT2Config(vocab_size=len(tokenizer), n_embd=64, n_head=2, n_layer=1, n_positions=32, bos_token_id=tokenizer.bos_token_id,
                               eos_token_id=tokenizer.eos_token_id)).save_pretrained(tmp_path / "model")
    tokenizer.save_pretrained(tmp_path / "model")
    for split, n in (("train", 24), ("valid", 8)):
        os.makedirs(tmp_path / split)
        pq.write_table(pa.table({"text": [" ".join(_texts(1000 * n + i, 1)) for i in range(n)]}), tmp_path / split / "en.parquet")
    out = tmp_path / "out"
    config = dict(output_dir=str(out), model_name_or_path=str(tmp_path / "model"), train_directory=str(tmp_path / "train"), valid_directory=str(tmp_path / "valid"), langs="en",
                  loss="clm", steps=3, logging_steps=1, save_steps=3, eval_steps=3, identity_steps=1, warmup_steps=1, learning_rate=1e-3, do_tokenizer_sampling=False,
                  add_prefix_space=False, do_sequence_packing=False,          # (the test tokenizer prepends its own space; packed texts would hold the eos string)
                  target_tokenizer_name=str(tmp_path / "model"), train_batch_size=4, eval_batch_size=4, block_size=32, n_token_subsample=256, identity_n_subsample=256,
                  pad_to_multiple_of=8, n_embd=64, hn_surface_maxlen=7, hn_n_layers=1, hn_hidden_size=64, hn_intermediate_size=128, hn_num_attention_heads=2,
                  hn_embed_using_source_embeddings=True, hn_rescale_embeddings=True, hn_embed_lang_id=True, hn_model_name_or_path=None, lexical_loss_weight=0.5, max_grad_norm=0.1,
                  dtype="float32", use_unigram_bias=True)
    return tokenizer, config


def test_cli_trains_logs_evaluates_and_saves(tmp_path):
    tokenizer, config = _cli_config(tmp_path)
    out = tmp_path / "out"
    (tmp_path / "cfg.json").write_text(json.dumps(config))
    with open(tmp_path / "stderr.log", "wb") as err:
        done = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "train.py"), str(tmp_path / "cfg.json")], cwd=REPO, timeout=240, stdout=subprocess.DEVNULL, stderr=err)
    assert done.returncode == 0, (tmp_path / "stderr.log").read_text()[-3000:]
    lines = [json.loads(line) for line in open(out / "metrics.jsonl")]
    assert [line["step"] for line in lines] == [1, 2, 3, 3]
    assert "train/identity_loss" in lines[0] and "train/loss" not in lines[0]
    for line in lines[1:3]:
        assert {"train/loss", "train/en_loss", "train/lexical_loss", "train/mean_lexical_overlap", "train/learning_rate", "train/grad_norm", "train/skipped", "train/time",
                "train/en_avg_byte_length", "train/en_std_byte_length", "train/en_unk_ratio", "train/en_pad_ratio"} <= set(line)
    assert {"eval/main_en_loss", "eval/main_en_bpb", "eval/main_en_avg_byte_length"} <= set(lines[3])
    assert all(math.isfinite(v) for line in lines for v in line.values())
    assert os.path.exists(out / "trainer_state.pt") and os.path.exists(out / "tokenizer.json")
    model = ZettHypernet.from_pretrained(out).to(DEV)
    src = torch.randn(len(tokenizer) + 4, 64, device=DEV) * 0.02
    with torch.no_grad():
        pred_in, pred_out, _ = model(torch.full((8, 7), 5, dtype=torch.int32, device=DEV), source_embeddings=src, lang_index=0)
    assert pred_in.shape == (8, 64) and pred_out is None and bool(torch.isfinite(pred_in).all())
