"""zett_amd.trainer / zett_amd.dataset / zett_amd.train_config without a GPU: the schedule against a hand-computed table, the datasets
against rows recorded from the reference's own classes (tests/golden/make_golden_dataset.py), window and evaluation aggregation against
hand-written records, the loader draw, config parsing and the constructor's refusals."""
import gzip
import json
import math
import os

import numpy as np
import pytest

from zett_amd.dataset import TrainDataset, ValidDataset
from zett_amd.train_config import parse_config
from zett_amd.trainer import HypernetTrainer, aggregate_eval, aggregate_window, item_seed, learning_rate_schedule, loader_draw

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _close(got, want):
    return math.isclose(got, want, rel_tol=1e-12, abs_tol=0.0) if want != 0 else got == 0


# ---- schedule -------------------------------------------------------------------------------------------------------------------------------
def test_schedule_table():
    s = learning_rate_schedule(dict(steps=100, warmup_steps=10, learning_rate=1e-3, learning_rate_alpha=0.1))
    for step, want in ((0, 0.0), (5, 5e-4), (10, 1e-3), (55, 5.5e-4), (100, 1e-4), (150, 1e-4)):
        assert _close(s(step), want), (step, s(step), want)


def test_schedule_random_warmup_table():
    s = learning_rate_schedule(dict(steps=100, warmup_steps=[10], learning_rate=1e-3, learning_rate_alpha=0.1, random_warmup_steps=4, random_learning_rate=2e-3))
    for step, want in ((2, 1e-3), (4, 0.0), (7, 5e-4), (10, 1e-3)):
        assert _close(s(step), want), (step, s(step), want)


def test_schedule_constant_stages_and_refusals():
    s = learning_rate_schedule(dict(steps=50, warmup_steps=[0], learning_rate_alpha=1.0, learning_rate=[3e-6]))
    assert all(_close(s(step), 3e-6) for step in (0, 1, 7, 49, 50, 1000))
    two = learning_rate_schedule(dict(steps=100, warmup_steps=[10, 30], learning_rate=[3e-4, 6e-5], learning_rate_alpha=0.1))
    for step, want in ((0, 0.0), (5, 1.5e-4), (9, 2.7e-4), (10, 0.0), (20, 3e-5), (29, 5.7e-5), (30, 6e-5), (100, 6e-6)):          # every stage restarts from 0
        assert _close(two(step), want), (step, two(step), want)
    empty = learning_rate_schedule(dict(steps=100, warmup_steps=[10, 10], learning_rate=[1.0, 2e-3], learning_rate_alpha=0.0))          # a stage of zero length
    assert _close(empty(9), 0.9) and _close(empty(10), 2e-3)
    obj = type("Args", (), dict(steps=100, warmup_steps=10, learning_rate=1e-3, learning_rate_alpha=0.1))()          # an object, not a mapping
    assert _close(learning_rate_schedule(obj)(5), 5e-4)
    for bad in (dict(steps=10, warmup_steps=10, learning_rate=1e-3), dict(steps=5, warmup_steps=[2, 10], learning_rate=[1e-3, 1e-3]),
                dict(steps=100, warmup_steps=[20, 10], learning_rate=[1e-3, 1e-3]), dict(steps=100, warmup_steps=[10, 20], learning_rate=[1e-3])):
        with pytest.raises(ValueError):
            learning_rate_schedule(bad)


# ---- datasets -------------------------------------------------------------------------------------------------------------------------------
def _golden(name):
    with gzip.open(os.path.join(GOLDEN, name)) as f:
        return json.loads(f.read().decode("utf-8"))


def test_train_dataset_equals_the_reference_s_batches():
    g = _golden("dataset_train.json.gz")
    assert len(g["cases"]) == 6 and {(c["case"]["do_sequence_packing"], c["case"]["eos_token"]) for c in g["cases"]} >= {(True, None), (True, "</s>"), (False, None), (False, "</s>")}
    for c in g["cases"]:
        k = c["case"]
        ds = TrainDataset(k["langs"], os.path.join(GOLDEN, "dataset"), np.array(k["probs"]), g["batch_size"], g["block_size"], do_sequence_packing=k["do_sequence_packing"],
                          eos_token=k["eos_token"])
        it = iter(ds)
        got = [next(it) for _ in range(len(c["batches"]))]
        assert len(got) == 6 and got == c["batches"], k
        assert got[0]["lang_code"] == ("all" if len(k["langs"]) > 1 else k["langs"][0])
        first = {lang: np.random.RandomState(0).permutation(len(ds.dataset[lang])) for lang in k["langs"]}
        assert any(not np.array_equal(first[lang], ds.language_orders[lang]) for lang in k["langs"]), "the recorded batches cross a reshuffle"
        assert ds.get_texts(5) == c["get_texts_5"] and ds.get_texts_in_each_language(3) == c["in_each_language_3"]
        assert [next(iter(ds)) for _ in range(2)] == [c["batches"][0]] * 2          # every iteration starts over


def test_valid_dataset_equals_the_reference_s_items():
    g = _golden("dataset_valid.json.gz")
    for c in g["cases"]:
        k = c["case"]
        ds = ValidDataset(k["langs"], os.path.join(GOLDEN, "dataset"), k["n_subsample"], k["batch_size"])
        assert len(ds) == c["len"] > 0 and [ds[i] for i in range(len(ds))] == c["items"], k
        assert list(ds) == c["items"]          # the sequence protocol ends at len()
    with pytest.raises(ValueError, match="zz"):
        ValidDataset(["zz"], os.path.join(GOLDEN, "dataset"), None, 4)


# ---- aggregation ----------------------------------------------------------------------------------------------------------------------------
def test_window_aggregation():
    records = [{"identity_loss": 4.0, "learning_rate": 0.0, "grad_norm": 2.0, "skipped": 0.0},
               {"loss": 1.0, "lexical_loss": 0.5, "learning_rate": 1e-3, "avg_byte_length": 3.0, "unk_ratio": 0.0, "pad_ratio": 0.25},
               {"loss": 3.0, "lexical_loss": 1.5, "learning_rate": 2e-3, "grad_norm": 4.0, "skipped": 1.0, "avg_byte_length": 5.0, "unk_ratio": 0.5, "pad_ratio": 0.75},
               {"loss": 8.0, "lexical_loss": 1.0, "learning_rate": 3e-3, "avg_byte_length": 2.0, "unk_ratio": 0.25, "pad_ratio": 0.0}]
    got = aggregate_window(records, [0, 1, 1, 2], ["de", "en", "fr", "sw"], 12.5)
    want = {"identity_loss": 4.0, "loss": 4.0, "lexical_loss": 1.0, "learning_rate": 1.5e-3, "grad_norm": 3.0, "skipped": 0.5, "time": 12.5,
            "de_loss": math.nan, "en_loss": 2.0, "fr_loss": 8.0, "sw_loss": math.nan,
            "en_avg_byte_length": 4.0, "en_std_byte_length": 1.0, "en_unk_ratio": 0.25, "en_pad_ratio": 0.5,
            "fr_avg_byte_length": 2.0, "fr_std_byte_length": 0.0, "fr_unk_ratio": 0.25, "fr_pad_ratio": 0.0}
    assert set(got) == {"train/" + k for k in want}
    for k, v in want.items():
        assert (math.isnan(v) and math.isnan(got["train/" + k])) or math.isclose(got["train/" + k], v, rel_tol=1e-12), (k, got["train/" + k], v)
    only_identity = aggregate_window(records[:1], [0], ["de"], 1.0)
    assert set(only_identity) == {"train/identity_loss", "train/learning_rate", "train/grad_norm", "train/skipped", "train/time"}          # no loss: no per-language loss


def test_eval_aggregation():
    records = [{"loss": 2.0, "bpb": 1.0, "avg_byte_length": 4.0, "unk_ratio": 0.0}, {"loss": 4.0, "bpb": 3.0, "avg_byte_length": 8.0, "unk_ratio": 0.5},
               {"loss": 10.0, "bpb": 5.0, "avg_byte_length": 1.0, "unk_ratio": 0.125}]
    got = aggregate_eval(records, [1, 1, 0], ["de", "en", "fr"], "main")
    want = {"en_loss": 3.0, "en_bpb": 2.0, "de_loss": 10.0, "de_bpb": 5.0, "en_avg_byte_length": 6.0, "en_std_byte_length": 2.0, "en_unk_ratio": 0.25,
            "de_avg_byte_length": 1.0, "de_std_byte_length": 0.0, "de_unk_ratio": 0.125}
    assert got == {"eval/main_" + k: v for k, v in want.items()}          # nothing for "fr", which has no batch


# ---- draws ----------------------------------------------------------------------------------------------------------------------------------
def test_loader_draw_is_a_pure_function_of_seed_and_micro_step():
    probs = [0.2, 0.5, 0.3]
    a = [loader_draw(42, m, probs) for m in range(400)]
    assert a == [loader_draw(42, m, probs) for m in range(400)] and a[::-1] == [loader_draw(42, m, probs) for m in reversed(range(400))]          # in any order
    assert a != [loader_draw(43, m, probs) for m in range(400)] and set(a) == {0, 1, 2}
    counts = np.bincount(a, minlength=3) / 400.0
    assert np.abs(counts - probs).max() < 0.1          # (binomial std at n = 400 is 0.025)
    assert all(loader_draw(7, m, [1.0]) == 0 for m in range(20)) and all(loader_draw(7, m, [0.0, 2.0]) == 1 for m in range(20))          # unnormalised weights
    assert item_seed(3, 5) == item_seed(3, 5) and len({item_seed(s, i) for s in range(8) for i in range(8)}) == 64 and 0 <= item_seed(2 ** 63, 9) < 2 ** 64


# ---- config parsing -------------------------------------------------------------------------------------------------------------------------
# The key sets of the reference's configs/zeroshot/*.json, copied as data (the files themselves do not travel with this repository): every key
# any of them has, with one of the values it has there, and per group of files the keys it lacks.
VALUES = dict(adam_beta2=0.95, add_target_priors_to_bias=False, dataloader_num_workers=64, debug=False, do_tokenizer_sampling=True, dtype="bfloat16", eval_batch_size=128,
              eval_steps=10000, extra_lang_codes=["en", "python"], extra_valid_files=["valid/en.parquet", "valid/python.parquet"],
              extra_valid_tokenizer_names=["artifacts/tokenizers/en_raw", "artifacts/tokenizers/starcoder0001"], gradient_accumulation_steps=1, hn_add_inter_token_attention=False,
              hn_embed_lang_id=True, hn_embed_target_priors=False, hn_embed_using_source_embeddings=True, hn_hidden_size=768, hn_inter_token_attention_bias_by_priors=False,
              hn_intermediate_size=1536, hn_model_name_or_path="roberta-base", hn_num_attention_heads=32, hn_rescale_embeddings=True, hn_surface_maxlen=7,
              identity_n_subsample=16384, identity_steps=10000, init_from_params="benjamin/zett-hypernetwork-Mistral-7B-v0.1", langs="en", language_sampling_alpha=0.1,
              learnable_bias=False, learning_rate=[3e-4, 6e-5], lexical_loss_weight=0.5, loss="clm", max_grad_norm=0.1, mix_languages=False, model_name_or_path="gpt2", n_embd=768,
              n_token_subsample=None, n_valid_subsample=8192, output_dir="output_gpt2", random_warmup_steps=0, resume_from_checkpoint="output2", revision="refs/pr/129",
              steps=200000, tokenizer_batch_size=2048, tokenizer_name="artifacts/tokenizers/gpt20001", tokenizer_noise_mean=1e-5, tokenizer_noise_std=4, tokenizer_sample_max=32768,
              tokenizer_sample_mean=32768, tokenizer_sample_std=0, train_batch_size=128, train_directory="train", use_unigram_bias=True, valid_directory="valid",
              warmup_steps=[10000, 20000], weight_decay=0.01)
LACKS = {"gpt2*": ("eval_steps", "hn_embed_lang_id", "hn_num_attention_heads", "init_from_params", "language_sampling_alpha", "mix_languages", "resume_from_checkpoint", "revision"),
         "llama3-8b_en+code, mistral7b_en+code": ("hn_embed_lang_id", "init_from_params", "language_sampling_alpha", "resume_from_checkpoint", "tokenizer_name"),
         "llama3-8b_en+code_resume": ("hn_embed_lang_id", "init_from_params", "language_sampling_alpha", "tokenizer_name"),
         "mistral7b_multilingual": ("eval_steps", "language_sampling_alpha", "resume_from_checkpoint", "tokenizer_name"),
         "tinyllama_en+code": ("eval_steps", "hn_embed_lang_id", "hn_num_attention_heads", "init_from_params", "language_sampling_alpha", "resume_from_checkpoint", "tokenizer_name"),
         "tinyllama_multilingual": ("eval_steps", "hn_num_attention_heads", "language_sampling_alpha", "resume_from_checkpoint", "tokenizer_name"),
         "xlmr_multilingual": ("eval_steps", "hn_num_attention_heads", "init_from_params", "resume_from_checkpoint", "revision", "tokenizer_name")}
N_KEYS = {"gpt2*": 48, "llama3-8b_en+code, mistral7b_en+code": 51, "llama3-8b_en+code_resume": 52, "mistral7b_multilingual": 52, "tinyllama_en+code": 49,
          "tinyllama_multilingual": 51, "xlmr_multilingual": 50}
COMMON = {k: v for k, v in VALUES.items() if k not in LACKS["gpt2*"]}


@pytest.mark.parametrize("name", LACKS)
def test_config_key_sets_parse(name):
    cfg = {k: v for k, v in VALUES.items() if k not in LACKS[name]}
    assert len(VALUES) == 56 and len(cfg) == N_KEYS[name]
    model_args, data_args, training_args, hn_args = parse_config(dict(cfg, an_unknown_key=1))          # unknown keys are ignored
    groups = (model_args, data_args, training_args, hn_args)
    for key, value in cfg.items():
        holders = [g for g in groups if hasattr(g, key)]
        assert len(holders) == 1 and getattr(holders[0], key) == value, key
    assert training_args.adam_beta1 == 0.9 and training_args.logging_steps == 500 and training_args.save_state is True and data_args.block_size == 128          # defaults
    assert data_args.pad_to_multiple_of == 128 and data_args.n_pools == 1 and hn_args.hn_n_layers == 3 and hn_args.hn_predict_bias is True and model_args.config_name is None
    assert ("eval_steps" in cfg) or training_args.eval_steps == 10000
    learning_rate_schedule(training_args)(0)          # the list-valued fields reach the schedule as they are


def test_config_file_and_missing_required_key(tmp_path):
    path = tmp_path / "cfg.json"
    path.write_text(json.dumps(COMMON))
    assert parse_config(str(path))[2].steps == 200000
    with pytest.raises((ValueError, TypeError)):
        parse_config({k: v for k, v in COMMON.items() if k != "output_dir"})


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------
def _trainer(**fields):
    args = dict(steps=10, warmup_steps=2, learning_rate=1e-3, **fields)
    return HypernetTrainer(object(), lambda x, m: x, None, args, hn_pad_token_id=1, optimizer=object())


@pytest.mark.parametrize("field,value", (("backbone_training", "full"), ("apply_lexical_loss_to_init", True), ("run_backbone_in_training_mode", True),
                                         ("do_cost_analysis", True), ("mix_languages", True)))
def test_refused_fields_name_themselves(field, value):
    with pytest.raises(NotImplementedError, match=field):
        _trainer(**{field: value})


@pytest.mark.parametrize("fields", (dict(gradient_accumulation_steps=0), dict(logging_steps=0), dict(loss="span")))
def test_value_errors(fields):
    with pytest.raises(ValueError, match=next(iter(fields))):
        _trainer(**fields)
    assert _trainer().micro_step == 0          # and the plain arguments construct
