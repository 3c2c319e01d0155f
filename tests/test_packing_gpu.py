"""Sequence packing end to end on the GPU: ``TrainDataset(do_sequence_packing=True, eos_token=...)`` joins rows with the eos STRING, and
the collator's encoders split it out of the texts the way the library does (``DeviceTextEncoder(split_added_tokens=True)``) — a fixed
tokenizer gives the library's rows, a sampled one treats the string as text, as its host-built twin does, and ``scripts/train.py`` runs a
config that leaves ``do_sequence_packing`` at the reference's default."""
import json
import math
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import collate_ref as cr
from zett_amd.collate import MAX_CHARS_PER_TOKEN, DeviceCollator
from zett_amd.dataset import TrainDataset
from zett_amd.train_config import parse_config
from zett_amd.trainer import device_loader, item_seed

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(REPO, "tests", "golden", "dataset")
BLOCK, EOS = 24, "</s>"
WORDS = "the quick brown fox jumps over the lazy dog , it's 12 345 times . we'll see".split(" ")


def _args(**kw):
    base = dict(do_tokenizer_sampling=False, n_token_subsample=None, pad_to_multiple_of=8, subsample_mode="random", block_size=BLOCK, use_passthrough_hypernet=False,
                add_prefix_space=False, hn_surface_maxlen=7, sample_text_span=False, langs=["aa", "bb"], tokenizer_sample_max=1536, tokenizer_sample_min=1100,
                tokenizer_sample_mean=1200, tokenizer_sample_std=30, tokenizer_noise_mean=0.0, tokenizer_noise_std=0.0)
    return types.SimpleNamespace(**dict(base, **kw))


def _packed_batches(n=2):
    """the first batches of the packed golden dataset: 4 texts of at least 8 * 16 characters, rows joined with the eos string"""
    it = iter(TrainDataset(["aa"], DATA, np.array([1.0]), 4, 8, do_sequence_packing=True, eos_token=EOS))
    batches = [next(it) for _ in range(n)]
    for b in batches:
        assert b["lang_code"] == "aa" and len(b["texts"]) == 4 and all(EOS in t[:-len(EOS)] and not t.endswith(EOS) for t in b["texts"])
    return batches


def test_fixed_tokenizer_gives_the_rows_of_the_library():
    """The collator's tokenizer is what ``convert_to_byte_level`` rebuilds: whatever its backend's added tokens are (none with the installed
    transformers: the eos string is text), they are the spec's, and the rows are the library's."""
    c = DeviceCollator(cr.bpe_tokenizer(), cr.bpe_tokenizer(False), _args(), loss="clm", tokenizer=cr.bpe_tokenizer(), device=DEV)
    backend = json.loads(c.tokenizer._tokenizer.to_str())["added_tokens"]
    assert c.encoder.spec.split_added_tokens and [(a.content, a.id) for a in c.encoder.spec.added_tokens] == [(a["content"], a["id"]) for a in backend]
    for k, batch in enumerate(_packed_batches()):
        got = c([batch], seed=5 + k)
        texts = [t[:MAX_CHARS_PER_TOKEN * BLOCK] for t in batch["texts"]]
        want = c.tokenizer(texts, max_length=BLOCK, truncation=True, padding="max_length", return_tensors="np", add_special_tokens=True)
        ids = torch.from_numpy(want["input_ids"])
        assert torch.equal(got["input_ids"].cpu(), ids) and torch.equal(got["attention_mask"].cpu(), torch.from_numpy(want["attention_mask"]))
        assert got["lang_code"] == "aa" and int(got["lang_index"]) == 0
    c.encoder.close()


def test_tokenizer_whose_backend_holds_the_eos_token():
    """the test tokenizer as loaded: </s> and <mask> are added tokens of its backend, and every packed row holds eos ids inside"""
    from zett_amd.text_encode import DeviceTextEncoder
    tokenizer = cr.bpe_tokenizer()
    enc = DeviceTextEncoder.from_tokenizer(tokenizer, DEV, split_added_tokens=True)
    assert {EOS, "<mask>"} <= {a.content for a in enc.spec.added_tokens if enc.spec.is_plain(a)} and enc.spec.refused_strings == ()
    texts = [t for b in _packed_batches() for t in b["texts"]] + ["a<mask>b" + EOS, EOS + EOS, ""]
    for block in (BLOCK, 256):
        want = tokenizer(texts, max_length=block, truncation=True, padding="max_length", return_tensors="np", add_special_tokens=True)
        for dtype in (torch.int32, torch.int64):
            got = enc(texts, block, dtype=dtype)
            assert torch.equal(got["input_ids"].cpu(), torch.from_numpy(want["input_ids"]).to(dtype))
            assert torch.equal(got["attention_mask"].cpu(), torch.from_numpy(want["attention_mask"]).to(dtype))
        assert all(int((row[1:-1] == tokenizer.eos_token_id).sum()) >= 1 for row in want["input_ids"][:8]), "every packed row holds an eos id inside"
    with pytest.raises(NotImplementedError):
        DeviceTextEncoder.from_tokenizer(tokenizer, DEV)(texts, BLOCK)          # the default mode refuses as before
    enc.close()


def test_sampled_tokenizer_equals_its_host_built_twin():
    from zett_amd.tokenizer_sampling import DeviceTokenizerSampler, sample_tokenizer
    seed, reference, hn = 4, cr.bpe_tokenizer(), cr.bpe_tokenizer(False)
    batch = _packed_batches(1)[0]
    texts = [t[:MAX_CHARS_PER_TOKEN * BLOCK] for t in batch["texts"]]
    assert len(set(texts)) == len(texts)
    args = _args(do_tokenizer_sampling=True, add_prefix_space=True)
    host_sampler, sampler = (DeviceTokenizerSampler(table_capacity=1 << 14, max_depth=2, max_pieces=1 << 12) for _ in range(2))
    c = DeviceCollator(reference, hn, args, loss="clm", samplers={"aa": [sampler]}, device=DEV)
    got = c([batch], seed=seed)
    rng = np.random.default_rng(seed)
    assert int(rng.integers(0, 1)) == 0
    n_total = min(1536, max(1100, int(rng.normal(1200, 30))))
    tokenizer, special_ids_map, _, _, _ = sample_tokenizer(texts, host_sampler, reference, n_total=n_total, noise_std=0.0, add_prefix_space=True, hn_tokenizer=hn,
                                                           hn_surface_maxlen=7)
    enc = tokenizer(texts, max_length=BLOCK, truncation=True, padding="max_length", return_tensors="np", add_special_tokens=True)
    ids = enc["input_ids"].copy()
    for k, v in special_ids_map.items():
        ids[ids == k] = v
    assert torch.equal(got["input_ids"].cpu(), torch.from_numpy(ids)) and torch.equal(got["attention_mask"].cpu(), torch.from_numpy(enc["attention_mask"]))
    eos_at = int(special_ids_map.get(reference.eos_token_id, reference.eos_token_id))
    assert not (ids[:, 1:-1] == eos_at).any(), "a sampled tokenizer's backend has no added token: the eos string is text"
    host_sampler.close()
    sampler.close()
    c.vocabulary.close()


def _texts(seed, n=1):
    rng = np.random.default_rng(seed)
    return [" ".join(WORDS[i] for i in rng.integers(0, len(WORDS), size=int(rng.integers(8, 30)))) for _ in range(n)]


def test_cli_runs_a_config_with_packing_left_at_its_default(tmp_path):
    """The three updates of tests/test_trainer_gpu.py's CLI case without ``do_sequence_packing`` in the config; by hand: the two training
    batches of the run built from the same dataset, collator and seeds hold the library's rows, and the data metrics the CLI logged for
    them are theirs bit for bit."""
    import pyarrow as pa
    import pyarrow.parquet as pq
    from transformers import AutoTokenizer, GPT2Config, GPT2LMHeadModel
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
                  add_prefix_space=False, target_tokenizer_name=str(tmp_path / "model"), train_batch_size=4, eval_batch_size=4, block_size=32, n_token_subsample=256,
                  identity_n_subsample=256, pad_to_multiple_of=8, n_embd=64, hn_surface_maxlen=7, hn_n_layers=1, hn_hidden_size=64, hn_intermediate_size=128,
                  hn_num_attention_heads=2, hn_embed_using_source_embeddings=True, hn_rescale_embeddings=True, hn_embed_lang_id=True, hn_model_name_or_path=None,
                  lexical_loss_weight=0.5, max_grad_norm=0.1, dtype="float32", use_unigram_bias=True)
    (tmp_path / "cfg.json").write_text(json.dumps(config))
    model_args, data_args, training_args, hn_args = parse_config(str(tmp_path / "cfg.json"))
    assert data_args.do_sequence_packing is True
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
    # by hand: what main() builds for the data of the two training updates
    from zett_amd.byte_level import convert_to_byte_level
    import copy
    reference = AutoTokenizer.from_pretrained(str(tmp_path / "model"))
    data_args.hn_surface_maxlen, data_args.langs = hn_args.hn_surface_maxlen, ["en"]
    dataset = TrainDataset(["en"], data_args.train_directory, np.array([1.0]), training_args.train_batch_size, data_args.block_size, do_sequence_packing=True,
                           eos_token=reference.eos_token)
    collator = DeviceCollator(reference, convert_to_byte_level(copy.deepcopy(reference))[0], data_args, loss="clm", tokenizer=AutoTokenizer.from_pretrained(str(tmp_path / "model")),
                              device=DEV)
    loader = iter(device_loader(dataset, collator, seed=item_seed(int(training_args.seed), 1)))
    items = iter(dataset)
    for step, line in ((2, lines[1]), (3, lines[2])):
        batch, item = next(loader), next(items)
        assert all(EOS in t for t in item["texts"])
        assert line["train/en_avg_byte_length"] == float(batch["metrics"]["avg_byte_length"]) and line["train/en_unk_ratio"] == float(batch["metrics"]["unk_ratio"])
        assert line["train/en_pad_ratio"] == float((batch["attention_mask"] == 0).to(torch.float64).mean())
        rng = np.random.default_rng(item_seed(item_seed(int(training_args.seed), 1), step - 2) & 0xFFFFFFFFFFFFFFFF)
        texts = []
        for t in item["texts"]:
            start = int(rng.integers(0, max(len(t) - MAX_CHARS_PER_TOKEN * data_args.block_size, 0) + 1))
            texts.append(t[start:start + MAX_CHARS_PER_TOKEN * data_args.block_size])
        want = collator.tokenizer(texts, max_length=data_args.block_size, truncation=True, padding="max_length", return_tensors="np", add_special_tokens=True)
        assert torch.equal(batch["attention_mask"].cpu(), torch.from_numpy(want["attention_mask"]))
        ids = torch.from_numpy(want["input_ids"])
        sub = batch["ids_to_embed"].cpu()[batch["input_ids"].cpu().long()]          # rows of the step's sub-vocabulary back to the tokenizer's ids
        assert torch.equal(sub, ids)
    collator.encoder.close()
