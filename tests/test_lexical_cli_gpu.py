"""scripts/transfer_lexical.py end to end on tiny local model directories (no network), built the way the lexical fixtures'
generator builds its two cases: a Unigram / Metaspace source with a tied RoBERTa whose matrix has FEWER rows than the tokenizer,
and a byte-fallback BPE source with an untied GPT-NeoX whose matrices have MORE rows.  The written embedding matrices are
compared with the CPU restatement (tests/lexical_ref.py — pinned bit for bit to the reference script's own output by
tests/test_lexical_oracle.py) on the same converted tokenizers.  Only files and return codes are asserted on."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import lexical_cases as lc
from tests import lexical_ref

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "golden"))


def _lines(seed):
    import glob
    import random
    rng = random.Random(seed)
    files = sorted(glob.glob(os.path.join(os.path.dirname(os.__file__), "*.py")))
    rng.shuffle(files)
    out = []
    for f in files[:25]:
        out += [ln.strip() for ln in open(f, encoding="utf-8", errors="ignore") if len(ln.strip()) > 20]
    rng.shuffle(out)
    return out[:3000]


def _make_dirs(tmp_path, kind):
    import make_golden_retok as mgr          # the trainers of the fixtures (no reference import at module level)
    from transformers import GPTNeoXConfig, GPTNeoXForCausalLM, RobertaConfig, RobertaForMaskedLM

    from zett_amd.byte_level import convert_to_byte_level
    model_dir, tgt_dir = str(tmp_path / "model"), str(tmp_path / "target_tok")
    mgr.wrap(mgr.train_bytelevel_bpe(_lines(2), 900, ["<|endoftext|>"]), eos_token="<|endoftext|>").save_pretrained(tgt_dir)
    torch.manual_seed(3)
    if kind == "unigram":
        def make():
            return mgr.wrap(mgr.train_metaspace_unigram(_lines(1), 700), bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>")
        tok = make()
        rows = len(convert_to_byte_level(make())[0]) - 20
        model = RobertaForMaskedLM(RobertaConfig(vocab_size=rows, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                                                 max_position_embeddings=66, pad_token_id=tok.pad_token_id, bos_token_id=tok.bos_token_id,
                                                 eos_token_id=tok.eos_token_id, tie_word_embeddings=True))
        model_class = "AutoModelForMaskedLM"
    else:
        def make():
            return mgr.wrap(mgr.train_mistral_like(_lines(1), 900), bos_token="<s>", eos_token="</s>", unk_token="<unk>")
        tok = make()
        rows = len(convert_to_byte_level(make())[0]) + 9
        model = GPTNeoXForCausalLM(GPTNeoXConfig(vocab_size=rows, hidden_size=32, num_hidden_layers=1, num_attention_heads=2, intermediate_size=64,
                                                 max_position_embeddings=64, bos_token_id=tok.bos_token_id, eos_token_id=tok.eos_token_id,
                                                 tie_word_embeddings=False))
        model_class = "AutoModelForCausalLM"
    tok.save_pretrained(model_dir)
    model.save_pretrained(model_dir)
    return model_dir, tgt_dir, model_class, model


def _expected(model_dir, tgt_dir, model, fvt_mode):
    from transformers import AutoTokenizer

    from zett_amd.byte_level import convert_to_byte_level
    source = convert_to_byte_level(AutoTokenizer.from_pretrained(model_dir))[0]
    target = convert_to_byte_level(AutoTokenizer.from_pretrained(tgt_dir), match_special_tokens_to=source, make_whitespace_consistent=True)[0]
    tokens = target.convert_ids_to_tokens(range(len(target)))
    s_in = model.get_input_embeddings().weight.detach().numpy()
    S = s_in if model.config.tie_word_embeddings else np.concatenate([s_in, model.get_output_embeddings().weight.detach().numpy()], axis=1)
    model_json = json.loads(source._tokenizer.to_str())["model"]
    want, overlap, id_lists = lexical_ref.transfer(model_json, source.get_vocab(), tokens, S, fvt_mode, source.unk_token_id)
    assert len(S) != len(source)
    return want, id_lists, S, len(tokens)


@pytest.mark.parametrize("kind,fvt_mode", [("unigram", "fvt"), ("bpe", "bfvt")])
def test_cli_end_to_end(tmp_path, kind, fvt_mode):
    import transformers
    model_dir, tgt_dir, model_class, model = _make_dirs(tmp_path, kind)
    out_dir = str(tmp_path / "out")
    env = dict(os.environ, HF_HUB_OFFLINE="1", TRANSFORMERS_OFFLINE="1")
    proc = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "transfer_lexical.py"), "--output", out_dir, "--tokenizer_name", tgt_dir,
                           "--model_name_or_path", model_dir, "--model_class", model_class, "--fvt_mode", fvt_mode],
                          env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    assert proc.returncode == 0
    for f in ("config.json", "tokenizer.json", "tokenizer_config.json"):
        assert os.path.exists(os.path.join(out_dir, f)), f
    want, id_lists, S, n_tokens = _expected(model_dir, tgt_dir, model, fvt_mode)
    new = getattr(transformers, model_class).from_pretrained(out_dir)
    assert new.config.vocab_size == n_tokens
    got_in = new.get_input_embeddings().weight.detach().numpy()
    assert got_in.shape == (n_tokens, 32)
    lc.assert_rows_match(got_in, want[:, :32], id_lists, S[:, :32], f"{kind} {fvt_mode} input embeddings")
    if not model.config.tie_word_embeddings:
        got_out = new.get_output_embeddings().weight.detach().numpy()
        lc.assert_rows_match(got_out, want[:, 32:], id_lists, S[:, 32:], f"{kind} {fvt_mode} output embeddings")
    assert any(len(ids) > 1 for ids in id_lists) and any(len(ids) == 1 for ids in id_lists)


def test_cli_other_ranks_do_nothing(tmp_path):
    """Under WORLD_SIZE > 1 every rank but 0 returns at once: no output directory, return code 0."""
    out_dir = str(tmp_path / "out")
    env = dict(os.environ, WORLD_SIZE="2", RANK="1", HF_HUB_OFFLINE="1")
    proc = subprocess.run([sys.executable, os.path.join(REPO, "scripts", "transfer_lexical.py"), "--output", out_dir, "--tokenizer_name", "nowhere",
                           "--model_name_or_path", "nowhere"], env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
    assert proc.returncode == 0 and not os.path.exists(out_dir)
