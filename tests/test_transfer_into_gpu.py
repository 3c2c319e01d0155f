"""GPU: predict_vocabulary's direct path (one process, no --sample_batches: every batch stores its rows straight into the [V, E]
results with zett_forward_into) against the accumulating path (ZETT_DIRECT_OUT=0): the same tensors, bit for bit up to the sign
of zero (index_add_ into zeros turns -0.0 into +0.0), and no index_add_ at all."""
import numpy as np
import pytest
import torch

from tests import util
from zett_amd import synth

pytestmark = pytest.mark.gpu


def _run(model, sfm, src, lang, env, monkeypatch, **kw):
    from zett_amd.transfer import Args, predict_vocabulary
    monkeypatch.setenv("ZETT_DIRECT_OUT", env)
    calls = {"n": 0}
    real = torch.Tensor.index_add_

    def counting(self, *a, **k):
        calls["n"] += 1
        return real(self, *a, **k)

    monkeypatch.setattr(torch.Tensor, "index_add_", counting)
    out = predict_vocabulary(model, sfm, src, lang, Args(output="", batch_size=96), rng=np.random.default_rng(5), **kw)
    monkeypatch.setattr(torch.Tensor, "index_add_", real)
    torch.cuda.synchronize()
    return out, calls["n"], predict_vocabulary.last_direct


@pytest.mark.parametrize("separate_out", [True, False], ids=["untied", "tied"])
@pytest.mark.parametrize("job_table", ["1", "0"])
def test_predict_vocabulary_direct_equals_accumulating(separate_out, job_table, monkeypatch):
    cfg, *_ = synth.workload("tiny")
    cfg = dict(cfg, n_embd=256, hn_hidden_size=512, hn_intermediate_size=1024, hn_num_attention_heads=8, separate_out_embeddings=separate_out)
    w = synth.make_weights(cfg, seed=91)
    src = torch.from_numpy(synth.make_source_embeddings(cfg, 91)).cuda()
    sfm = torch.from_numpy(synth.make_surface_forms(cfg, 333, seed=91, n_special=2)).cuda()        # 4 batches of 96, the last padded
    monkeypatch.setenv("ZETT_JOB_TABLE", job_table)
    model = util.hip_model(cfg, w, "f16")
    direct, n_direct, was_direct = _run(model, sfm, src, 2, "1", monkeypatch)
    assert was_direct and n_direct == 0
    old, n_old, was_direct = _run(model, sfm, src, 2, "0", monkeypatch)
    assert not was_direct and n_old > 0
    for a, b in zip(direct, old):
        if b is None:
            assert a is None
            continue
        assert torch.equal((a + 0.0).view(torch.int32), (b + 0.0).view(torch.int32))


def test_cli_direct_and_accumulating_save_identical_tensors(tmp_path):
    """scripts/transfer.py run once with ZETT_DIRECT_OUT=1 and once with =0 (tiny checkpoints of tests/test_transfer_gpu.py, a target
    vocabulary of 900 walked in batches of 256 with a padded last batch): the saved model and bias are the same tensors."""
    import os
    import subprocess
    import sys

    from safetensors.torch import load_file

    from tests.test_transfer_gpu import _cli_args, _make_checkpoints

    dirs, *_ = _make_checkpoints(tmp_path, "pt")
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = {}
    for flag in ("1", "0"):
        out = str(tmp_path / f"out_direct{flag}")
        res = subprocess.run([sys.executable, os.path.join(repo, "scripts", "transfer.py")] + _cli_args(dirs, out), cwd=repo,
                             env=dict(os.environ, ZETT_DIRECT_OUT=flag), capture_output=True, text=True, timeout=900)
        assert res.returncode == 0, res.stderr[-3000:]
        outs[flag] = (load_file(os.path.join(out, "model.safetensors")), load_file(os.path.join(out, "bias.safetensors")))
    (ma, ba), (mb, bb) = outs["1"], outs["0"]
    assert set(ma) == set(mb)
    for k in ma:
        assert torch.equal(ma[k], mb[k]), k
    assert torch.equal(ba["bias"], bb["bias"])
