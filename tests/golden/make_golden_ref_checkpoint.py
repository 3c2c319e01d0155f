"""Checkpoint fixtures: what the reference's own torch class (hf_hypernet) writes with save_pretrained.

    python tests/golden/make_golden_ref_checkpoint.py REFERENCE_DIR

The "tiny" hypernet with synth.make_weights(cfg, 5) and (auto-class registration on) synth.make_weights(cfg, 8) is
saved by the reference; kept here are the two config.json files verbatim and, instead of the 2.8 MB weights
file, its safetensors header and sha256.  The weights are synth.make_weights, so tests/test_host_logic.py
rebuilds model.safetensors from header + weights and checks the digest: the checkpoint under test is
byte for byte the one the reference wrote.  The modeling / configuration modules that save_pretrained copies
next to an auto-class checkpoint are the reference's program text and are not kept (install_remote_code
replaces them anyway).  The backbone config lives at the relative path "rb", which no test resolves:
it holds the roberta-base values our loader falls back to.
"""
from __future__ import annotations

import hashlib
import json
import os
import shutil
import struct
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "ref_checkpoint")

_SAVE = """
import sys, json, torch, os
sys.path.insert(0, {reference!r}); sys.path.insert(0, {repo!r})
from hf_hypernet.configuration_hypernet import ZettHypernetConfig
from hf_hypernet.modeling_hypernet import ZettHypernet
from zett_amd import synth
os.makedirs("rb")
json.dump({{"model_type": "roberta", "max_position_embeddings": 514, "type_vocab_size": 1, "layer_norm_eps": 1e-5,
           "hidden_act": "gelu", "vocab_size": 50265, "pad_token_id": 1}}, open(os.path.join("rb", "config.json"), "w"))
cfg, *_ = synth.workload("tiny")
if {auto!r}:
    ZettHypernetConfig.register_for_auto_class()
    ZettHypernet.register_for_auto_class("AutoModel")
m = ZettHypernet(ZettHypernetConfig(**dict(cfg, hn_model_name_or_path="rb")))
m.load_state_dict({{k: torch.from_numpy(v) for k, v in synth.make_weights(cfg, {seed}).items()}})
m.save_pretrained("ckpt")
"""


def main(reference: str) -> None:
    os.makedirs(OUT, exist_ok=True)
    header, digests = None, {}
    for seed, auto, name in ((5, False, "config.json"), (8, True, "config_auto_map.json")):
        work = tempfile.mkdtemp(prefix="zett_refckpt_")
        try:
            subprocess.run([sys.executable, "-c", _SAVE.format(reference=reference, repo=REPO, auto=auto, seed=seed)], check=True, cwd=work)
            shutil.copyfile(os.path.join(work, "ckpt", "config.json"), os.path.join(OUT, name))
            blob = open(os.path.join(work, "ckpt", "model.safetensors"), "rb").read()
        finally:
            shutil.rmtree(work, ignore_errors=True)
        n = struct.unpack("<Q", blob[:8])[0]
        hdr = blob[8:8 + n].decode()
        assert header in (None, hdr), "the two checkpoints have different layouts"
        header = hdr
        digests[str(seed)] = {"sha256": hashlib.sha256(blob).hexdigest(), "size": len(blob)}
    with open(os.path.join(OUT, "model_safetensors.json"), "w") as f:
        json.dump({"header": header, "by_seed": digests}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    main(sys.argv[1])
