"""Writes the dataset fixtures of tests/test_trainer_host.py: two tiny parquet tables (dataset/aa.parquet, dataset/bb.parquet: short rows, some
empty, some only whitespace) and what the reference's own ``TrainDataset`` / ``ValidDataset`` (zett/dataset.py) yield for them, as
dataset_train.json.gz and dataset_valid.json.gz.

    python tests/golden/make_golden_dataset.py PATH_TO_REFERENCE_CHECKOUT

Runs only next to a checkout of the reference, with ``jax`` and the other absent libraries stubbed the way make_golden_retok.py does.  Every
recorded TrainDataset case is checked to reshuffle at least one language inside its six batches."""
import gzip
import json
import os
import sys
from unittest.mock import MagicMock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DATA = os.path.join(HERE, "dataset")
LANGS = ["aa", "bb"]
N_BATCHES, BATCH_SIZE, BLOCK_SIZE = 6, 4, 2          # block_size 2: texts are packed up to 32 characters
TRAIN_CASES = [dict(langs=LANGS, probs=[0.3, 0.7], do_sequence_packing=packing, eos_token=eos) for packing in (True, False) for eos in (None, "</s>")]
TRAIN_CASES += [dict(langs=["bb"], probs=[1.0], do_sequence_packing=True, eos_token="</s>"), dict(langs=["bb"], probs=[1.0], do_sequence_packing=False, eos_token=None)]
VALID_CASES = [dict(langs=LANGS, n_subsample=None, batch_size=4), dict(langs=LANGS, n_subsample=10, batch_size=4), dict(langs=["bb", "aa"], n_subsample=7, batch_size=3)]


def rows(lang: str, n: int):
    rng = np.random.RandomState(len(lang) + n)
    words = ["alpha", "beta", "gamma", "delta", "tokens", "of", "text", "zett", "übung", "naïve", "日本", "x"]
    out = []
    for i in range(n):
        if i % 7 == 3:
            out.append("")
        elif i % 7 == 5:
            out.append(" \t\n ")
        else:
            text = " ".join(words[j] for j in rng.randint(0, len(words), size=rng.randint(1, 4)))
            out.append(f"  {lang}{i} {text} " if i % 4 == 0 else f"{lang}{i} {text}")
    return out


def write_tables():
    import pyarrow as pa
    import pyarrow.parquet as pq
    os.makedirs(DATA, exist_ok=True)
    for lang, n in (("aa", 30), ("bb", 9)):
        pq.write_table(pa.table({"text": rows(lang, n)}), os.path.join(DATA, f"{lang}.parquet"))


def main():
    reference = sys.argv[1]
    os.environ["HF_DATASETS_OFFLINE"] = "1"
    import datasets  # noqa: F401  (before the stubs: it probes for a real jax)
    for name in ("jax", "jax.numpy", "jax.sharding", "jax.experimental", "jax.experimental.multihost_utils", "flax", "flax.core", "flax.core.frozen_dict",
                 "flax.traverse_util", "flax.serialization", "flax.training", "flax.training.common_utils", "flax.training.train_state", "optax", "h5py",
                 "jax.experimental.pjit", "jax.tree_util", "flax.linen"):
        sys.modules.setdefault(name, MagicMock())
    sys.path.insert(0, reference)
    os.environ["HF_DATASETS_OFFLINE"] = "1"
    from zett.dataset import TrainDataset, ValidDataset
    write_tables()
    train = []
    for case in TRAIN_CASES:
        ds = TrainDataset(case["langs"], DATA, np.array(case["probs"]), BATCH_SIZE, BLOCK_SIZE, do_sequence_packing=case["do_sequence_packing"], eos_token=case["eos_token"])
        batches = []
        for batch in ds:
            batches.append({"texts": [str(t) for t in batch["texts"]], "lang_code": str(batch["lang_code"])})
            if len(batches) == N_BATCHES:
                break
        first = {lang: np.random.RandomState(0).permutation(len(ds.dataset[lang])) for lang in case["langs"]}
        assert any(not np.array_equal(first[lang], ds.language_orders[lang]) for lang in case["langs"]), ("no reshuffle", case)
        train.append({"case": case, "batches": batches, "get_texts_5": [str(t) for t in ds.get_texts(5)],
                      "in_each_language_3": {k: [str(t) for t in v] for k, v in ds.get_texts_in_each_language(3).items()}})
    valid = []
    for case in VALID_CASES:
        ds = ValidDataset(case["langs"], DATA, case["n_subsample"], case["batch_size"])
        valid.append({"case": case, "len": len(ds), "items": [{"texts": [str(t) for t in ds[i]["texts"]], "lang_code": str(ds[i]["lang_code"])} for i in range(len(ds))]})
    for name, what in (("dataset_train.json.gz", {"batch_size": BATCH_SIZE, "block_size": BLOCK_SIZE, "cases": train}), ("dataset_valid.json.gz", {"cases": valid})):
        with gzip.GzipFile(os.path.join(HERE, name), "wb", mtime=0) as f:
            f.write(json.dumps(what, ensure_ascii=False, indent=0).encode("utf-8"))
    print("wrote", len(train), "train cases and", len(valid), "valid cases")


if __name__ == "__main__":
    main()
