"""Loader of the lexical-transfer fixtures (tests/golden/lexical_*.json.gz|npz, made by tests/golden/make_golden_lexical.py)."""
import gzip
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("unigram", "bpe")          # tied RoBERTa with 60 rows fewer than the tokenizer; untied GPT-NeoX with 24 rows more
MODES = ("no", "fvt", "bfvt")
MAX_EXACT_N = 16                    # torch's CPU mean(0) adds in order up to 16 rows: such rows are bit-identical to the reference


def load(name):
    with gzip.open(os.path.join(GOLDEN, f"lexical_{name}.json.gz"), "rt", encoding="utf-8") as f:
        meta = json.load(f)
    src = np.load(os.path.join(GOLDEN, f"lexical_{name}_source.npz"))
    meta["source_in"] = src["source_in"]
    meta["source_out"] = src["source_out"] if "source_out" in src.files else None
    meta["S"] = meta["source_in"] if meta["source_out"] is None else np.concatenate([meta["source_in"], meta["source_out"]], axis=1)
    return meta


def expected(name, key):
    """(expected_in, expected_out or None) the reference script saved for run `key` ("no", "fvt", "bfvt", "fvt_random")."""
    g = np.load(os.path.join(GOLDEN, f"lexical_{name}_{key}.npz"))
    return g["expected_in"], (g["expected_out"] if "expected_out" in g.files else None)


def expected_cat(name, key):
    e_in, e_out = expected(name, key)
    return e_in if e_out is None else np.concatenate([e_in, e_out], axis=1)


def assert_rows_match(got, want, id_lists, S, what):
    """Rows with n <= 16 constituents: bit-identical.  Rows with n > 16: |got - ref| <= 2 n 2^-24 mean_k |S[ids_k, c]| per element
    (worst-case reordering error of an fp32 sum of n terms on each side; the division's half ulp absorbed by the factor 2).
    No row is left out."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    n = np.array([len(ids) for ids in id_lists])
    short = n <= MAX_EXACT_N
    bad = np.flatnonzero(short & (got.view(np.uint32) != want.view(np.uint32)).any(axis=1))
    assert len(bad) == 0, f"{what}: {len(bad)} rows with n <= {MAX_EXACT_N} differ from the reference, first {bad[:5]} (n = {n[bad[:5]]})"
    for r in np.flatnonzero(~short):
        bound = 2.0 * n[r] * 2.0 ** -24 * np.abs(S[id_lists[r]].astype(np.float64)).mean(axis=0)
        err = np.abs(got[r].astype(np.float64) - want[r].astype(np.float64))
        assert (err <= bound).all(), f"{what}: row {r} (n = {n[r]}) exceeds the reordering bound by {float((err - bound).max()):.3e}"
