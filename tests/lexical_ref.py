"""CPU restatement of the lexical (FVT / BFVT) transfer, for the tests (reference scripts/transfer_lexical.py:50-91).

Test infrastructure, not product: numpy and oracle.retok_ref only.  For each target token t (byte-level string), S the source
matrix of R rows (cat([in, out], 1) when untied):

  1. the row starts as the fallback: S[unk_token_id] ("unk"), or is left to the caller ("random": count 0);
  2. idx = vocab.get(t) — the WHOLE get_vocab() dictionary; if it exists and idx < R the row is S[idx];
  3. else, unless fvt_mode == "no": ids = tokenize(bare model, t) — no special-token matching;
       "fvt":  no id >= R and at least one id -> the mean of S[ids]; otherwise the fallback;
       "bfvt": ids >= R dropped; any left -> their mean; otherwise the fallback;
  4. overlap = rows set in 2 or 3.

THE MEAN (include/zett_hip.h): add the rows in ids order in fp32, then one IEEE division by float32(n).
"""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from oracle import retok_ref


def bare_model(model_json: dict) -> retok_ref.RetokModel:
    """The source tokenizer's model WITHOUT specials (step 3 never matches a special token by string)."""
    return retok_ref.model_from_tokenizer_json(model_json)


def plan(model: retok_ref.RetokModel, vocab: Dict[str, int], tokens: Sequence[str], n_source_rows: int, fvt_mode: str) -> List[List[int]]:
    """ids per token: [idx] for an exact match, the filtered decomposition otherwise, [] = fallback."""
    assert fvt_mode in ("no", "fvt", "bfvt")
    R = int(n_source_rows)
    out: List[List[int]] = []
    for t in tokens:
        idx = vocab.get(t)
        if idx is not None and idx < R:
            out.append([int(idx)])
            continue
        ids: List[int] = []
        if fvt_mode != "no":
            raw = retok_ref.token_to_bytes(t)          # KeyError on a character outside the byte table (the product's ZETT_E_KEY)
            ids = [int(i) for i in retok_ref.tokenize(model, raw)] if raw else []
            if fvt_mode == "fvt":
                ids = [] if any(i >= R for i in ids) else ids
            else:
                ids = [i for i in ids if i < R]
        out.append(ids)
    return out


def mean_rows(S: np.ndarray, ids: Sequence[int]) -> np.ndarray:
    """The product's definition of the mean: in-order fp32 sum, one division."""
    S = np.asarray(S, dtype=np.float32)
    acc = S[ids[0]].copy()
    for i in ids[1:]:
        acc = (acc + S[i]).astype(np.float32)
    return acc if len(ids) == 1 else (acc / np.float32(len(ids))).astype(np.float32)


def rows(S: np.ndarray, id_lists: Sequence[Sequence[int]], fallback_id: int, base: np.ndarray = None) -> Tuple[np.ndarray, int]:
    """fp32 [len(id_lists), D] and the overlap count.  fallback_id < 0: rows without constituents keep `base`'s values."""
    S = np.asarray(S, dtype=np.float32)
    out = np.zeros((len(id_lists), S.shape[1]), dtype=np.float32) if base is None else np.array(base, dtype=np.float32)
    overlap = 0
    for r, ids in enumerate(id_lists):
        if len(ids):
            out[r] = mean_rows(S, ids)
            overlap += 1
        elif fallback_id >= 0:
            out[r] = S[fallback_id]
    return out, overlap


def random_fallback(S: np.ndarray, n_rows: int, block: int = 128) -> np.ndarray:
    """fallback_mode="random" (transfer_lexical.py:52-57) drawn in row blocks from numpy's GLOBAL generator: the same stream as
    the reference's single (n_rows, D) draw.  loc / scale are torch's CPU mean(0) / std(0), as in the reference."""
    import torch
    St = torch.from_numpy(np.ascontiguousarray(S))
    loc, scale = St.mean(0), St.std(0)
    out = np.empty((n_rows, S.shape[1]), dtype=np.float64)
    for r0 in range(0, n_rows, block):
        r1 = min(n_rows, r0 + block)
        out[r0:r1] = np.random.normal(loc=loc, scale=scale, size=(r1 - r0, S.shape[1]))
    return out


def transfer(model_json: dict, vocab: Dict[str, int], tokens: Sequence[str], S: np.ndarray, fvt_mode: str, unk_token_id: int,
             fallback_mode: str = "unk"):
    """The whole of steps 1-4: (fp32 matrix, overlap count, id lists)."""
    id_lists = plan(bare_model(model_json), vocab, tokens, len(S), fvt_mode)
    if fallback_mode == "random":
        base = random_fallback(S, len(tokens)).astype(np.float32)
        out, overlap = rows(S, id_lists, -1, base)
    else:
        out, overlap = rows(S, id_lists, unk_token_id)
    return out, overlap, id_lists
