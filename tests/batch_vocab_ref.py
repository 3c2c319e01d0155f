"""What zett_amd.training.subsample_batch_vocabulary is held to (tests/test_batch_vocab_host.py, tests/test_batch_vocab_gpu.py): the
numpy restatement of its definition — the n_token_subsample branch of the reference's collator (collator.py:207-282) with the two
deviations of the docstring — the literal list form of the specials' moves, and the input recipe both files share.

THE DEFINITION.  positives: ascending, the ids of input_ids and of labels != -100 that are not special.  pre-list = special_ids (list order)
++ positives ++ negatives ("positives_only": id 0 repeated; "random": the first entries of negative_order that are not in the list so
far).  For each special id ascending: ``del list[list.index(id)]; list.insert(id, id)``.  inv[list] = arange (the last write wins)."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("batch_vocab_clm_random", "batch_vocab_clm_positives_only", "batch_vocab_mlm_random", "batch_vocab_absent_special_random")
OUTPUTS = ("input_ids", "labels", "ids_to_embed", "target_surface_forms", "target_priors", "mask", "special_indices")


def moves_by_list(special_ids, n):
    """(final list of a pre-list whose other entries are -1 - row, special_indices) by Python's own del / insert"""
    lst = list(special_ids) + [-1 - r for r in range(len(special_ids), n)]
    for s in sorted(special_ids):
        del lst[lst.index(s)]
        lst.insert(s, s)
    return lst, [lst.index(s) for s in special_ids]


def batch_vocab_ref(input_ids, labels, special_ids, n, surface_forms, priors, mode="random", negative_order=None):
    """numpy in, dict of numpy out (the members of BatchVocabulary; special_indices a list, n_positive an int)."""
    input_ids, labels = np.asarray(input_ids), np.asarray(labels)
    special = np.asarray(list(special_ids), dtype=np.int64)
    v = len(priors)
    seen = np.concatenate([input_ids.reshape(-1), labels.reshape(-1)[labels.reshape(-1) != -100]]).astype(np.int64)
    assert ((seen >= 0) & (seen < v)).all() and n <= v
    tokens_in_batch = np.concatenate([special, np.setdiff1d(np.unique(seen), special)])
    n_positive = len(tokens_in_batch)
    assert n_positive <= n
    k = n - n_positive
    if mode == "positives_only":
        negatives = np.zeros(k, dtype=np.int64)
    else:
        order = np.asarray(negative_order).astype(np.int64)
        negatives = order[~np.isin(order, tokens_in_batch)][:k]
        assert len(negatives) == k
    lst = [int(x) for x in np.concatenate([tokens_in_batch, negatives])]
    for s in sorted(int(x) for x in special):
        del lst[lst.index(s)]
        lst.insert(s, s)
    ids_to_embed = np.array(lst, dtype=np.int64)
    inv = np.zeros(v, dtype=np.int64)
    inv[ids_to_embed] = np.arange(n)
    return {
        "input_ids": inv[input_ids].astype(input_ids.dtype),
        "labels": np.where(labels != -100, inv[np.where(labels != -100, labels, 0)], -100).astype(labels.dtype),
        "ids_to_embed": ids_to_embed.astype(input_ids.dtype),
        "target_surface_forms": np.asarray(surface_forms)[ids_to_embed],
        "target_priors": np.asarray(priors)[ids_to_embed],
        "mask": np.ones(n, dtype=bool),
        "special_indices": [lst.index(int(s)) for s in special],
        "n_positive": n_positive,
    }


def load_fixture(name):
    """A fixture of tests/golden/make_golden_batch_vocab.py: (inputs, what the reference's Collator.encode returned)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    inputs = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    inputs["mode"] = str(inputs["mode"])
    inputs["n"] = int(inputs["n"])
    inputs["special_ids"] = [int(x) for x in inputs["special_ids"]]
    expected = {k[4:]: z[k] for k in z.files if k.startswith("out_")}
    return inputs, expected


def blank_labels(inputs):
    """labels with -100 wherever the label's id still occurs elsewhere: most of them, and the set of ids of the batch is unchanged"""
    ids, labels = inputs["input_ids"], inputs["labels"].copy()
    flat = labels.reshape(-1)
    for p in range(flat.size):
        rest = np.concatenate([ids.reshape(-1), flat[:p], flat[p + 1:]])
        if flat[p] in rest:
            flat[p] = -100
    return labels


@functools.lru_cache(maxsize=None)
def recipe(v, t, l, special=(0,), seed=0, label_only=2):
    """(input_ids int64 [T], labels int64 [T], surface_forms int64 [V, L], priors fp32 [V], negative_order int64 [V]) of a case: Zipf-like
    ids, clm labels with a few of them -100 and `label_only` ids that occur in the labels alone.  Shared between tests: read-only."""
    rng = np.random.default_rng(1000 * seed + v + t)
    ids = np.minimum(np.floor(v * rng.random(t) ** 3).astype(np.int64), v - 1)
    labels = ids.copy()
    if t >= 8:
        labels[rng.choice(t, t // 8, replace=False)] = -100
        for j in range(label_only):
            labels[(j * 3 + 1) % t] = v - 2 - j
    sf = rng.integers(0, 1 << 20, (v, l)).astype(np.int64)
    priors = rng.standard_normal(v).astype(np.float32)
    order = rng.permutation(v).astype(np.int64)
    for a in (ids, labels, sf, priors, order):
        a.setflags(write=False)
    return ids, labels, sf, priors, order
