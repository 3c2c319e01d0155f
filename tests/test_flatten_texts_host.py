"""``text_encode.flatten_texts`` against the plain definition: the texts' UTF-8 bytes end to end and the cumulative sum of their byte
lengths.  Pure numpy: no GPU, no library."""
import numpy as np
import pytest

from zett_amd.text_encode import flatten_texts

TWO, THREE, FOUR = "é", "€", "𝄞"          # 2, 3 and 4 bytes of UTF-8


def _random_texts():
    rng = np.random.default_rng(0)
    alphabet = list("ab z'\n09") + [TWO, "ß", THREE, "語", FOUR, "😀", "́", " "]
    return ["".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=rng.integers(0, 40))) for _ in range(1000)]


CASES = {
    "no texts": [],
    "one empty text": [""],
    "two empty texts": ["", ""],
    "ascii": ["hello world", " it's 12", "x"],
    "starts with 2, 3, 4 bytes": [TWO + "a", THREE + "bc", FOUR + " d"],
    "ends with 2, 3, 4 bytes": ["a" + TWO, "bc" + THREE, "d " + FOUR],
    "only wide characters": [TWO, THREE, FOUR, FOUR + THREE + TWO],
    "empty texts between": ["", "ab", "", "", THREE + "c", "", "d" + FOUR, ""],
    "1000 random texts": _random_texts(),
}


@pytest.mark.parametrize("name", list(CASES))
def test_flatten_texts_equals_the_plain_definition(name):
    texts = CASES[name]
    blob, offsets = flatten_texts(texts)
    want = np.zeros(len(texts) + 1, dtype=np.int64)
    np.cumsum([len(t.encode()) for t in texts], out=want[1:])
    assert isinstance(blob, bytes) and blob == b"".join(t.encode() for t in texts)
    assert isinstance(offsets, np.ndarray) and offsets.dtype == np.int64 and offsets.shape == (len(texts) + 1,)
    assert offsets[0] == 0 and offsets[-1] == len(blob)
    assert np.array_equal(offsets, want)
    assert all(blob[offsets[i]:offsets[i + 1]] == t.encode() for i, t in enumerate(texts))
    again, offsets2 = flatten_texts(texts, "".join(texts))          # the joined text, where the caller has it already
    assert again == blob and np.array_equal(offsets2, want)


def test_flatten_texts_imports_without_torch_at_module_level():
    import sys

    import zett_amd.text_encode as te
    assert "torch" not in te.__dict__ and "torch" not in sys.modules["zett_amd._glue"].__dict__
