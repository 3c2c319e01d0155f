"""The reference's datasets (zett/dataset.py): ``TrainDataset``, an endless stream of ``{"texts": [batch_size strings], "lang_code"}`` packed
from per-language text tables, and ``ValidDataset``, the fixed batches of the validation tables.  Constructor arguments, iteration order and
yielded dicts are the reference's, so a run here sees the texts a run there sees; always one reader (``worker_idx = 0`` of one worker).

A language's table is the directory ``{directory}/{lang}`` (``datasets.load_from_disk``; of a ``DatasetDict`` its "train" split) or the file
``{directory}/{lang}.parquet`` (``pyarrow.parquet``, column ``text``).  Both are read from local files only."""
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from .collate import MAX_CHARS_PER_TOKEN


def load_texts(directory: str, lang: str, what: str = "training", n_rows: Optional[int] = None) -> Sequence[str]:
    """The ``text`` column of a language's table, the first `n_rows` rows of it if given"""
    path = os.path.join(directory, lang)
    if os.path.exists(path):
        from datasets import DatasetDict, load_from_disk
        table = load_from_disk(path)
        if isinstance(table, DatasetDict):
            table = table["train"]
        if n_rows is not None:
            table = table.select(range(min(len(table), n_rows)))
        return table["text"]
    if os.path.exists(path + ".parquet"):
        import pyarrow.parquet as pq
        texts = pq.read_table(path + ".parquet", columns=["text"]).column("text").to_pylist()
        return texts if n_rows is None else texts[:n_rows]
    raise ValueError(f"Could not find {what} data for language {lang} in {directory}")


class TrainDataset:
    """``for batch in dataset`` never ends.  Each of a batch's texts belongs to one language, drawn with ``RandomState(0).choice(langs,
    p=language_probs)``; the language's rows are visited in the order of ``RandomState(0).permutation(len(rows))``, one generator per language,
    which also draws the next permutation when the rows run out (in the middle of a text, too).  Rows are stripped and empty ones skipped.
    With ``do_sequence_packing`` rows are appended — `eos_token` after each, the last one removed — until the text has ``block_size *
    MAX_CHARS_PER_TOKEN`` characters; without it a text is one row.  ``lang_code`` is "all" for more than one language, else the language."""

    def __init__(self, langs: Sequence[str], train_directory: str, language_probs, batch_size: int, block_size: int, do_sequence_packing: bool = True,
                 eos_token: Optional[str] = None):
        probs = np.asarray(language_probs, dtype=np.float64)
        self.langs, self.train_directory, self.language_probs = langs, train_directory, probs / probs.sum()
        self.batch_size, self.block_size, self.do_sequence_packing, self.eos_token = batch_size, block_size, do_sequence_packing, eos_token
        self.min_char_length = block_size * MAX_CHARS_PER_TOKEN
        self.dataset: Dict[str, Sequence[str]] = {lang: load_texts(train_directory, lang) for lang in list(langs)}

    def get_texts_in_each_language(self, n: int) -> Dict[str, List[str]]:
        return {lang: list(self.dataset[lang][:n]) for lang in self.langs}

    def get_texts(self, n: int) -> List[str]:
        texts: List[str] = []
        for batch in self:
            texts.extend(batch["texts"])
            if len(texts) >= n:
                break
        return texts[:n]

    def _rows(self, lang, orders, order_rng, position):
        """the stripped rows of `lang` in visiting order, for ever; the permutation is redrawn as soon as its last row has been read"""
        while True:
            row = self.dataset[lang][int(orders[lang][position[lang]])].strip()
            position[lang] += 1
            if position[lang] == len(orders[lang]):
                orders[lang] = order_rng[lang].permutation(len(self.dataset[lang]))
                position[lang] = 0
            yield row

    def __iter__(self):
        order_rng = {lang: np.random.RandomState(0) for lang in self.langs}
        lang_rng = np.random.RandomState(0)          # (RandomState(worker_idx))
        orders = {lang: order_rng[lang].permutation(len(self.dataset[lang])) for lang in self.langs}
        position = {lang: 0 for lang in self.langs}
        rows = {lang: self._rows(lang, orders, order_rng, position) for lang in self.langs}
        self.language_orders = orders
        eos = self.eos_token if self.do_sequence_packing else None
        while True:
            texts = []
            for _ in range(self.batch_size):
                lang = lang_rng.choice(self.langs, p=self.language_probs)
                text = ""
                while len(text) < self.min_char_length:
                    row = next(rows[lang])
                    if not row:
                        continue
                    text += row
                    if not self.do_sequence_packing:
                        break
                    if eos is not None:
                        text += eos
                if eos is not None:
                    text = text[:-len(eos)]          # the last eos
                texts.append(text)
            yield {"texts": texts, "lang_code": "all" if len(self.langs) > 1 else str(lang)}


class ValidDataset:
    """``len(dataset)`` batches: per language, in the order of `langs`, ``floor(rows / batch_size)`` full batches of consecutive rows (the
    remainder is dropped), of the first `n_subsample` rows if given.  ``dataset[i]`` is ``{"texts", "lang_code"}``.  The language "flan"
    reads the table "en", as in the reference."""

    def __init__(self, langs: Sequence[str], valid_directory: str, n_subsample: Optional[int], batch_size: int):
        self.batch_size, self.langs, self.n_subsample = batch_size, langs, n_subsample
        self.dataset = {lang: load_texts(valid_directory, "en" if lang == "flan" else lang, "validation", n_subsample) for lang in langs}

    def _batches(self, lang) -> int:
        return len(self.dataset[lang]) // self.batch_size

    def __len__(self) -> int:
        return sum(self._batches(lang) for lang in self.langs)

    def __getitem__(self, idx: int):
        if idx < 0 or idx >= len(self):
            raise IndexError(idx)
        for lang in self.langs:
            if idx < self._batches(lang):
                return {"texts": list(self.dataset[lang][idx * self.batch_size:(idx + 1) * self.batch_size]), "lang_code": lang}
            idx -= self._batches(lang)
