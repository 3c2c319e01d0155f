"""From a sampled piece list to input_ids: the host-built path against the device-built one (profiles/sampled_tables_bench.md).

    python tools/sampled_tables_bench.py [--texts 512] [--chars 2048] [--depth 8] [--seed-size 32768] [--block 128] [--json out.json] [--once]

One process, two samplers with the same queue (--depth batches each), the two paths alternating on the same batch, the median of 10
after 3 warm-ups, by host clock with the stream synchronised after every stage:

  (a) the parent path   sampler.sample_tokenizer(as_list=True) -> build_sampled_tokenizer -> DeviceTextEncoder.from_tokenizer ->
                        convert_ids_to_tokens + get_surface_form_matrix -> encode
  (b) the device path   sampler.sample_tokenizer(check=False) -> DeviceSampledVocabulary.build -> encode

The reference tokenizer is a stand-in with four special tokens and a <s> $A </s> template; the hn tokenizer and hn_surface_maxlen are
those of tests/golden/sample_tokenizer_prefix.json.gz.  Before anything is timed the device path's input_ids, surface forms, priors, byte
lengths and map are compared with the host path's, and the device-built piece table with the host-built tokenizer's model.  --once: the
fill and six device-path steps, nothing timed (for a kernel trace).

No ratio is asserted.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from encode_bench import SPECIALS, corpus                                                                       # noqa: E402
from tests import sampler_ref                                                                                   # noqa: E402
from zett_amd.sampled_vocab import DeviceSampledVocabulary, json_round_trip as sv_json                         # noqa: E402
from zett_amd.surface_forms import HnTokenizerSpec, get_surface_form_matrix                                     # noqa: E402
from zett_amd.text_encode import DeviceTextEncoder                                                              # noqa: E402
from zett_amd.tokenizer_sampling import DeviceTokenizerSampler, build_sampled_tokenizer                         # noqa: E402


def reference_tokenizer():
    from tokenizers import Tokenizer, models, processors
    from transformers import PreTrainedTokenizerFast
    tk = Tokenizer(models.WordLevel(dict(SPECIALS), unk_token="<unk>"))
    tk.post_processor = processors.TemplateProcessing(single="<s> $A </s>", special_tokens=[("<s>", 0), ("</s>", 2)])
    return PreTrainedTokenizerFast(tokenizer_object=tk, bos_token="<s>", eos_token="</s>", unk_token="<unk>", pad_token="<pad>", clean_up_tokenization_spaces=False)


class Clock:
    def __init__(self):
        self.stages = {}
        self.t = None

    def start(self):
        torch.cuda.synchronize()
        self.t = time.perf_counter()

    def lap(self, name, keep):
        torch.cuda.synchronize()
        now = time.perf_counter()
        if keep:
            self.stages.setdefault(name, []).append(now - self.t)
        self.t = now

    def medians(self):
        out = {k: float(np.median(v)) * 1e3 for k, v in self.stages.items()}
        out["total"] = float(np.median(np.sum([v for v in self.stages.values()], axis=0))) * 1e3
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=512)
    ap.add_argument("--chars", type=int, default=2048)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--seed-size", type=int, default=32768)
    ap.add_argument("--block", type=int, default=128)
    ap.add_argument("--table", type=int, default=1 << 21)
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    fx = sampler_ref.load_fixture(sampler_ref.FIXTURES[0])
    hn, maxlen = sampler_ref.tokenizer_of(fx["hn_tokenizer"]), int(fx["hn_surface_maxlen"])
    reference = reference_tokenizer()
    n_batches = args.depth + 4
    batches = [corpus(args.texts, args.chars, seed=s) for s in range(n_batches)]
    samplers = [DeviceTokenizerSampler(dev, max_depth=args.depth, table_capacity=args.table, list_capacity=args.table // 4, max_pieces=1 << 16) for _ in range(2)]
    for sampler in samplers:
        for texts in batches[:args.depth]:
            sampler.sample_tokenizer(texts, 30000, 16, 4, 0.0, False)
    vocabulary = DeviceSampledVocabulary(reference, True, hn_tokenizer=hn, hn_surface_maxlen=maxlen, device=dev)
    bare = DeviceSampledVocabulary(reference, True, device=dev)          # no surface forms: flag + emit + tables + record read alone
    host_clock, device_clock, bare_clock = Clock(), Clock(), Clock()

    def host_path(texts, step, keep):
        c = host_clock
        c.start()
        sampled = samplers[0].sample_tokenizer(texts, args.seed_size, 16, 4, 0.0, True, True, seed=step, check=False)
        c.lap("sample", keep)
        found = sampled.to_list()
        c.lap("read_back_as_list", keep)
        tokenizer, special_ids_map, scores = build_sampled_tokenizer(found, reference, True)
        c.lap("build_sampled_tokenizer", keep)
        encoder = DeviceTextEncoder.from_tokenizer(tokenizer, device=dev)
        c.lap("from_tokenizer", keep)
        tokens = tokenizer.convert_ids_to_tokens(range(len(tokenizer)))
        byte_lengths = np.array([len(token) for token in tokens])
        surface_forms = get_surface_form_matrix(tokens, maxlen, hn, verbose=False, device=dev)[0]
        c.lap("surface_forms", keep)
        rows = encoder(texts, args.block, special_ids_map)
        c.lap("encode", keep)
        encoder.close()
        return rows, special_ids_map, surface_forms, scores, byte_lengths, tokenizer

    def device_path(texts, step, keep):
        c = device_clock
        c.start()
        sampled = samplers[1].sample_tokenizer(texts, args.seed_size, 16, 4, 0.0, True, True, seed=step, check=False)
        c.lap("sample", keep)
        built = vocabulary.build(sampled, args.seed_size)
        c.lap("build_with_surface_forms", keep)
        rows = built.encoder(texts, args.block, built.special_ids_map)
        c.lap("encode", keep)
        bare_clock.start()
        bare.build(sampled, args.seed_size)
        bare_clock.lap("build_alone", keep)
        return rows, built

    step = args.depth
    texts = batches[step % n_batches]
    rows_h, map_h, sf_h, priors_h, lengths_h, tokenizer_h = host_path(texts, step, False)
    rows_d, built = device_path(texts, step, False)
    assert torch.equal(rows_d["input_ids"], rows_h["input_ids"]) and torch.equal(rows_d["attention_mask"], rows_h["attention_mask"]), "input_ids differ"
    assert np.array_equal(built.surface_forms.cpu().numpy(), np.asarray(sf_h)), "surface forms differ"
    assert built.priors.cpu().numpy().tobytes() == np.asarray(priors_h, dtype=np.float64).tobytes(), "priors differ"
    assert built.byte_lengths.cpu().tolist() == lengths_h.tolist() and built.special_ids_map == map_h, "byte lengths or map differ"
    spec = HnTokenizerSpec.from_tokenizer(tokenizer_h)          # the model the host-built encoder segments with, against the device-built table
    o = spec.piece_offsets
    want = {(bytes(spec.piece_bytes[o[i]:o[i + 1]]), int(spec.piece_ids[i]), np.float64(spec.piece_scores[i]).tobytes()) for i in range(len(spec.piece_ids))}
    keys, ids, scores, _ = vocabulary.piece_table()
    got = {(k, int(i), np.float64(s).tobytes()) for k, i, s in zip(keys, ids, scores)}
    assert got == want, f"the piece table differs from the host-built model's in {len(got ^ want)} entries"
    moved = int((np.asarray([sv_json(x) for x in np.asarray(priors_h).tolist()]) != np.asarray(priors_h)).sum())
    result = {"scores_through_json": bool(vocabulary.scores_through_json), "scores_the_round_trip_moves": moved, "texts": args.texts, "text_bytes": len("".join(texts).encode("utf-8")), "depth": args.depth, "seed_size": args.seed_size, "block_size": args.block,
              "hn_surface_maxlen": maxlen, "n_vocab": built.n_vocab, "checked": True}
    if args.once:
        for i in range(5):
            step += 1
            device_path(batches[step % n_batches], step, False)
        torch.cuda.synchronize()
        print(json.dumps(result), flush=True)
        return
    for i in range(13):
        step += 1
        texts = batches[step % n_batches]
        host_path(texts, step, i >= 3)
        device_path(texts, step, i >= 3)
    result["host_path_ms"] = host_clock.medians()
    result["device_path_ms"] = device_clock.medians()
    result["device_build_alone_ms"] = bare_clock.medians()["build_alone"]
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
