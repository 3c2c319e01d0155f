"""Tokenizer sampling on the device (profiles/sample_tokenizer_bench.md).

    python tools/sample_tokenizer_bench.py [--texts 512] [--chars 2048] [--depth 8] [--seed-size 32768] [--stride 4] [--check] [--json out.json] [--once]

One process.  The queue is filled with --depth batches (pop_prev = False), then every timed call pops the oldest batch and pushes a new one,
as a training step does: ``DeviceTokenizerSampler.sample_tokenizer(texts, seed_size, 16, stride, noise_std, True, True, check=False)``,
with noise_std 0 and 0.05 alternating, the median of 10 after 3 warm-ups, by host clock (call to synchronised stream) and between HIP
events.  Reported with them: the distinct keys of the merged table and the table's occupancy.  --check compares the first merged table with
tests/sampler_ref.py (tens of seconds of plain Python).  --once: the fill and ten calls, nothing timed (for a kernel trace).

No ratio is asserted: the Rust sampler cannot be built here, and the Python restatement is not a fair opponent.
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

from encode_bench import corpus                                            # noqa: E402
from zett_amd.tokenizer_sampling import DeviceTokenizerSampler             # noqa: E402


def median_ms(samples):
    return float(np.median(samples)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--texts", type=int, default=512)
    ap.add_argument("--chars", type=int, default=2048)
    ap.add_argument("--depth", type=int, default=8)
    ap.add_argument("--seed-size", type=int, default=32768)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--table", type=int, default=1 << 21)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--once", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n_batches = args.depth + 4
    batches = [corpus(args.texts, args.chars, seed=s) for s in range(n_batches)]
    t0 = time.perf_counter()
    sampler = DeviceTokenizerSampler(dev, max_depth=args.depth, table_capacity=args.table, list_capacity=args.table // 4, max_pieces=1 << 16)
    torch.cuda.synchronize()
    t_create = time.perf_counter() - t0
    for texts in batches[:args.depth]:
        sampler.sample_tokenizer(texts, 30000, 16, args.stride, 0.0, False)
    step = [args.depth]

    def call(noise_std):
        texts = batches[step[0] % n_batches]
        step[0] += 1
        return sampler.sample_tokenizer(texts, args.seed_size, 16, args.stride, noise_std, True, True, seed=step[0], check=False)
    first = call(0.0)
    torch.cuda.synchronize()
    assert int(first.status.item()) == 0, f"status {int(first.status.item())}"
    keys, counts, _ = sampler.merged_table()
    result = {"texts": args.texts, "text_bytes": len("".join(batches[args.depth]).encode("utf-8")), "depth": args.depth, "seed_size": args.seed_size,
              "stride": args.stride, "table_capacity": args.table, "distinct_keys": len(keys), "occupancy": len(keys) / args.table,
              "score_sum": int(counts.astype(np.int64).sum()), "pieces": int(first.n.item()), "create_ms": t_create * 1e3}
    if args.check:
        sys.path.insert(0, os.path.join(REPO))
        from tests import sampler_ref
        ref = sampler_ref.SamplerRef()
        for texts in batches[:args.depth]:
            ref.sample(texts, 30000, 16, args.stride, 0.0, False)
        want = ref.sample(batches[args.depth], args.seed_size, 16, args.stride, 0.0, True, True)
        assert {k: int(c) for k, c in zip(keys, counts)} == ref.merged, "the merged table differs from the definition"
        got = first.to_list()
        assert [p for p, _ in got] == [sampler_ref.byte_level(k) for k, _ in want], "the pieces differ from the definition"
        g, w = np.array([s for _, s in got]), np.array([s for _, s in want])
        ok = w != 0.0
        result["checked"] = True
        result["max_score_ulp"] = float((np.abs(g[ok] - w[ok]) / np.spacing(np.abs(w[ok]))).max())
    if args.once:
        for i in range(10):
            call(0.05 * (i % 2))
        torch.cuda.synchronize()
        print(json.dumps(result), flush=True)
        return
    timings = {0.0: ([], []), 0.05: ([], [])}
    for i in range(13):
        for noise_std in (0.0, 0.05):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            a.record()
            out = call(noise_std)
            b.record()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert int(out.status.item()) == 0
            if i >= 3:
                timings[noise_std][0].append(dt)
                timings[noise_std][1].append(a.elapsed_time(b) * 1e-3)
    for noise_std, (host, events) in timings.items():
        result[f"noise_{noise_std}_host_ms"] = median_ms(host)
        result[f"noise_{noise_std}_events_ms"] = median_ms(events)
    t0 = time.perf_counter()
    call(0.0).to_list()
    result["as_list_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
