#!/usr/bin/env python
"""Time of the Rescaler fit on the GPU: the column-moments pass alone, and the whole ZettHypernet.init_rescaler.

    python tools/rescaler_init_bench.py [--shapes 32000x8192,128256x8192] [--dtypes float32,bfloat16] [--reps 10]
                                        [--workload mistral_gpt2_32k] [--anchors 2048] [--md profiles/rescaler_init.md]

Prints ONE JSON line; --md also writes the table.  Every figure is the min and max of `reps` single calls, each between two device
events after a warm-up call (init_rescaler: a host clock around a call that ends in a device synchronise — it waits for the host
itself, to read the states' counts and the range word).  bytes/s of the moments pass = rows * cols * sizeof(element) / time: the
matrix is read once, the partials and the state are under 1 % of that.

The yardstick measured in the same process, not the code under test, is the torch path of a naive port: x.float().mean(0) and
x.float().std(0, unbiased=False), run twice for the two matrices such a port reads (the source matrix for in_scaler, and its halves
again as the targets).  The project's other streaming passes, for scale: the lexical gather-mean at 4.9 TB/s and the AdamW update at
5.7 TB/s (profiles/)."""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from zett_amd import synth, training  # noqa: E402
from zett_amd.config import ZettHypernetConfig  # noqa: E402
from zett_amd.hypernet import ZettHypernet  # noqa: E402

PEAK_TBS = 8.0          # sanity only: an implied bandwidth above the HBM peak means the timing or the byte count is wrong


def event_reps(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return min(out), max(out)


def wall_reps(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return min(out), max(out)


def torch_path(x):
    for _ in range(2):
        x.float().mean(0)
        x.float().std(0, unbiased=False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="32000x8192,128256x8192")
    ap.add_argument("--dtypes", default="float32,bfloat16")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--workload", default="mistral_gpt2_32k")
    ap.add_argument("--anchors", type=int, default=2048)
    ap.add_argument("--md", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/rescaler_init_bench.py needs an MI355X"
    dev = torch.device("cuda", 0)
    out = {"reps": args.reps, "chunk": training.COL_MOMENTS_CHUNK, "moments": [], "init_rescaler": None}

    for shape in args.shapes.split(","):
        rows, cols = (int(v) for v in shape.split("x"))
        for name in args.dtypes.split(","):
            dtype = getattr(torch, name)
            x = (torch.randn((rows, cols), dtype=torch.float32, device=dev) * 0.02 + 0.01).to(dtype)
            lo, hi = event_reps(lambda: training.column_moments(x), args.reps)
            t_lo, t_hi = event_reps(lambda: torch_path(x), max(2, args.reps // 3))
            nbytes = float(rows) * cols * x.element_size()
            run = {"rows": rows, "cols": cols, "dtype": name, "ms_min": lo, "ms_max": hi, "TBps_at_min": nbytes / (lo * 1e-3) / 1e12, "TBps_at_max": nbytes / (hi * 1e-3) / 1e12,
                   "torch_two_matrices_ms_min": t_lo, "torch_two_matrices_ms_max": t_hi}
            assert run["TBps_at_min"] <= PEAK_TBS, f"implied {run['TBps_at_min']:.2f} TB/s exceeds the HBM peak: timing or byte count is wrong"
            out["moments"].append(run)
            del x
            torch.cuda.empty_cache()

    cfg, _rows, src_dtype, hist = synth.workload(args.workload)
    model = ZettHypernet(ZettHypernetConfig(**cfg)).to(dev)
    src = torch.from_numpy(synth.make_source_embeddings(cfg, seed=3, dtype=src_dtype)).to(dev)
    ids = torch.from_numpy(synth.make_surface_forms(cfg, args.anchors, seed=3, hist=hist)).to(dev)
    lo, hi = wall_reps(lambda: model.init_rescaler(ids, src), args.reps)
    m_lo, m_hi = event_reps(lambda: training.column_moments(src), args.reps)
    f_lo, f_hi = wall_reps(lambda: model(ids, source_embeddings=src, lang_index=0), args.reps)
    t_lo, t_hi = event_reps(lambda: torch_path(src), max(2, args.reps // 3))
    out["init_rescaler"] = {"workload": args.workload, "anchors": args.anchors, "source": list(src.shape), "source_dtype": src_dtype, "precision": model.precision,
                            "ms_min": lo, "ms_max": hi, "source_moments_ms_min": m_lo, "source_moments_ms_max": m_hi,
                            "anchor_forward_ms_min": f_lo, "anchor_forward_ms_max": f_hi, "torch_two_matrices_ms_min": t_lo, "torch_two_matrices_ms_max": t_hi}
    print(json.dumps(out))
    if args.md:
        lines = ["# Rescaler fit: the column-moments pass and the whole init_rescaler (tools/rescaler_init_bench.py)", "",
                 f"min – max of {args.reps} single calls on one MI355X; chunk = {out['chunk']} rows.  torch: `x.float().mean(0)` and",
                 "`x.float().std(0, unbiased=False)`, twice, for the two matrices a naive port reads.", "",
                 "| matrix | type | moments pass ms | TB/s | torch path ms |", "|---|---|---|---|---|"]
        for r in out["moments"]:
            lines.append(f"| {r['rows']} x {r['cols']} | {r['dtype']} | {r['ms_min']:.3f} – {r['ms_max']:.3f} | {r['TBps_at_max']:.2f} – {r['TBps_at_min']:.2f} | "
                         f"{r['torch_two_matrices_ms_min']:.2f} – {r['torch_two_matrices_ms_max']:.2f} |")
        i = out["init_rescaler"]
        lines += ["", f"`init_rescaler`, {i['workload']} hypernet, {i['anchors']} anchors, source {i['source'][0]} x {i['source'][1]} {i['source_dtype']}, {i['precision']} arithmetic:", "",
                  "| step | ms |", "|---|---|",
                  f"| whole call (host clock; re-uploads the weights it changed, waits for the counts and the range word) | {i['ms_min']:.2f} – {i['ms_max']:.2f} |",
                  f"| of which: moments of the source matrix | {i['source_moments_ms_min']:.3f} – {i['source_moments_ms_max']:.3f} |",
                  f"| of which: a forward over the anchors on an engine that is already built | {i['anchor_forward_ms_min']:.2f} – {i['anchor_forward_ms_max']:.2f} |",
                  f"| torch path on the source matrix | {i['torch_two_matrices_ms_min']:.2f} – {i['torch_two_matrices_ms_max']:.2f} |", ""]
        os.makedirs(os.path.dirname(os.path.abspath(args.md)), exist_ok=True)
        with open(args.md, "w") as f:
            f.write("\n".join(lines))


if __name__ == "__main__":
    main()
