"""The N > 1 path on REAL devices over RCCL (backend "nccl"): runs wherever at least two GPUs are visible and skips
otherwise (the build's GPU boxes have one; the row-block / all-gather logic itself is covered on CPU over gloo by
tests/test_host_logic.py and, with two ranks sharing one device, by tests/test_bench_gpu.py).

  * bench.py --gpus 2 under torch.distributed.run, nccl: one JSON line, the gathered rows equal a local forward bit
    for bit (bench.py checks that itself and exits non-zero otherwise);
  * predict_sharded on two GPUs: the gathered matrices equal a single-GPU forward of the whole vocabulary bit for bit,
    for one and for several row blocks per rank, over both transports (RCCL all-gather, direct fan-out) and with the
    exchange of pred_in / bias started behind their own completion point (zett_stream_wait_output) or behind the forward.
"""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

needs_two_gpus = pytest.mark.skipif(not torch.cuda.is_available() or torch.cuda.device_count() < 2,
                                    reason="needs at least two GPUs (RCCL over xGMI)")


def _torchrun(script_args, port, timeout=900):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("ZETT_BENCH_ONE_DEVICE", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port)] + script_args
    return subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=timeout)


@needs_two_gpus
@pytest.mark.parametrize("extra", [[], ["--serial-allgather"], ["--chunks", "3"], ["--gather-mode", "fanout"], ["--serial-allgather", "--gather-mode", "fanout"],
                                   ["--serial-allgather", "--no-early-gather"], ["--partition", "affinity", "--gather-mode", "fanout"], ["--table-exchange"]],
                         ids=["two-blocks-self-launched", "serial", "three-blocks", "fanout", "serial-fanout", "serial-late", "affinity-fanout", "shared-table"])
def test_bench_two_gpus_nccl(extra):
    bench_args = [os.path.join(REPO, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--workload", "tinyllama_neox",
                  "--rows", "30001", "--no-cpu-baseline", "--full"] + extra
    if not extra:
        # the driver's form: `python bench.py --gpus N` with no launcher — bench.py re-executes itself under torch.distributed.run
        env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "ZETT_BENCH_ONE_DEVICE")}
        out = subprocess.run([sys.executable] + bench_args, cwd=REPO, env=env, capture_output=True, text=True, timeout=900)
    else:
        out = _torchrun(bench_args, 29541)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["rows"] == 30001 and d["value"] > 0 and "TEST HOOK" not in d["data"]
    assert d["exchange"]["mode"] == ("fanout" if "fanout" in extra else "allgather") and d["exchange_exposed_ms_per_step"] is not None
    assert d["exchange"]["GPU_MAX_HW_QUEUES"] == "8" and len(lines[0].encode()) < 6000


_WORKER = r"""
import os, sys, json
import numpy as np, torch, torch.distributed as dist
sys.path.insert(0, {repo!r})
import zett_amd
zett_amd.configure_hw_queues()          # before the first CUDA call: the exchange overlaps the forward only on its own hardware queue
from bench import device_weights
from zett_amd import synth
from zett_amd.dims import HypernetDims
from zett_amd.hypernet import HipEngine
from zett_amd.sharding import predict_sharded
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
torch.cuda.set_device(rank)
dev = torch.device("cuda", rank)
dist.init_process_group("nccl", device_id=dev)
cfg, _, src_dtype, hist = synth.workload("tinyllama_neox")
eng = HipEngine(HypernetDims.from_config(cfg), 1e-5, dev, "f16")
eng.load_weights(device_weights(cfg, dev, seed=5))
src = torch.from_numpy(synth.make_source_embeddings(cfg, 5, dtype=src_dtype)).to(dev)
ids = torch.from_numpy(synth.make_surface_forms(cfg, 40001, seed=5, hist=hist, n_special=1)).to(dev)
predict = lambda rows: eng.forward(rows, src, -1)
single = predict(ids)
ok = True
for chunks in (1, 2, 4):
    for mode in ("allgather", "fanout"):
        for ready in (None, eng.stream_wait_output):      # exchange behind the whole forward / pred_in and bias behind their own completion point
            full = predict_sharded(predict, ids, chunks=chunks, mode=mode, ready=ready)
            torch.cuda.synchronize()
            ok = ok and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(full, single))
# r5: the rows sharded in the id-affinity order (zett_partition_rows: every rank computes the same order, no communication) and
# scattered back behind each block's exchange — over RCCL, both transports; the orders of all ranks must be identical
from zett_amd.sharding import affinity_order
n_ids = cfg["original_vocab_size"] + cfg["hn_n_extra_tokens"]
for chunks in (1, 2):
    order = affinity_order(ids, world, cfg["pad_token_id"], n_ids, chunks=chunks)
    same = [torch.empty_like(order) for _ in range(world)]
    dist.all_gather(same, order)
    ok = ok and all(torch.equal(o, order) for o in same) and sorted(order.tolist()) == list(range(ids.shape[0]))
    for mode in ("allgather", "fanout"):
        for ready in (None, eng.stream_wait_output):
            full = predict_sharded(predict, ids, chunks=chunks, mode=mode, ready=ready, order=order)
            torch.cuda.synchronize()
            ok = ok and all((a is None and b is None) or torch.equal(a, b) for a, b in zip(full, single))
flag = torch.tensor([1 if ok else 0], device=dev)
dist.all_reduce(flag, op=dist.ReduceOp.MIN)
if rank == 0:
    json.dump({{"ok": bool(flag.item())}}, open({out!r}, "w"))
dist.barrier(); dist.destroy_process_group()
"""


@needs_two_gpus
def test_predict_sharded_two_gpus_nccl(tmp_path):
    out = os.path.join(tmp_path, "res.json")
    script = os.path.join(tmp_path, "worker.py")
    open(script, "w").write(_WORKER.format(repo=REPO, out=out))
    res = _torchrun([script], 29543)
    assert res.returncode == 0, res.stderr[-3000:]
    assert json.load(open(out))["ok"], "rows gathered over RCCL differ from the single-GPU forward"
