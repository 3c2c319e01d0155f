"""Host parts of the shared table's contract (tests/test_shared_table_contract_gpu.py holds the device's): sharding.SharedTable on a
stand-in engine — a table with fewer rows than ranks over gloo, and the range word of the table's build (cleared before, read after,
OR-reduced over the group; left alone when the engine accumulates)."""
import json
import os
import subprocess
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# tests/test_host_logic.py's FakeEngine (table row i = a function of id_list[i]), plus the range word of HipEngine: table_rows raises
# bit 1 for source id 7, a forward starts a word of its own unless the engine accumulates, an accumulating read clears.
_FAKE_ENGINE = r"""
import torch
class FakeEngine:
    V = 1000
    def __init__(self):
        self.word, self.range_accumulate, self.calls = 0, False, []
    def set_option(self, key, value):
        assert key == "range_accumulate"
        self.range_accumulate = bool(value)
    def range_flags(self):
        word = self.word
        if self.range_accumulate:
            self.word = 0
        return word
    def table_plan(self, m):
        ids = torch.unique(m)
        flag = torch.zeros(self.V, dtype=torch.int32); flag[ids] = 1
        slot = torch.zeros(self.V + 1, dtype=torch.int32); slot[1:] = torch.cumsum(flag, 0)
        return slot, ids.to(torch.int32), int(ids.numel())
    def table_buffers(self, n):
        return torch.full((n, 8), float("nan"), dtype=torch.float16), torch.full((n, 2), float("nan"))
    def table_rows(self, id_list, first, count, src, table, stats):
        self.calls.append((first, count))
        i = id_list[first:first + count].long()
        if (i == 7).any():
            self.word |= 1
        table[first:first + count] = src[i].to(torch.float16); stats[first:first + count, 0] = i.float(); stats[first:first + count, 1] = 1.0
    def forward_table(self, rows, table, stats, id_slot, lang):
        if not self.range_accumulate:
            self.word = 0
        sl = id_slot[rows.long()].long()
        x = table[sl].float().sum(1) * stats[sl][..., 1].sum(1, keepdim=True) + stats[sl][..., 0].sum(1, keepdim=True)
        return x, None, x[:, 0].clone() + lang
"""

_WORKER = _FAKE_ENGINE + r"""
import os, sys, json
import torch.distributed as dist
sys.path.insert(0, {repo!r})
from zett_amd.sharding import SharedTable, predict_sharded
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
g = torch.Generator(); g.manual_seed(11)
src = torch.randn(1000, 8, generator=g)
two = torch.tensor([[7, 400, 7], [400, 400, 7], [7, 7, 7], [400, 7, 400]])          # 2 distinct ids on 3 ranks: rank 2's slice is empty
eng = FakeEngine()
eng.word = 4                                            # what an earlier forward left: not the build's
shared = SharedTable(eng, two, src)
ok = shared.n_ids == 2 and shared.per == 1 and shared.ranges == [(min(rank, 2), min(rank + 1, 2))] and eng.calls == [(min(rank, 2), 1 if rank < 2 else 0)]
alone = SharedTable(FakeEngine(), two, src, only_rank=0, world=1)
ok = ok and torch.equal(shared.table[:2], alone.table[:2]) and torch.equal(shared.stats[:2], alone.stats[:2])
# only rank 0 built the row of id 7: every rank holds its bit, and nobody the earlier forward's
ok = ok and shared.range_flags == 1 and alone.range_flags == 1 and eng.range_accumulate is False and eng.word == 0
full = predict_sharded(shared.predict(3), two); one = alone.predict(3)(two)
ok = ok and torch.equal(full[0], one[0]) and full[1] is None and torch.equal(full[2], one[2])
mine = torch.cat([shared.table[:2].float(), shared.stats[:2]], dim=1)          # (float32 holds a float16 exactly)
tables = [torch.empty_like(mine) for _ in range(world)]
dist.all_gather(tables, mine)
ok = ok and all(torch.equal(t, tables[0]) for t in tables)
# an accumulating engine keeps its word: no reduction, no clearing read
acc = FakeEngine(); acc.set_option("range_accumulate", 1); acc.word = 4
kept = SharedTable(acc, two, src)
ok = ok and kept.range_flags is None and acc.range_accumulate is True and acc.word == (5 if rank == 0 else 4)
flag = torch.tensor([1 if ok else 0]); dist.all_reduce(flag, op=dist.ReduceOp.MIN)
if rank == 0:
    json.dump({{"ok": bool(flag.item())}}, open({out!r}, "w"))
dist.barrier(); dist.destroy_process_group()
"""


def test_shared_table_with_fewer_ids_than_ranks_gloo(tmp_path):
    """World 3, a matrix of 2 distinct ids: the rank with the empty slice takes part in the exchange and in the reduction of the
    build's range word; every rank ends with the same table and the same flags."""
    out = os.path.join(tmp_path, "res.json")
    script = os.path.join(tmp_path, "worker.py")
    open(script, "w").write(_WORKER.format(repo=REPO, out=out))
    port = str(29900 + (os.getpid() % 90))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=port, OMP_NUM_THREADS="2")
    subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3",
                    "--master-addr", "127.0.0.1", "--master-port", port, script],
                   check=True, env=env, timeout=60, cwd="/tmp")
    assert json.load(open(out))["ok"], "the ranks of a 2-id table disagree"


def test_shared_table_range_word_protocol_single_process():
    """Without a group: the build's bits are the table's, an earlier forward's are dropped, a later forward does not take them away;
    a failing build leaves the engine's option as it was; an engine without a range word is left alone."""
    scope = {}
    exec(_FAKE_ENGINE, scope)
    FakeEngine = scope["FakeEngine"]
    from zett_amd.sharding import SharedTable
    g = torch.Generator(); g.manual_seed(11)
    src = torch.randn(1000, 8, generator=g)
    hot = torch.tensor([[7, 400, 7], [400, 400, 9]])
    clean = torch.tensor([[8, 400, 8], [400, 400, 9]])
    eng = FakeEngine()
    eng.word = 6
    shared = SharedTable(eng, hot, src)
    assert shared.range_flags == 1 and eng.range_accumulate is False
    shared.predict(0)(hot)
    assert eng.range_flags() == 0 and shared.range_flags == 1
    eng.word = 2
    assert SharedTable(eng, clean, src).range_flags == 0
    for world, want in ((2, [1, 0]), (4, [1, 0, 0, 0])):          # ids 7, 9, 400: only the rank that builds id 7's row sees its bit
        assert [SharedTable(eng, hot, src, only_rank=r, world=world).range_flags for r in range(world)] == want

    class Refusing(FakeEngine):
        def table_rows(self, *args):
            raise ValueError("no folded table")

    bad = Refusing()
    try:
        SharedTable(bad, hot, src)
        raise AssertionError("the refusal was swallowed")
    except ValueError:
        pass
    assert bad.range_accumulate is False

    class Wordless:
        table_plan, table_buffers = FakeEngine.table_plan, FakeEngine.table_buffers
        V = FakeEngine.V

        def table_rows(self, id_list, first, count, src, table, stats):
            table[first:first + count] = 0

    assert SharedTable(Wordless(), hot, src).range_flags is None
