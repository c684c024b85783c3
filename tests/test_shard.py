"""Multi-process path (world_size 2, gloo, CPU): env sharding + rollout-stats all-reduce + max-over-ranks timing."""
import os
import socket
import subprocess

import pytest
import sys

import numpy as np

from robosuite_amd import shard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKER = r"""
import os, sys, json
sys.path.insert(0, os.environ["RSIM_ROOT"])
import numpy as np, torch
from robosuite_amd import shard, lift
rank, local_rank, world = shard.init_process_group("gloo")
ids = shard.env_block(11, rank, world)
acts = lift.env_actions(ids, 3)
st = shard.RolloutStats()
st.add(env_steps=len(ids) * 3, reward_sum=float(acts.sum()), episodes=len(ids))
tot = st.allreduce()
tmax = shard.max_over_ranks(1.0 + rank)
class StandInComm:      # same call signature as backend.HipComm.allreduce (the C-ABI's rsim_allreduce_stats), carried by gloo here
    def allreduce(self, values, op="sum"):
        t = torch.tensor(np.asarray(values, dtype=np.float64))
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.SUM if op == "sum" else torch.distributed.ReduceOp.MAX)
        return t.numpy()
st2 = shard.RolloutStats(comm=StandInComm())
st2.add(env_steps=len(ids) * 3, successes=rank + 1)
tot2 = st2.allreduce()
if rank == 0:
    print(json.dumps(dict(tot=tot, tmax=tmax, n0=len(ids), path=st.path, tot2=tot2, path2=st2.path)))
torch.distributed.destroy_process_group()
"""


def test_env_block_partitions_exactly():
    for n, w in ((4096, 8), (11, 2), (7, 8), (2048, 3)):
        blocks = [shard.env_block(n, r, w) for r in range(w)]
        assert np.array_equal(np.concatenate(blocks), np.arange(n))
        assert max(len(b) for b in blocks) - min(len(b) for b in blocks) <= 1


def test_world_size_2_gloo(tmp_path):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, RSIM_ROOT=ROOT)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    import json
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    r = json.loads(line)
    from robosuite_amd import lift
    assert r["tot"]["env_steps"] == 33 and r["tot"]["episodes"] == 11 and r["n0"] == 6
    assert abs(r["tot"]["reward_sum"] - float(lift.env_actions(np.arange(11), 3).sum())) < 1e-4
    assert r["tmax"] == 2.0
    # the same fields through a communicator object (bench.py hands RolloutStats the C-ABI's RCCL communicator when there is more than one rank)
    assert r["path"] == "torch.distributed (gloo)" and r["path2"].startswith("rsim_allreduce_stats")
    assert r["tot2"]["env_steps"] == 33 and r["tot2"]["successes"] == 3


HANDSHAKE_WORKER = r"""
import os, sys, json
sys.path.insert(0, os.environ["RSIM_ROOT"])
import numpy as np, torch
from robosuite_amd import shard
rank, local_rank, world = shard.init_process_group("gloo")
class Comm:
    def __init__(self, uid, rank, world, device): self.uid, self.closed = uid, False
    def close(self): self.closed = True
def draw_ok(): return bytes(range(128))
def draw_fails(): raise OSError("librccl: undefined symbol ncclGetUniqueId")
made = []
def create_ok(uid, r, w, d): made.append(Comm(uid, r, w, d)); return made[-1]
def create_fails_on_1(uid, r, w, d):
    if r == 1: raise RuntimeError("ncclCommInitRank: unhandled system error")
    return create_ok(uid, r, w, d)
res = {}
for name, draw, create in (("ok", draw_ok, create_ok), ("draw_fails", draw_fails, create_ok), ("create_fails_on_1", draw_ok, create_fails_on_1)):
    made.clear()
    try:
        c = shard.hip_comm(rank, world, 0, unique_id=draw, create=create)
        res[name] = ["comm", c.uid == bytes(range(128))]
    except shard.CommUnavailable as e:
        res[name] = ["unavailable", str(e), len(made), all(m.closed for m in made)]
    # whatever happened, the ranks are still in step: a collective right behind it pairs up
    res[name].append(shard.max_over_ranks(float(rank)))
# one file per rank: two ranks writing to the launcher's one stdout pipe can land on the same line
with open(os.path.join(os.environ["RSIM_OUT"], "rank%d.json" % rank), "w") as f: json.dump(res, f)
torch.distributed.destroy_process_group()
"""


def test_c_abi_communicator_handshake_is_collective_safe(tmp_path):
    """Round-5 advisor finding: a rank that failed before the broadcast of the unique id left the others blocked in it, and a creation that failed on a subset of
    ranks left the job with a half-formed communicator.  With injected failures (rank 0 cannot draw the id; rank 1 cannot create) every rank must raise
    CommUnavailable -- none hangs, none keeps a communicator -- and the next collective of the job still pairs up."""
    import json
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    script = tmp_path / "worker.py"
    script.write_text(HANDSHAKE_WORKER)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
                          "--master-port", str(port), str(script)], env=dict(os.environ, RSIM_ROOT=ROOT, RSIM_OUT=str(tmp_path)), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {r: json.loads((tmp_path / ("rank%d.json" % r)).read_text()) for r in (0, 1) if (tmp_path / ("rank%d.json" % r)).exists()}
    assert sorted(rows) == [0, 1]
    for r in (0, 1):
        assert rows[r]["ok"] == ["comm", True, 1.0]
        assert rows[r]["draw_fails"][0] == "unavailable" and rows[r]["draw_fails"][2] == 0 and rows[r]["draw_fails"][-1] == 1.0      # nobody called create
        assert rows[r]["create_fails_on_1"][0] == "unavailable" and rows[r]["create_fails_on_1"][3] is True and rows[r]["create_fails_on_1"][-1] == 1.0   # rank 0 closed the one it made
    assert "undefined symbol" in rows[0]["draw_fails"][1] and "this rank" in rows[1]["create_fails_on_1"][1] and "another rank" in rows[0]["create_fails_on_1"][1]


@pytest.mark.parametrize("config", ("lift", "stack"))     # stack = BASELINE configs[2], the one BASELINE.json assigns to eight GPUs
def test_bench_launches_its_own_ranks(config):
    """`python bench.py --gpus 2` (no torchrun around it) must spawn one rank per GPU itself; without a GPU every rank stops at the
    device check, after the process group came up (gloo here, RCCL on the GPU box)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--config", config],
                         capture_output=True, text=True, timeout=600)
    import torch
    if torch.cuda.is_available():
        return   # on a GPU box the run either completes (>= 2 GPUs) or fails on the device ordinal; the launcher is what is under test here
    assert out.returncode != 0
    assert "bench.py rank 0/2: no GPU visible" in out.stderr and "bench.py rank 1/2: no GPU visible" in out.stderr, out.stderr[-3000:]


def test_bench_secondary_region_child_fails_loudly_without_a_gpu():
    """`python bench.py --full` times BASELINE configs[2..4] in one child process each (`--secondary-only <config>`); a child that dies -- a fault of the GPU queue
    aborts the process that owns it -- must leave a non-zero exit code and no JSON record, which the parent reports as `{"error": ...}` in config.other_configs."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("the child runs the region on a GPU box")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--secondary-only", "stack", "--other-steps", "1", "--other-preroll", "0"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 3 and not [ln for ln in out.stdout.splitlines() if ln.startswith("{")]


def test_c_abi_comm_rejects_bad_arguments_before_touching_rccl():
    """rsim_comm_create / rsim_allreduce_stats (include/rsim.h) fail loudly on bad arguments -- checked before RCCL or a device is touched, so this runs without a GPU."""
    import ctypes as C

    from robosuite_amd import backend

    L = backend.lib()
    out = C.c_void_p()
    uid = C.create_string_buffer(128)
    assert L.rsim_comm_create(C.cast(uid, C.c_void_p), 128, 2, 2, 0, C.byref(out)) != 0 and b"rank 2 of 2" in L.rsim_last_error()
    assert L.rsim_comm_create(C.cast(uid, C.c_void_p), 64, 0, 1, 0, C.byref(out)) != 0      # id too short
    assert L.rsim_comm_unique_id(C.cast(uid, C.c_void_p), 16) != 0
    v = np.zeros(3)
    assert L.rsim_allreduce_stats(None, v.ctypes.data_as(C.c_void_p), 3, 0) != 0


@pytest.mark.gpu
def test_c_abi_allreduce_over_rccl_one_rank():
    """The RCCL path of rsim_allreduce_stats end to end on the one GPU a test box has: unique id, communicator of world 1, sum and max of a float64 vector
    (what a one-rank reduction must return: the input).  The N > 1 reduction semantics are covered by the gloo test above through the same RolloutStats fields."""
    from robosuite_amd import backend

    uid = backend.HipComm.unique_id()
    assert len(uid) == 128 and any(uid)
    c = backend.HipComm(uid, 0, 1, device=0)
    v = np.array([4096.0 * 200, 1234.5, 17.0, 0.0, 3.0])
    assert np.array_equal(c.allreduce(v, "sum"), v) and np.array_equal(c.allreduce(v, "max"), v)
    with pytest.raises(backend.RsimError):
        c.allreduce(np.zeros(65))          # more than the communicator's staging buffer holds
    c.close()
