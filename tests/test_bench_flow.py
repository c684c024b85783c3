"""bench.py's control flow and output contract, run on the CPU against a stand-in batch (no kernel, no oracle): the driver parses ONE JSON line from rank 0, so a
NameError on a path only a GPU box reaches would cost the round its measurement.  Everything device-side is replaced (torch.cuda, the env the factory would build, the
child processes of the secondary regions); what runs is main() itself: argument handling, pre-roll / warm-up / timed regions, the headline region alone in a plain run,
the order of the regions of a --full run (the secondary configurations directly behind the headline region, ahead of the open-loop and double-buffered ones),
statistics, PMC evidence lookup and the JSON assembly."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "robosuite_amd", "librsim_hip.so")), reason="needs the built library (its sha goes into the line)")


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self, stream=None):
        pass

    def elapsed_time(self, other):
        return 1.5


class _Batch:
    maxcon, maxefc = 16, 64

    def __init__(self, n, log):
        self.n, self.log = n, log

    def stream(self):
        return 0

    def group_stream(self, g):
        return g

    def sync(self):
        pass

    def set(self, name, value):
        self.log.append(("set", name))

    def set_stream_groups(self, g):
        self.log.append(("groups", g))

    def randomize_dynamics(self, seed, step):
        self.log.append(("dr", step))

    def tier_stats(self):
        return (3 * self.log.count(("step", self.n)), self.log.count(("step", self.n)))

    def tensor(self, name):
        if name == "qpos":
            return torch.zeros(self.n, 9)
        if name == "cap_need":
            return torch.ones(self.n * 2, dtype=torch.int32)
        return torch.zeros(self.n, dtype=torch.int32)

    def get(self, name):
        self.log.append(("get", name))
        rows = np.arange(self.n, dtype=np.int32 if name in ("done", "success") else np.float32)   # row i holds env i
        return np.repeat(rows[:, None], 60, axis=1) if name in ("obs", "terminal_obs") else rows


class _Env:
    def __init__(self, n, log, episodes):
        self.batch = _Batch(n, log)
        self.model = types.SimpleNamespace(action_dim=7, nobs=60, cstate_size=32, int=lambda name: 128)
        self.n, self.log, self.steps = n, log, 0
        log.append(("env", n, episodes))

    def step(self, a):
        assert a.shape == (self.n, 7)
        self.steps += 1
        self.log.append(("step", self.n))
        self.log.append(("action", a.numpy().tobytes()))

    def bank_stats(self):
        return {"steps": self.steps, "polls": self.steps // 2, "rows": 3 * self.steps, "tick_s": 1e-6 * self.steps, "upkeep_s": 2e-6 * self.steps}

    def bank_quiesce(self):
        self.log.append(("quiesce", self.n))

    def _bank_stop(self):
        pass

    def _bank_patch_offsets(self):
        return [0, 1, 2]

    def reward(self):
        return torch.zeros(self.n)

    def success(self):
        return torch.zeros(self.n)


def _run_main(monkeypatch, capsys, argv, child=None):
    import bench

    log = []
    fake_cuda = types.SimpleNamespace(is_available=lambda: True, set_device=lambda d: None, synchronize=lambda: None, Event=_Event,
                                      ExternalStream=lambda s, device=None: s, empty_cache=lambda: None)

    class _Torch:                                   # the real torch, except that "cuda" devices are the CPU and torch.cuda is the stand-in above
        cuda = fake_cuda

        def __getattr__(self, k):
            return getattr(torch, k)

        def device(self, *a):
            return torch.device("cpu")

    monkeypatch.setattr(bench, "torch", _Torch())
    monkeypatch.setattr(bench, "build_env", lambda config, flat, cfg, ids, device, episodes: _Env(len(ids), log, episodes))
    monkeypatch.setattr(bench.shard, "max_over_ranks", lambda x, device="cpu": float(x))

    def default_child(cmd, **kw):
        assert "--secondary-only" in cmd
        oc = cmd[cmd.index("--secondary-only") + 1]
        log.append(("child", oc, cmd[cmd.index("--other-steps") + 1], cmd[cmd.index("--other-preroll") + 1]))
        return types.SimpleNamespace(returncode=0, stderr="", stdout="noise\n" + json.dumps({"workload": oc, "value": 1.0, "ms_per_step": 2.0}) + "\n")

    monkeypatch.setattr(subprocess, "run", child or default_child)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines                  # ONE JSON line
    return json.loads(lines[0]), log


def test_default_command_flow_and_contract(monkeypatch, capsys):
    d, log = _run_main(monkeypatch, capsys, ["--full", "--steps", "4", "--warmup", "2", "--preroll", "3", "--envs-per-gpu", "8", "--groups", "2", "--no-cpu-baseline"])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["higher_is_better"] is True and d["scaling"] == "weak" and d["dtype"] == "f32"
    assert d["unit"] == "env-steps/s" and d["value"] > 0 and d["vs_baseline"] is None and "Lift" in d["metric"] and "workload" in d["config"]
    assert d["config"]["envs_per_gpu"] == 8 and d["config"]["open_loop"]["stream_groups"] == 2 and d["config"]["double_buffered"]["halves"] == [4, 4]
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and r["kernel_ms"] == 1.5 and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    assert isinstance(r["traffic"], (float, str)) and r["traffic"] != "absent"       # a figure, or "stale:<sha>" said out loud
    # the three secondary configurations, each in its child process, on the quick protocol ...
    oc = d["config"]["other_configs"]
    assert set(oc) == {"stack", "peg", "pickplace"} and all(v["value"] == 1.0 for v in oc.values())
    kids = [e for e in log if e[0] == "child"]
    assert kids == [("child", "stack", "50", "500"), ("child", "peg", "50", "500"), ("child", "pickplace", "20", "500")]       # pre-roll = the horizon: steady state
    # the slow-window diagnostics of the round-5 review: per-step distribution and what the capacity tier did in the timed region, at top level
    assert d["step_ms"] == {"min": 1.5, "p50": 1.5, "p90": 1.5, "max": 1.5} and d["tier_env_steps"] == 3 * 4 and d["tier_changes_in_mid_step"] == 4
    assert d["collective"] == "none (one rank)" and d["config"]["steady_state"] is False and d["config"]["episode_window"] == [5, 9]
    # ... directly behind the headline region: 3 pre-roll + 2 warm-up + 4 timed steps of the full batch, the children, THEN stream groups and the two half batches
    first_child, groups_on = log.index(kids[0]), log.index(("groups", 2))
    assert [e for e in log[:first_child] if e[0] == "step"] == [("step", 8)] * 9 and log[first_child - 1] == ("quiesce", 8)
    assert first_child < groups_on and not any(e == ("step", 4) for e in log[:groups_on])
    assert [e for e in log[groups_on:] if e == ("step", 8)] == [("step", 8)] * 4 and sum(e == ("step", 4) for e in log) == 2 * (3 + 2 + 4)


def test_plain_run_is_the_headline_region_alone(monkeypatch, capsys):
    """Without --full the run is set-up, pre-roll, warm-up, the timed region and the line: no child process, no stream groups, no half batches, no CPU
    baseline.  Its line has the fields of a --full line, and its timed region the inputs of a --full run: the same actions and a reset ring of the same size
    (493 + 2 + 4 launches stay inside one horizon, the --full run's 4 open-loop launches go past it)."""
    import bench

    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **k: pytest.fail("a plain run timed the CPU baseline"))
    argv = ["--steps", "4", "--warmup", "2", "--preroll", "493", "--envs-per-gpu", "8", "--groups", "2"]
    d, log = _run_main(monkeypatch, capsys, argv)
    assert {e[0] for e in log} == {"env", "set", "step", "action"} and [e for e in log if e[0] == "step"] == [("step", 8)] * (493 + 2 + 4)
    c = d["config"]
    assert d["cpu_baseline"] is None and c["open_loop"] is None and c["double_buffered"] is None and c["other_configs"] is None
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 4 and d["warmup"] == 2 and c["episode_window"] == [495, 499]

    monkeypatch.setattr(bench, "cpu_baseline", lambda *a, **k: {"value": 1.0})
    f, full_log = _run_main(monkeypatch, capsys, argv + ["--full"])
    assert set(f) == set(d) and set(f["config"]) == set(c) and f["cpu_baseline"] == {"value": 1.0}
    assert f["config"]["open_loop"] and f["config"]["double_buffered"] and set(f["config"]["other_configs"]) == {"stack", "peg", "pickplace"}
    envs = [e for e in log if e[0] == "env"]
    assert envs == [("env", 8, 4)] and [e for e in full_log if e[0] == "env"][0] == envs[0]
    actions = [e for e in log if e[0] == "action"]
    assert actions == [e for e in full_log if e[0] == "action"][:len(actions)]


def test_other_config_line_and_a_failing_child(monkeypatch, capsys):
    d, log = _run_main(monkeypatch, capsys, ["--full", "--config", "stack", "--steps", "2", "--warmup", "1", "--preroll", "0", "--envs-per-gpu", "4", "--no-open-loop", "--no-cpu-baseline"])
    assert "Stack" in d["metric"] and d["config"]["other_configs"] is None and d["config"]["open_loop"] is None and not any(e[0] == "child" for e in log)

    # a child that dies (a fault of the GPU queue aborts the process that owns it) is reported in the record; the headline line stands
    def dying(cmd, **kw):
        return types.SimpleNamespace(returncode=-6, stderr="Memory access fault by GPU node-2\n", stdout="")

    d, log = _run_main(monkeypatch, capsys, ["--full", "--steps", "2", "--warmup", "1", "--preroll", "0", "--envs-per-gpu", "4", "--no-open-loop", "--no-cpu-baseline"], child=dying)
    oc = d["config"]["other_configs"]
    assert set(oc) == {"stack", "peg", "pickplace"} and all("Memory access fault" in v["error"] for v in oc.values()) and d["value"] > 0


def test_dump_outputs_holds_the_last_timed_step(monkeypatch, capsys, tmp_path):
    """--dump-outputs DIR: what a caller of the timed path receives after its last step, read directly behind the headline region (before the
    open-loop region steps the envs on), one float32 / float64 .npy per array; above the byte cap every run keeps the same seeded sample of envs."""
    import bench

    names = ("env_ids", "obs", "reward", "done", "success", "terminal_obs")
    argv = ["--full", "--steps", "3", "--warmup", "1", "--preroll", "0", "--envs-per-gpu", "8", "--groups", "2", "--no-other-configs", "--no-cpu-baseline", "--dump-outputs"]
    d, log = _run_main(monkeypatch, capsys, argv + [str(tmp_path / "all")])
    first_get = log.index(("get", "obs"))
    assert [e for e in log[:first_get] if e[0] == "step"] == [("step", 8)] * (1 + 3) and first_get < log.index(("groups", 2))
    out = {k: np.load(tmp_path / "all" / f"{k}.npy") for k in names}
    assert sorted(os.listdir(tmp_path / "all")) == sorted(f"{k}.npy" for k in names)
    assert out["env_ids"].dtype == np.float64 and all(out[k].dtype == np.float32 for k in names[1:])
    assert out["obs"].shape == out["terminal_obs"].shape == (8, 60) and out["reward"].shape == out["done"].shape == (8,)
    assert np.array_equal(out["env_ids"], np.arange(8)) and np.array_equal(out["obs"][:, 0], out["env_ids"])

    row = sum(a[:1].nbytes for a in out.values())
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * row)
    samples = []
    for run in ("s1", "s2"):
        _run_main(monkeypatch, capsys, argv + [str(tmp_path / run)])
        samples.append({k: np.load(tmp_path / run / f"{k}.npy") for k in names})
    ids = samples[0]["env_ids"]
    assert len(ids) == 3 and np.all(np.diff(ids) > 0) and np.array_equal(samples[0]["obs"][:, 0], ids) and np.array_equal(samples[0]["done"], ids)
    assert all(np.array_equal(samples[0][k], samples[1][k]) for k in names)


def test_reference_baseline_harness_is_blocked_loudly_without_mujoco_and_runs_on_the_shim():
    """tools/bench_reference.py (BASELINE.md section 2, B-ref): without the `mujoco` wheel it must say so and exit 3 -- never substitute anything silently; with
    `--backend shim` the same harness (N processes, barrier, suite.make with the B-ref kwargs, env.step loop) runs end to end on the fp64 oracle and labels its number
    "port" / B-cpu, so that the day a wheel exists only the backend changes."""
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tool = os.path.join(root, "tools", "bench_reference.py")
    if importlib.util.find_spec("mujoco") is None:
        r = subprocess.run([sys.executable, tool, "--procs", "1", "--steps", "1", "--warmup", "0"], capture_output=True, text=True, timeout=600)
        d = json.loads(r.stdout.strip().splitlines()[-1])
        assert r.returncode == 3 and d["baseline"] == "B-ref" and "not importable" in d["error"]
    if not os.path.isdir("/root/reference/robosuite"):
        pytest.skip("no reference checkout: the shim run needs robosuite's own Python")
    r = subprocess.run([sys.executable, tool, "--procs", "2", "--steps", "3", "--warmup", "1", "--backend", "shim"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["baseline"] == "B-cpu" and d["kind"] == "port" and d["cores"] == 2 and d["value"] > 0 and "NOT MuJoCo" in d["sample"] and len(d["per_worker_steps_per_s"]) == 2
