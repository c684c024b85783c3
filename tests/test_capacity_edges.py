"""-m gpu: every compiled kernel configuration at its dof and body capacity edges, against the fp64 oracle.

The fixtures run each configuration at one size (Lift nv 15, Stack nv 21, Baxter 36 bodies, PickPlace nv 37) and the 64 x 64 configuration not at all.
The models of tests/capacity_models.py put a configuration's bottom dof edge (nv = 17, 33, 49), its top edge (a full last tile: nv = 16, 32, 48, 64), its
body edge (nbody = 32, 64: every lane a body) and, for 64 x 64, dof 63 of the 64-bit dof masks, nq = 71 (two passes of the `i += 64` loops) and eight
articulated trees under the same comparisons the fixture models get.  The 64-body models are one chain 56 - 62 bodies deep: body trees deeper than 32 need
a sixth pointer-jumping round in the kinematics, which the 64-body builds had not had (frames off by a metre at nbody 64 before it).  At the top edges both orders run: chain last (its dense mass-matrix block holds the
top dofs and straddles the last tile boundary) and chain first (the contact rows touch the top dofs).

Tolerances are the ones the suite holds for the same quantities on the fixture models (tests/test_hip_parity.py): frames 3e-6, qM / qfrc_bias 1e-5 relative,
qfrc_passive 1e-4 of max(1, max), contact dist / pos 2e-6, normal force 1e-3 relative, qacc 1e-3 of max(1, max |qacc|), Jacobians 5e-6, tracking
|dq| < 5e-4 and |dv| < 5e-3, ctrl 2e-3 of max(1, max |ctrl|).  Counts and contact identity get no slack.  Measured errors of every case: profiles/capacity_edges_parity.txt.

cfg1_nq40 holds the qpos edge of that build (nq = nv + 8) with six ball joints in mid-chain: ball joints with descendants (mass-matrix off-diagonals, the
velocity recursion of their children, Jacobian columns below them).  The rows cfg1_top / cfg1_top_nb32 reach nv = 32 within configuration 1's 16 joints and four trees only through a ball joint (13 hinges + 3 free bodies
= nv 31 is the most without one): the 32 x 32 build carries ball joints for them (frames, motion axes, quaternion integration; csrc/Makefile -DRSIM_BALL).
"""
import functools

import numpy as np
import pytest
import torch

from robosuite_amd import backend, mjcf
from tests import capacity_models as cm
from tests.util import make_oracle

pytestmark = pytest.mark.gpu

CASES = [(n, True) for n in cm.COMPOSITIONS] + [(n, False) for n in cm.TOP_EDGES]
IDS = [n + ("" if last else "-chain_first") for n, last in CASES]
B = 3
TOL = dict(xpos=3e-6, xquat=3e-6, qM=1e-5, full_M=1e-5, qfrc_bias=1e-5, qfrc_passive=1e-4, con_dist=2e-6, con_pos=2e-6, con_force=1e-3, qacc=1e-3, jac=5e-6, dq=5e-4, dv=5e-3, ctrl=2e-3)


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-12, np.abs(np.asarray(b)).max()))


def frozen(a):
    a = np.array(a, dtype=np.float64)
    a.setflags(write=False)
    return a


class Figures:
    """Measured error beside the tolerance held: every figure is printed, then all are asserted."""

    def __init__(self, test, case):
        self.test, self.case, self.rows = test, case, []

    def add(self, what, err, tol):
        self.rows.append((what, float(err), float(tol)))

    def check(self):
        worst = {}
        for what, err, tol in self.rows:
            k = what.split("@")[0]
            if k not in worst or err / tol > worst[k][0] / worst[k][1]:
                worst[k] = (err, tol, what)
        for k, (err, tol, what) in worst.items():
            print(f"[capacity] {self.test:8s} {self.case:22s} {k:13s} err {err:9.2e} tol {tol:8.1e} ({what})")
        bad = [(w, e, t) for w, e, t in self.rows if not e < t]
        assert not bad, (self.case, bad)


def forward_record(od, tip):
    jp, jr = od.jac("site", tip)
    return dict(xpos=frozen(od.xpos), xquat=frozen(od.xquat), qM=frozen(od.qM), full_M=frozen(od.full_M()), qfrc_bias=frozen(od.qfrc_bias),
                qfrc_passive=frozen(od.qfrc_passive), qacc=frozen(od.qacc), ncon=od.ncon, nefc=od.nefc, contacts=od.contacts(), jacp=frozen(jp), jacr=frozen(jr))


@functools.lru_cache(maxsize=None)
def reference(name, chain_last):
    """The compiled model and, computed once on the oracle and left unchanged: the three states of (a) with their forward quantities, and the tracking
    run of (b) under its seeded ctrl."""
    _, flat = cm.build(name, chain_last)
    tip = flat.names["site"].index("tip")
    om, od, _ = make_oracle(flat)
    q, v = cm.start_state(flat, 1)
    od.qpos[:] = q; od.qvel[:] = v; od.qacc_warmstart[:] = 0; od.ctrl[:] = 0; od.forward()
    states = []
    for k in range(51):
        if k in (0, 25, 50):
            states.append((frozen(od.qpos), frozen(od.qvel)))
        od.step()
    fwd = []
    for sq, sv in states:
        od.qpos[:] = sq; od.qvel[:] = sv; od.qacc_warmstart[:] = 0; od.ctrl[:] = 0; od.forward()
        fwd.append(forward_record(od, tip))
    rng = np.random.default_rng(2)
    ctrl = frozen(0.3 * rng.standard_normal((50, flat.nu)))
    od.qpos[:] = q; od.qvel[:] = v; od.qacc_warmstart[:] = 0; od.ctrl[:] = 0; od.forward()
    track = []
    for k in range(50):
        od.ctrl[:] = ctrl[k]
        od.step()
        if k % 10 == 9:
            track.append((frozen(od.qpos), frozen(od.qvel), od.ncon, od.nefc))
    return dict(flat=flat, tip=tip, states=states, fwd=fwd, ctrl=ctrl, track=track, start=(frozen(q), frozen(v)))


def batch_for(name, flat, controller=None, task=None):
    hm = backend.HipModel(flat)
    assert hm.kernel_config()[0] == cm.COMPOSITIONS[name][0]
    if controller is not None:
        hm.set_controller(controller)
    if task is not None:
        hm.set_task(task)
    return hm, backend.HipBatch(hm, B)


def put(hb, q, v):
    hb.set("qpos", np.asarray(q)); hb.set("qvel", np.asarray(v)); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)


@pytest.mark.parametrize("name,chain_last", CASES, ids=IDS)
def test_forward_quantities_at_the_capacity_edges_match_the_oracle(name, chain_last):
    """(a) the form of test_forward_quantities_match_oracle at the seeded start state (hinges in +-0.5 rad: some limits active) and the oracle's states
    25 and 50 substeps on: frames, full qM, bias and passive forces, counts, the contact list, accelerations, the tip site's Jacobian (its columns are the
    chain's dofs) and the C-ABI full_M export."""
    ref = reference(name, chain_last)
    flat, tip = ref["flat"], ref["tip"]
    hm, hb = batch_for(name, flat)
    fig = Figures("forward", IDS[CASES.index((name, chain_last))])
    nv = flat.nv
    for i, ((q, v), o) in enumerate(zip(ref["states"], ref["fwd"])):
        put(hb, q, v)
        hb.forward()
        assert hb.get("ncon")[0] == o["ncon"] and hb.get("nefc")[0] == o["nefc"], (i, hb.get("ncon"), o["ncon"], hb.get("nefc"), o["nefc"])
        fig.add(f"xpos@{i}", np.abs(hb.get("xpos")[0].ravel() - o["xpos"]).max(), TOL["xpos"])
        fig.add(f"xquat@{i}", np.abs(hb.get("xquat")[0].ravel() - o["xquat"]).max(), TOL["xquat"])
        fig.add(f"qM@{i}", rel(hb.get("qM")[0].ravel(), o["qM"]), TOL["qM"])
        fig.add(f"full_M@{i}", rel(hb.full_M(0), o["full_M"]), TOL["full_M"])
        fig.add(f"qfrc_bias@{i}", rel(hb.get("qfrc_bias")[0], o["qfrc_bias"]), TOL["qfrc_bias"])
        fig.add(f"qfrc_passive@{i}", np.abs(hb.get("qfrc_passive")[0] - o["qfrc_passive"]).max(), TOL["qfrc_passive"] * max(1.0, np.abs(o["qfrc_passive"]).max()))
        fig.add(f"qacc@{i}", np.abs(hb.get("qacc")[0] - o["qacc"]).max(), TOL["qacc"] * max(1.0, np.abs(o["qacc"]).max()))
        hc = hb.contacts(0)
        assert len(hc) == len(o["contacts"])
        for a, b in zip(hc, o["contacts"]):
            assert (a["geom1"], a["geom2"], a["dim"]) == (b["geom1"], b["geom2"], b["dim"]), i
            fig.add(f"con_dist@{i}", abs(a["dist"] - b["dist"]), TOL["con_dist"])
            fig.add(f"con_pos@{i}", np.abs(a["pos"] - b["pos"]).max(), TOL["con_pos"])
            fig.add(f"con_force@{i}", abs(a["normal_force"] - b["normal_force"]), TOL["con_force"] * max(1.0, abs(b["normal_force"])))
        jp, jr = hb.jac_site(0, tip)
        fig.add(f"jac@{i}", max(np.abs(jp - o["jacp"]).max(), np.abs(jr - o["jacr"]).max()), TOL["jac"])
        assert jp.shape == (3, nv) and np.abs(o["jacp"]).max() > 0.01       # the comparison is not of zeros
        # every env of the batch computes the same
        assert np.array_equal(hb.get("qacc")[0], hb.get("qacc")[B - 1]) and np.array_equal(hb.get("qM")[0], hb.get("qM")[B - 1])
    fig.check()


@pytest.mark.parametrize("name,chain_last", CASES, ids=IDS)
def test_substeps_at_the_capacity_edges_track_the_oracle(name, chain_last):
    """(b) 50 substeps of rsim_step against the oracle's under seeded ctrl (sigma 0.3, redrawn every substep), compared every ten."""
    ref = reference(name, chain_last)
    flat = ref["flat"]
    hm, hb = batch_for(name, flat)
    fig = Figures("substeps", IDS[CASES.index((name, chain_last))])
    put(hb, *ref["start"])
    hb.forward()
    for k in range(50):
        hb.set("ctrl", ref["ctrl"][k])
        hb.step()
        if k % 10 == 9:
            oq, ov, ncon, nefc = ref["track"][k // 10]
            fig.add(f"dq@{k + 1}", np.abs(hb.get("qpos")[0] - oq).max(), TOL["dq"])
            fig.add(f"dv@{k + 1}", np.abs(hb.get("qvel")[0] - ov).max(), TOL["dv"])
            assert hb.get("ncon")[0] == ncon and hb.get("nefc")[0] == nefc, (k, hb.get("ncon"), ncon, hb.get("nefc"), nefc)
    assert np.array_equal(hb.get("qpos")[0], hb.get("qpos")[B - 1])
    fig.check()


def torque_controller(flat):
    """JOINT_TORQUE with torque compensation on the last eight actuated hinges (for chain last at nv 64: dofs 50 - 57), no gripper."""
    act = list(range(flat.nu))[-8:]
    jid = [flat.names["joint"].index(f"h{a}") for a in act]
    n = len(act)
    return dict(type="JOINT_TORQUE", qpos_idx=[int(flat.jnt_qposadr[j]) for j in jid], dof_idx=[int(flat.jnt_dofadr[j]) for j in jid], act_idx=act,
                eef_site=flat.names["site"].index("tip"), base_site=flat.names["site"].index("base_site"), input_min=[-1.0] * n, input_max=[1.0] * n,
                output_min=[-0.5] * n, output_max=[0.5] * n, grip_act=[], grip_sign=[], grip_speed=0.0, torque_limits=[[-2.0] * n, [2.0] * n],
                use_torque_compensation=1)


@pytest.mark.parametrize("name,chain_last", CASES, ids=IDS)
def test_fused_control_step_at_the_capacity_edges(name, chain_last):
    """(c) rsim_control_step, four control steps of 25 substeps, each against the oracle's controller loop from the kernel's own state.  The observation
    program reads qpos[0 .. nq), the top 16 qvel and the top 16 qacc (at nv 64: more than 64 slots, qpos indices beyond 64).  Envs 0 and 1 start equal and stay
    bitwise equal beside an env 2 in another state; a second run from the same inputs is bitwise equal.  ctrl = clip(goal + qfrc_bias of the controlled
    dofs) is held to 2e-3 of max(1, max |ctrl|), the tightest bound the suite holds for ctrl elsewhere."""
    ref = reference(name, chain_last)
    flat = ref["flat"]
    nq, nv = flat.nq, flat.nv
    cfg = torque_controller(flat)
    top = list(range(max(0, nv - 16), nv))
    prog = [("qpos", i, 0) for i in range(nq)] + [("qvel", i, 0) for i in top] + [("qacc", i, 0) for i in top]
    hm, hb = batch_for(name, flat, cfg, dict(task="none", obs=prog))
    assert hm.action_dim == len(cfg["act_idx"])
    fig = Figures("control", IDS[CASES.index((name, chain_last))])
    om, od, _ = make_oracle(flat)
    from oracle.oracle import OracleController
    oc = OracleController(cfg)
    q0, v0 = ref["start"]
    q2, v2 = cm.start_state(flat, 5)
    rng = np.random.default_rng(3)
    actions = rng.uniform(-1, 1, (4, 1, hm.action_dim)).repeat(B, 1)
    actions[:, 2] = rng.uniform(-1, 1, (4, hm.action_dim))

    def run(against_oracle):
        put(hb, np.stack([q0, q0, q2]), np.stack([v0, v0, v2]))
        hb.set("time", 0)
        hb.forward(); hb.ctrl_reset()
        out = []
        for t in range(4):
            pre = {k: hb.get(k) for k in ("qpos", "qvel", "qacc_warmstart", "ctrl")}
            hb.control_step(torch.tensor(actions[t], dtype=torch.float32, device="cuda"), 25)
            hb.sync()
            post = {k: hb.get(k) for k in ("qpos", "qvel", "ctrl", "obs")}
            out.append(post)
            assert all(np.isfinite(a).all() for a in post.values())
            # the observation record is the state the step ended in
            assert np.array_equal(post["obs"][:, :nq], post["qpos"]) and np.array_equal(post["obs"][:, nq:nq + len(top)], post["qvel"][:, top])
            for k in post:
                assert np.array_equal(post[k][0], post[k][1]), (t, k)
            assert not np.array_equal(post["qpos"][0], post["qpos"][2])
            if not against_oracle:
                continue
            for e in (0, 2):
                od.qpos[:] = pre["qpos"][e]; od.qvel[:] = pre["qvel"][e]; od.qacc_warmstart[:] = pre["qacc_warmstart"][e]; od.ctrl[:] = pre["ctrl"][e]
                od.forward(); oc.reset(od)
                oc.env_step(od, actions[t][e].astype(np.float64), 25)
                fig.add(f"dq@{t}.{e}", np.abs(post["qpos"][e] - od.qpos).max(), TOL["dq"])
                fig.add(f"dv@{t}.{e}", np.abs(post["qvel"][e] - od.qvel).max(), TOL["dv"])
                fig.add(f"ctrl@{t}.{e}", np.abs(post["ctrl"][e] - od.ctrl).max(), TOL["ctrl"] * max(1.0, np.abs(od.ctrl).max()))
                # the qacc slots: the acceleration of the last substep
                fig.add(f"obs_qacc@{t}.{e}", np.abs(post["obs"][e, nq + len(top):] - od.qacc[top]).max(), TOL["qacc"] * max(1.0, np.abs(od.qacc).max()))
            assert np.abs(od.ctrl[cfg["act_idx"]]).max() > 0.05
        return out

    first = run(True)
    second = run(False)
    for a, b in zip(first, second):
        for k in a:
            assert np.array_equal(a[k], b[k]), k
    fig.check()


def test_contact_overflow_on_the_64_dof_configuration_is_counted():
    """(d) the 64 x 64 configuration has no capacity tier above it: a state that needs more than its 32 contacts must show in RSIM_OVERFLOW.  Seven boxes
    piled 1 mm into the floor and each other, 40 contacts / 120 rows on the oracle; envs 1 and 2 hold the same pile half a metre up (24 contacts)."""
    flat = mjcf.compile_mjcf(cm.overflow_xml())
    hm = backend.HipModel(flat)
    assert hm.kernel_config()[0] == 4
    hb = backend.HipBatch(hm, B)
    om, od, _ = make_oracle(flat)
    od.qpos[:] = flat.qpos0; od.qvel[:] = 0; od.qacc_warmstart[:] = 0; od.ctrl[:] = 0; od.forward()
    assert (od.ncon, od.nefc) == (40, 120) and hb.maxcon == 32
    up = np.array(flat.qpos0, dtype=np.float64)
    for j in range(len(flat.jnt_type)):
        if int(flat.jnt_type[j]) == 0:
            up[int(flat.jnt_qposadr[j]) + 2] += 0.5
    put(hb, np.stack([np.asarray(flat.qpos0, dtype=np.float64), up, up]), np.zeros((B, flat.nv)))
    hb.set("overflow", 0)
    hb.forward()
    ncon, ovf = hb.get("ncon"), hb.get("overflow")
    assert list(ncon) == [32, 24, 24], ncon
    assert ovf[0] >= 40 - 32 and ovf[1] == 0 and ovf[2] == 0, ovf
    assert np.isfinite(hb.get("qacc")).all()
    # the kernel's contacts are, in order, a subsequence of the oracle's list
    oc, k = od.contacts(), 0
    for a in hb.contacts(0):
        while k < len(oc) and not ((a["geom1"], a["geom2"], a["dim"]) == (oc[k]["geom1"], oc[k]["geom2"], oc[k]["dim"]) and np.abs(a["pos"] - oc[k]["pos"]).max() < TOL["con_pos"]
                                   and abs(a["dist"] - oc[k]["dist"]) < TOL["con_dist"]):
            k += 1
        assert k < len(oc), (a["geom1"], a["geom2"], a["pos"])
        k += 1
    hb.forward()
    ovf2 = hb.get("overflow")
    assert ovf2[0] == 2 * ovf[0] and ovf2[1] == 0 and ovf2[2] == 0, (ovf, ovf2)


@pytest.mark.parametrize("name,why", (("trees9", "exceeds the largest compiled kernel configuration"), ("nq73", "with ball joints .*nq 73.* exceeds"),
                                      ("nq41", "with ball joints .*nq 41.* exceeds .*nq 40")))
def test_one_beyond_the_largest_configuration_is_refused_by_batch_create(name, why):
    """The GPU twin of the host test: with a device present rsim_batch_create itself refuses (nothing is truncated to fit).  nq 73 at nv 64 takes ball joints
    (eight trees give nq - nv = 8 at most without), which the 64 x 64 build does not carry: that is the refusal it meets first.  nq 41 at nv 32 is one qpos
    entry beyond the 32 x 32 build, which does carry them: the nq limit itself (cfg1_nq40, one ball joint fewer, runs in the three tests above)."""
    hm = backend.HipModel(mjcf.compile_mjcf(cm.model_xml(**cm.REFUSED[name])))
    assert hm.kernel_config()[0] == -1
    with pytest.raises(backend.RsimError, match=why):
        backend.HipBatch(hm, 1)


def test_ball_joints_beyond_the_one_build_that_carries_them_are_refused_loudly():
    """Ball joints are compiled into the 32 x 32 configuration only: a model with one that needs a larger build (here five trees, nv 38) is refused by name,
    and so is a limited ball joint (no limit rows for it)."""
    hm = backend.HipModel(mjcf.compile_mjcf(cm.model_xml(n_hinge=11, n_free=4, n_ball=1)))
    assert hm.kernel_config()[0] == -1
    with pytest.raises(backend.RsimError, match="with ball joints .* exceeds"):
        backend.HipBatch(hm, 1)
    xml = cm.model_xml(n_hinge=11, n_free=3, n_ball=1).replace('type="ball"', 'type="ball" limited="true" range="0 1"')
    hm = backend.HipModel(mjcf.compile_mjcf(xml))
    with pytest.raises(backend.RsimError, match="limited ball joints"):
        backend.HipBatch(hm, 1)
