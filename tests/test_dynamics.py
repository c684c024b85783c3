"""Dynamics at candidate configurations on the device (csrc/rsim_dyn.hip: rsim_config_inverse_dynamics, rsim_config_mass_matrix, rsim_config_jacobian) against
the fp64 statement by the definition (robosuite_amd/dynamics.py, model tables rounded to fp32 as the device holds them) and against the fp64 oracle.

  * scene D (tests/dynamics_scenes.py) at (5, 13): 65 candidates -- one wavefront that spans env boundaries and a second one with a single live lane -- on a
    batch with per-env parameters, one link's body_mass and one dof_armature overridden in every env, so that a lane reading another env's table is caught;
    for the arm's dofs and for every hinge and slide dof.
  * the shipped Lift / Panda asset at (3, 22), seven arm dofs, hand and fingers riding along, against the oracle directly (fed the fp32-rounded tables).
  * the shipped Baxter asset, both arms in one call at (2, 33): the arm-to-arm blocks of M are exactly zero and an arm's tau does not see the other's rates.
  * edges: n = 1, n = RSIM_JNT_MAX (a 16-hinge chain of tests/capacity_models.py), K = 1 with 2-D q, qd and qdd each None.
  * consistency with the simulator's own arrays, purity and determinism, M's symmetry, path_torques, refusals.

THE BOUND, by reasoning (dynamics_scenes.rounding_bound), not from a run: errors are absolute against per-scene scales (max |tau_ref|, max |M_ref|, 1 for J --
not per entry: entries cross zero) and bounded by (31 nbodies + 39) * 8 * 2^-24 for nbodies moved bodies on the longest path: ~31 roundings per body in
the pose, the forward walk and the backward sum, 39 once for joint frame, wrench or inertia and projection, intermediates within 8 times the scale.  Scene D
(4 bodies) 7.8e-5, the 16-hinge chain (16) 2.6e-4, Lift (11) 1.8e-4, Baxter (10) 1.7e-4.  The host rehearsal (tests/test_dynamics_core_host.py) is held to the
same bound: it runs the same source.  The device may differ from it by FMA contraction and its sincos: reorderings of roundings.  Measured worst values of
both are in profiles/dyn_parity.txt (tools/dyn_parity.py prints them from the functions below): rehearsal tau 1.9e-7, M 6.1e-7, J 4.4e-7 on scene D; device
tau 1.6e-7, M 4.9e-7, J 4.6e-7 there and tau 3.7e-7, M 6.3e-7, J 4.7e-7 at worst over every scene of this file -- no figure beyond the rehearsal's order."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from robosuite_amd import backend, dynamics, mjcf
from tests import clearance_scenes as S
from tests import dynamics_scenes as D
from tests import raycast_scenes as R
from tests.util import make_hip

pytestmark = pytest.mark.gpu


def dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def ask(hb, dofs, q, qd=None, qdd=None, site=None):
    """the three device calls -> dict of float64 arrays"""
    out = dict(tau=hb.config_inverse_dynamics(dofs, dev(q), dev(qd), dev(qdd)), M=hb.config_mass_matrix(dofs, dev(q)))
    if site is not None:
        out["jacp"], out["jacr"] = hb.config_jacobian(site, dofs, dev(q))
    assert all(t.dtype == torch.float32 for t in out.values())
    return {k: t.cpu().numpy().astype(np.float64) for k, t in out.items()}


def check(what, fig, bound):
    for k, v in fig.items():
        print(f"dynamics parity {what}: {k} {v:.3e} (bound {bound:.1e})")
    for k, v in fig.items():
        assert v <= bound, (what, k, v)


# ---- scene D, per-env parameters -------------------------------------------------------------------------------------------------------------------------
def scene_d_batch(B=5):
    flat = D.scene_d()
    hm, hb = make_hip(flat, None, B=B, per_env=True)
    hb.set("qpos", D.scene_d_qpos(flat, B).astype(np.float32)); hb.set("qvel", 0)
    mass, arm = hb.param_get("body_mass"), hb.param_get("dof_armature")
    b, d = flat.names["body"].index("l1"), S.dofs_of(flat, ("h2",))[0]
    for e in range(B):
        mass[e, b] *= 1.0 + 0.35 * (e + 1); arm[e, d] += 0.04 * (e + 1)
    hb.param_set("body_mass", mass); hb.param_set("dof_armature", arm)
    hb.forward()
    over = [{"body_mass": hb.param_get("body_mass")[e], "dof_armature": hb.param_get("dof_armature")[e]} for e in range(B)]
    return flat, hm, hb, over


def scene_d_figures(which, B=5, K=13, site_name="tip"):
    flat, hm, hb, over = scene_d_batch(B)
    dofs, site = D.dofs_d(flat, which), flat.names["site"].index(site_name)
    q, qd, qdd = D.draws(flat, dofs, B, K)
    qpos = hb.get("qpos").astype(np.float64)
    got = ask(hb, dofs, q, qd, qdd, site)
    assert got["tau"].shape == (B, K, len(dofs)) and got["M"].shape == (B, K, len(dofs), len(dofs)) and got["jacp"].shape == (B, K, 3, len(dofs))
    ref = D.reference(flat, qpos, dofs, q, qd, qdd, site, overrides=over)
    wrong = D.reference(flat, qpos, dofs, q, qd, qdd, site, overrides=over[0])      # every env on env 0's tables: what a lane off its env would compute
    return D.errors(got, ref), D.errors(got, wrong), D.rounding_bound(D.depth(flat, dofs), D.EPS32)


@pytest.mark.parametrize("which", ("arm", "all"))
def test_scene_d_per_env_parameters(which):
    fig, off, bound = scene_d_figures(which)
    check(f"scene D {which}", fig, bound)
    assert off["tau"] > 100 * bound and off["M"] > 100 * bound      # the overrides are visible: env 0's tables are wrong for the others


def test_scene_d_sites_moved_and_not():
    flat, hm, hb, over = scene_d_batch()
    dofs = D.dofs_d(flat, "arm")
    q = D.draws(flat, dofs, 5, 13)[0]
    qpos = hb.get("qpos").astype(np.float64)
    bound = D.rounding_bound(D.depth(flat, dofs), D.EPS32)
    for name in ("side_s", "f1_s"):
        site = flat.names["site"].index(name)
        jp, jr = (t.cpu().numpy().astype(np.float64) for t in hb.config_jacobian(site, dofs, dev(q)))
        ref = D.reference(flat, qpos, dofs, q, site=site, overrides=over, want=("J",))
        check(f"scene D arm, site {name}", D.errors(dict(jacp=jp, jacr=jr), ref), bound)
    jp, jr = hb.config_jacobian(flat.names["site"].index("side_s"), S.dofs_of(flat, ("s1", "h2")), dev(q[:, :, 1:]))
    assert not jp.any() and not jr.any()      # a site on a body no controlled dof moves: valid, zeros


# ---- the shipped assets ------------------------------------------------------------------------------------------------------------------------------------
def lift_batch(B=3):
    flat, cfg = R.lift()
    hm, hb = make_hip(flat, cfg, B=B)
    hb.set("qpos", np.tile(R.lift_init_qpos(flat, cfg), (B, 1)).astype(np.float32)); hb.set("qvel", 0)
    hb.forward(); hb.ctrl_reset()
    return flat, cfg, hm, hb


def baxter():
    assets = os.path.join(os.path.dirname(os.path.abspath(mjcf.__file__)), "assets")
    return mjcf.load_model(os.path.join(assets, "peg_baxter_joint_velocity.rsim")), json.load(open(os.path.join(assets, "peg_baxter_joint_velocity.cfg.json")))


def lift_figures(B=3, K=22):
    flat, cfg, hm, hb = lift_batch(B)
    dofs, site = list(range(7)), int(cfg["eef_site"])
    q, qd, qdd = D.draws(flat, dofs, B, K)
    got = ask(hb, dofs, q, qd, qdd, site)
    ref = D.oracle_reference(dynamics.model32(flat), hb.get("qpos").astype(np.float64), dofs, q, qd, qdd, site)
    return D.errors(got, ref), D.rounding_bound(D.depth(flat, dofs), D.EPS32)


def test_lift_panda_against_the_oracle():
    fig, bound = lift_figures()
    check("Lift / Panda", fig, bound)


def baxter_figures(B=2, K=33):
    flat, cfg = baxter()
    dofs = list(range(14))
    hm, hb = make_hip(flat, cfg, B=B)
    hb.set("qpos", np.tile(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel(), (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward()
    q, qd, qdd = D.draws(flat, dofs, B, K)
    got = ask(hb, dofs, q, qd, qdd)
    ref = D.oracle_reference(dynamics.model32(flat), hb.get("qpos").astype(np.float64), dofs, q, qd, qdd)
    return D.errors(got, ref), D.rounding_bound(D.depth(flat, dofs), D.EPS32), (hb, dofs, q, qd, qdd, got)


def test_baxter_both_arms_in_one_call():
    fig, bound, (hb, dofs, q, qd, qdd, got) = baxter_figures()
    check("Baxter, both arms", fig, bound)
    assert np.abs(got["M"][..., :7, :7]).min(axis=(0, 1)).max() > 0 and np.abs(got["M"][..., 7:, 7:]).max() > 0
    assert not got["M"][..., :7, 7:].any() and not got["M"][..., 7:, :7].any()      # the arm-to-arm blocks: exactly zero
    qd2, qdd2 = qd.copy(), qdd.copy()
    qd2[..., 7:] *= -0.5; qdd2[..., 7:] += 1.0      # other rates for the second arm ...
    tau2 = hb.config_inverse_dynamics(dofs, dev(q), dev(qd2), dev(qdd2)).cpu().numpy()
    assert np.array_equal(tau2[..., :7].astype(np.float64), got["tau"][..., :7])      # ... and the first arm's torques are the same bits
    assert np.abs(tau2[..., 7:] - got["tau"][..., 7:]).max() > 0.1


# ---- edges ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_one_dof_and_two_d_tensors_and_absent_rates():
    flat, hm, hb, over = scene_d_batch(B=3)
    qpos = hb.get("qpos").astype(np.float64)
    dofs = S.dofs_of(flat, ("h2",))
    q, qd, qdd = D.draws(flat, dofs, 3, 1)
    bound = D.rounding_bound(D.depth(flat, dofs), D.EPS32)
    site = flat.names["site"].index("tip")
    tau, M = hb.config_inverse_dynamics(dofs, dev(q[:, 0]), dev(qd[:, 0]), dev(qdd[:, 0])), hb.config_mass_matrix(dofs, dev(q[:, 0]))
    jp, jr = hb.config_jacobian(site, dofs, dev(q[:, 0]))
    assert tau.shape == (3, 1) and M.shape == (3, 1, 1) and jp.shape == (3, 3, 1) and jr.shape == (3, 3, 1)      # K = 1, 2-D q: [B, n]-style results
    got = dict(tau=tau.cpu().numpy()[:, None], M=M.cpu().numpy()[:, None], jacp=jp.cpu().numpy()[:, None], jacr=jr.cpu().numpy()[:, None])
    check("scene D, n = 1", D.errors(got, D.reference(flat, qpos, dofs, q, qd, qdd, site, overrides=over)), bound)
    dofs = D.dofs_d(flat, "all")
    q, qd, qdd = D.draws(flat, dofs, 3, 4)
    bound = D.rounding_bound(D.depth(flat, dofs), D.EPS32)
    for v, a in ((None, None), (qd, None), (None, qdd)):
        tau = hb.config_inverse_dynamics(dofs, dev(q), dev(v), dev(a)).cpu().numpy()
        check(f"scene D, qd {'given' if v is not None else 'None'}, qdd {'given' if a is not None else 'None'}",
              D.errors(dict(tau=tau), D.reference(flat, qpos, dofs, q, v, a, overrides=over, want=("tau",))), bound)


def test_sixteen_dofs():
    from tests import capacity_models

    flat = mjcf.compile_mjcf(capacity_models.model_xml(16, 1))
    dofs = S.dofs_of(flat, [f"h{i}" for i in range(16)])
    B, K = 2, 5
    hm, hb = make_hip(flat, None, B=B)
    hb.set("qpos", np.tile(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel(), (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward()
    q, qd, qdd = D.draws(flat, dofs, B, K)
    site = int(flat.nsite) - 1      # the tip
    got = ask(hb, dofs, q, qd, qdd, site)
    ref = D.oracle_reference(dynamics.model32(flat), hb.get("qpos").astype(np.float64), dofs, q, qd, qdd, site)
    check("16-hinge chain", D.errors(got, ref), D.rounding_bound(D.depth(flat, dofs), D.EPS32))
    assert np.array_equal(got["M"], np.swapaxes(got["M"], -1, -2))


# ---- consistency with the simulator's own arrays -------------------------------------------------------------------------------------------------------------
def test_consistency_with_the_state_arrays():
    from robosuite_amd.controllers import BatchState

    flat, cfg, hm, hb = lift_batch()
    dofs, site = list(range(7)), int(cfg["eef_site"])
    qvel = np.zeros((3, int(flat.nv)), dtype=np.float32)
    qvel[:, dofs] = D.rates(3, 1, 7, D.SEED_QD, 1.0)[:, 0]
    hb.set("qvel", qvel); hb.forward()
    qa = np.asarray(flat.arrays["jnt_qposadr"]).ravel()[[int(np.flatnonzero(np.asarray(flat.arrays["jnt_dofadr"]).ravel() == d)[0]) for d in dofs]]
    q, qd = hb.get("qpos")[:, qa], hb.get("qvel")[:, dofs]
    tau = hb.config_inverse_dynamics(dofs, dev(q), dev(qd)).cpu().numpy().astype(np.float64)
    M = hb.config_mass_matrix(dofs, dev(q)).cpu().numpy().astype(np.float64)
    jp, jr = (t.cpu().numpy().astype(np.float64) for t in hb.config_jacobian(site, dofs, dev(q)))
    damp = np.asarray(flat.arrays["dof_damping"], dtype=np.float32).ravel()[dofs].astype(np.float64)
    st = BatchState(hb)
    bias, qM = st.qfrc_bias.cpu().numpy().astype(np.float64)[:, dofs], st.qM.cpu().numpy().astype(np.float64)[:, dofs][:, :, dofs]
    sjp, sjr = (t.cpu().numpy().astype(np.float64)[:, :, dofs] for t in st.site_jacobian(site))
    bound = 2 * D.rounding_bound(D.depth(flat, dofs), D.EPS32)      # two fp32 evaluations of one quantity, each within the bound of it
    fig = {"qfrc_bias": np.abs(tau - damp * qd - bias).max() / np.abs(bias).max(), "qM": np.abs(M - qM).max() / np.abs(qM).max(),
           "site_jacobian": max(np.abs(jp - sjp).max(), np.abs(jr - sjr).max())}
    check("Lift, the state's own arrays", fig, bound)


# ---- purity and determinism ------------------------------------------------------------------------------------------------------------------------------
def test_pure_repeatable_and_independent_of_position():
    flat, cfg, hm, hb = lift_batch()
    dofs, site = list(range(7)), int(cfg["eef_site"])
    q, qd, qdd = (dev(x) for x in D.draws(flat, dofs, 3, 13))
    names = ("qpos", "qvel", "time", "xpos", "xquat", "qM", "qfrc_bias", "qacc", "cdof", "rootcom", "ctrl")
    before = [hb.tensor(n).clone() for n in names]
    calls = lambda q, qd, qdd: (hb.config_inverse_dynamics(dofs, q, qd, qdd), hb.config_mass_matrix(dofs, q)) + hb.config_jacobian(site, dofs, q)      # noqa: E731
    one = calls(q, qd, qdd)
    for n, a in zip(names, before):
        assert torch.equal(a, hb.tensor(n)), n      # every state tensor: the same bits
    two = calls(q, qd, qdd)
    assert all(torch.equal(a, b) for a, b in zip(one, two))      # a repeat call: the same bits
    for k in (0, 5, 12):
        row = calls(q[:, k], qd[:, k], qdd[:, k])      # K = 1 on that row: another lane, other strides, the same bits
        assert all(torch.equal(a[:, k], b) for a, b in zip(one, row)), k


def test_mass_matrix_is_symmetric_and_agrees_with_inverse_dynamics():
    flat, hm, hb, over = scene_d_batch()
    dofs = D.dofs_d(flat, "all")
    q, qd, qdd = (dev(x) for x in D.draws(flat, dofs, 5, 13))
    M = hb.config_mass_matrix(dofs, q)
    assert torch.equal(M, M.transpose(-1, -2))
    d = (hb.config_inverse_dynamics(dofs, q, qd, qdd) - hb.config_inverse_dynamics(dofs, q, qd)).double()
    want = torch.einsum("bkij,bkj->bki", M.double(), qdd.double())
    scale = float(hb.config_inverse_dynamics(dofs, q, qd, qdd).abs().max())
    assert float((d - want).abs().max()) <= 2 * D.rounding_bound(D.depth(flat, dofs), D.EPS32) * scale


# ---- the VecEnv layer ----------------------------------------------------------------------------------------------------------------------------------------
def test_vec_env_and_path_torques():
    from robosuite_amd.vec_env import VecEnv

    flat, cfg = R.lift()
    env = VecEnv("Lift", 3, flat, cfg, horizon=50)
    env.reset()
    dofs = list(range(7))
    q = dev(D.draws(flat, dofs, 3, 5)[0])
    hb = env.env.batch
    assert torch.equal(env.config_gravity_torque(q), hb.config_inverse_dynamics(dofs, q))
    assert torch.equal(env.config_mass_matrix(q), hb.config_mass_matrix(dofs, q))
    assert all(torch.equal(a, b) for a, b in zip(env.config_jacobian(q), hb.config_jacobian(int(cfg["eef_site"]), dofs, q)))
    w = dev(D.draws(flat, dofs, 3, 6)[0]).reshape(3, 2, 3, 7)      # two paths of three waypoints per env
    w = w[:, :, :1] + 0.05 * (w - w[:, :, :1])                        # ... near their first one
    dt = 0.05
    tau = env.path_torques(w, dt)
    assert tau.shape == (3, 2, 3, 7)
    qd = torch.stack([(w[:, :, 1] - w[:, :, 0]) / dt, (w[:, :, 2] - w[:, :, 0]) / (2 * dt), (w[:, :, 2] - w[:, :, 1]) / dt], dim=2)
    qdd = torch.stack([(qd[:, :, 1] - qd[:, :, 0]) / dt, (qd[:, :, 2] - qd[:, :, 0]) / (2 * dt), (qd[:, :, 2] - qd[:, :, 1]) / dt], dim=2)
    want = hb.config_inverse_dynamics(dofs, w.reshape(3, 6, 7), qd.reshape(3, 6, 7), qdd.reshape(3, 6, 7)).reshape(3, 2, 3, 7)
    # the hand-made differences and torch.gradient's may round differently: a few ulp of qdd (|qdd| dt^-2 amplified) through M; held to the parity bound
    assert float((tau - want).abs().max()) <= D.rounding_bound(D.depth(flat, dofs), D.EPS32) * float(want.abs().max())


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_by_name():
    flat, hm, hb, over = scene_d_batch(B=3)
    dofs = D.dofs_d(flat, "arm")
    q, qd, qdd = (dev(x) for x in D.draws(flat, dofs, 3, 5))
    site = flat.names["site"].index("tip")
    free_dof = int(np.asarray(flat.arrays["jnt_dofadr"]).ravel()[flat.names["joint"].index("fsj")])
    for call in (lambda d, x: hb.config_inverse_dynamics(d, x), lambda d, x: hb.config_mass_matrix(d, x), lambda d, x: hb.config_jacobian(site, d, x)):
        with pytest.raises(backend.RsimError, match="free joint"):
            call([free_dof] + dofs[1:], q)
        with pytest.raises(backend.RsimError, match="listed twice"):
            call([dofs[0]] + dofs[:2], q)
        with pytest.raises(backend.RsimError, match="shape"):
            call(dofs, q[:, :0])                                                    # K = 0 at the Python layer
        with pytest.raises(backend.RsimError, match="CUDA tensor"):
            call(dofs, q.cpu())
    ids = (C.c_int32 * 3)(*dofs)
    out = torch.empty((3, 5, 3, 3), device="cuda")
    assert hb._L.rsim_config_mass_matrix(hb.ptr, 3, ids, 0, C.c_void_p(q.data_ptr()), C.c_void_p(out.data_ptr())) != 0      # ... and at the C boundary
    assert "rsim_config_mass_matrix: k 0 < 1" in backend.lib().rsim_last_error().decode()
    with pytest.raises(backend.RsimError, match="qd must be a CUDA tensor"):
        hb.config_inverse_dynamics(dofs, q, qd.cpu())
    with pytest.raises(backend.RsimError, match="qdd must have q's shape"):
        hb.config_inverse_dynamics(dofs, q, qd, qdd[:, :4])
    with pytest.raises(backend.RsimError, match="qd must have q's shape"):
        hb.config_inverse_dynamics(dofs, q, qd[:, :, :2])
    with pytest.raises(backend.RsimError, match="rsim_config_jacobian: site 99 out of range"):
        hb.config_jacobian(99, dofs, q)
    with pytest.raises(backend.RsimError, match="rsim_config_jacobian: site -1 out of range"):
        hb.config_jacobian(-1, dofs, q)
