"""M^-1 at candidate configurations on the device (csrc/rsim_dyn_solve.hip: rsim_config_forward_dynamics, rsim_config_mass_solve, rsim_config_opspace).

  1 THE SOLVE, against numpy's fp64 solve ON THE DEVICE'S OWN INPUTS: M_dev, b_dev and J_dev are what the public calls config_mass_matrix,
    config_inverse_dynamics(q, qd) and config_jacobian return, so the bound is the solve's alone -- Higham's backward error of Cholesky, by reasoning
    (tests/dynamics_solve_scenes.py): per candidate and column ||x - x_ref|| <= 2 kappa_2(M_dev) (n (3n + 1) + 2) 2^-24 ||x_ref||, and for lambda_inv entrywise
    2 (kappa_2 n (3n + 1) + n + 2) 2^-24 ||J||^2 ||M^-1||.  Every candidate's relative bound is asserted below 5e-3 from the reference alone.  Agreement also
    proves that the launch chain feeds the solve the M, b and J those calls return.
      scene D at (5, 13) with per-env body_mass / dof_armature, arm and all dofs (65 candidates: a wavefront that spans envs and one with a single live lane; "all"
      has columns not in tree order) -- solving with env 0's tables is off by more than 100 bounds; Lift at (3, 22); the 16-hinge chain at (2, 5), the largest LDS
      footprint; n = 1 at K = 1 with 2-D tensors; r = 1, r = 16 and rhs [B, K, n]; ok true everywhere.
  2 END TO END against the fp64 statement (robosuite_amd/dynamics.py) and, for Lift and the chain, the fp64 oracle: with dM = M_dev - M_ref and db = b_dev - b_ref,
    both observable through the existing calls, ||x - x_ref|| <= ||M_ref^-1|| (||dM|| ||x|| + ||db||) + the bound of 1: the perturbation identity, no free constant.
  3 ROUND TRIP: config_forward_dynamics(q, qd, config_inverse_dynamics(q, qd, qdd)) against qdd within ||M_ref^-1|| sqrt(n) 2 beta S_tau + the bound of 1, beta =
    dynamics_scenes.rounding_bound and S_tau = max |tau|: what test_dynamics.py allows between M qdd and the difference of two torque calls.  Loose, because beta
    is; the measured figure is printed.
  4 Baxter, both arms: the arm-to-arm blocks of M^-1 are exactly zero and an arm's qdd does not see the other's torques and rates.
  5 lambda_inv is symmetric bit for bit; on Lift at the state it agrees with the float64 lines of TorchOSCPoseController.torques_from on BatchState's arrays.
  6 purity, determinism, the VecEnv / BatchState forms, refusals by name.
The not-positive-definite path is exercised on the host only (tests/test_dynamics_solve_core_host.py).  Measured figures: profiles/dyn_solve_parity.txt."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from robosuite_amd import backend, dynamics
from tests import clearance_scenes as S
from tests import dynamics_scenes as D
from tests import dynamics_solve_scenes as V
from tests import raycast_scenes as R
from tests import test_dynamics as T
from tests.util import make_hip

pytestmark = pytest.mark.gpu
dev = T.dev


def f64(t):
    return t.cpu().numpy().astype(np.float64)


# ---- the scenes: device results and references, computed once and shared (nothing below writes to them) ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict: the batch, the draws, the public calls' outputs in float64 (M, b, J), the new calls' outputs, and the fp64 references (mirror / oracle)"""
    if name in ("d_arm", "d_all"):
        flat, hm, hb, over = T.scene_d_batch(5)
        dofs, site, B, K = D.dofs_d(flat, name[2:]), flat.names["site"].index("f1_s" if name == "d_all" else "tip"), 5, 13
    elif name == "lift":
        flat, cfg, hm, hb = T.lift_batch(3)
        dofs, site, B, K, over = list(range(7)), int(cfg["eef_site"]), 3, 22, None
    else:
        flat, dofs = V.chain16()
        B, K, over, site = 2, 5, None, int(flat.nsite) - 1
        hm, hb = make_hip(flat, None, B=B)
        hb.set("qpos", np.tile(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel(), (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward()
    n = len(dofs)
    q, qd, qdd = D.draws(flat, dofs, B, K)
    tau, rhs = V.tau_draw(B, K, n), V.rhs_draw(B, K, n, 16)
    c = dict(name=name, flat=flat, hb=hb, keep=hm, over=over, dofs=dofs, site=site, B=B, K=K, n=n, q=q, qd=qd, qdd=qdd, tau=tau, rhs=rhs)
    c["M"], c["b"] = f64(hb.config_mass_matrix(dofs, dev(q))), f64(hb.config_inverse_dynamics(dofs, dev(q), dev(qd)))
    c["J"] = V.J6(*(f64(t) for t in hb.config_jacobian(site, dofs, dev(q))))
    x, ok = hb.config_forward_dynamics(dofs, dev(q), dev(qd), dev(tau), return_ok=True)
    c["fd"], c["fd_ok"] = f64(x), ok
    x, ok = hb.config_mass_solve(dofs, dev(q), dev(rhs), return_ok=True)
    c["x16"], c["x16_ok"] = f64(x), ok
    lam, mjt, ok = hb.config_opspace(site, dofs, dev(q), return_ok=True)
    c["lam32"], c["lam"], c["mjt"], c["op_ok"] = lam, f64(lam), f64(mjt), ok
    assert all(t.dtype == torch.bool and tuple(t.shape) == (B, K) for t in (c["fd_ok"], c["x16_ok"], c["op_ok"]))
    qpos = hb.get("qpos").astype(np.float64)
    c["qpos"] = qpos
    c["ref"] = D.reference(flat, qpos, dofs, q, qd, None, None, overrides=over, want=("tau", "M"))      # the statement at the fp32-rounded tables
    c["rel"] = V.solve_bound(c["M"])
    return c


CASES = ("d_arm", "d_all", "lift", "chain16")


# ---- 1: the solve on the device's own inputs ---------------------------------------------------------------------------------------------------------------
def solve_figures(c):
    """the checks of 1 on one scene -> {quantity: (worst error relative to ||x_ref||, worst share of the bound)}"""
    name, hb, dofs, q, n, B, K, M, rel = c["name"], c["hb"], c["dofs"], c["q"], c["n"], c["B"], c["K"], c["M"], c["rel"]
    assert rel.max() < V.LIMIT, (name, rel.max())      # the condition, from the reference alone
    print(f"dynamics solve {name}: kappa_2(M_dev) <= {V.kappa(M).max():.1f}")
    assert c["fd"].shape == (B, K, n) and c["x16"].shape == (B, K, n, 16) and c["lam"].shape == (B, K, 6, 6) and c["mjt"].shape == (B, K, n, 6)
    assert bool(c["fd_ok"].all()) and bool(c["x16_ok"].all()) and bool(c["op_ok"].all())
    fig = {"forward dynamics": V.hold_columns(f"{name}, forward dynamics", V.columns(c["fd"]), V.columns(V.solve(M, c["tau"] - c["b"])), rel),
           "mass solve r = 16": V.hold_columns(f"{name}, mass solve r = 16", c["x16"], V.solve(M, c["rhs"]), rel)}
    r1 = c["rhs"][..., :1]
    x1, xv = hb.config_mass_solve(dofs, dev(q), dev(r1)), hb.config_mass_solve(dofs, dev(q), dev(r1[..., 0]))
    assert tuple(x1.shape) == (B, K, n, 1) and tuple(xv.shape) == (B, K, n) and torch.equal(x1[..., 0], xv)      # rhs [B, K, n] is r = 1
    fig["mass solve r = 1"] = V.hold_columns(f"{name}, mass solve r = 1", f64(x1), V.solve(M, r1), rel)
    JT = np.swapaxes(c["J"], -1, -2)
    mjt_ref = V.solve(M, JT)
    fig["M^-1 J^T"] = V.hold_columns(f"{name}, M^-1 J^T", c["mjt"], mjt_ref, rel)
    err, bound = np.abs(c["lam"] - c["J"] @ mjt_ref).max(axis=(-2, -1)), V.lambda_bound(M, c["J"])
    print(f"dynamics solve {name}, lambda_inv: worst entry error {err.max():.3e}, {(err / bound).max():.3e} of its bound")
    assert (err <= bound).all()
    assert torch.equal(c["lam32"], c["lam32"].transpose(-1, -2))      # one product per unordered pair: symmetric bit for bit
    fig["lambda_inv (entry)"] = (float(err.max()), float((err / bound).max()))
    return fig


@pytest.mark.parametrize("name", CASES)
def test_solve_against_fp64_on_the_devices_own_inputs(name):
    c = case(name)
    solve_figures(c)
    if c["over"] is not None:      # the overrides are visible: env 0's tables are wrong for the others
        wrong = D.reference(c["flat"], c["qpos"], c["dofs"], c["q"], overrides=c["over"][0], want=("M",))["M"]
        x_wrong = V.solve(wrong, c["tau"] - c["b"])
        off = V.col_norm(V.columns(c["fd"] - x_wrong)) / V.col_norm(V.columns(x_wrong))
        print(f"dynamics solve {name}: with env 0's tables off by {off.max():.3e} ({off.max() / c['rel'].max():.0f} bounds)")
        assert off.max() > 100 * c["rel"].max()


def test_one_dof_and_two_d_tensors():
    flat, hm, hb, over = T.scene_d_batch(B=3)
    dofs = S.dofs_of(flat, ("h2",))
    site = flat.names["site"].index("tip")
    q, qd, _ = D.draws(flat, dofs, 3, 1)
    tau, rhs = V.tau_draw(3, 1, 1), V.rhs_draw(3, 1, 1, 4)
    M, b = f64(hb.config_mass_matrix(dofs, dev(q[:, 0]))), f64(hb.config_inverse_dynamics(dofs, dev(q[:, 0]), dev(qd[:, 0])))
    J = V.J6(*(f64(t) for t in hb.config_jacobian(site, dofs, dev(q[:, 0]))))
    qdd, ok = hb.config_forward_dynamics(dofs, dev(q[:, 0]), dev(qd[:, 0]), dev(tau[:, 0]), return_ok=True)
    x, xv = hb.config_mass_solve(dofs, dev(q[:, 0]), dev(rhs[:, 0])), hb.config_mass_solve(dofs, dev(q[:, 0]), dev(rhs[:, 0, :, 0]))
    lam, mjt, ok2 = hb.config_opspace(site, dofs, dev(q[:, 0]), return_ok=True)
    assert tuple(qdd.shape) == (3, 1) and tuple(ok.shape) == (3,) and tuple(x.shape) == (3, 1, 4) and tuple(xv.shape) == (3, 1)      # K = 1, 2-D q: no K axis
    assert tuple(lam.shape) == (3, 6, 6) and tuple(mjt.shape) == (3, 1, 6) and bool(ok.all()) and bool(ok2.all())
    rel = V.solve_bound(M)
    assert rel.max() < V.LIMIT
    V.hold_columns("scene D n = 1, forward dynamics", V.columns(f64(qdd)), V.columns(V.solve(M, tau[:, 0] - b)), rel)
    V.hold_columns("scene D n = 1, mass solve", f64(x), V.solve(M, rhs[:, 0]), rel)
    assert torch.equal(x[..., 0], xv)
    mjt_ref = V.solve(M, np.swapaxes(J, -1, -2))
    V.hold_columns("scene D n = 1, M^-1 J^T", f64(mjt), mjt_ref, rel)
    assert (np.abs(f64(lam) - J @ mjt_ref).max(axis=(-2, -1)) <= V.lambda_bound(M, J)).all() and torch.equal(lam, lam.transpose(-1, -2))


# ---- 2: end to end against the statement and the oracle ---------------------------------------------------------------------------------------------------------
def end_to_end(c, what, M_ref, b_ref):
    dM, db = np.linalg.norm(c["M"] - M_ref, 2, axis=(-2, -1)), np.linalg.norm(c["b"] - b_ref, axis=-1)
    minv = V.inv_norm(M_ref)
    x_ref = V.columns(V.solve(M_ref, c["tau"] - b_ref))
    extra = (minv * (dM * np.linalg.norm(c["fd"], axis=-1) + db))[..., None] + c["rel"][..., None] * V.col_norm(x_ref)
    fd = V.hold_columns(f"{c['name']} against {what}, forward dynamics", V.columns(c["fd"]), x_ref, np.zeros_like(c["rel"]), extra)
    x_ref = V.solve(M_ref, c["rhs"])
    extra = (minv * dM)[..., None] * V.col_norm(c["x16"]) + c["rel"][..., None] * V.col_norm(x_ref)
    return fd, V.hold_columns(f"{c['name']} against {what}, mass solve", c["x16"], x_ref, np.zeros_like(c["rel"]), extra)


@pytest.mark.parametrize("name", CASES)
def test_end_to_end_against_the_statement(name):
    c = case(name)
    end_to_end(c, "the fp64 statement", c["ref"]["M"], c["ref"]["tau"])


@pytest.mark.parametrize("name", ("lift", "chain16"))
def test_end_to_end_against_the_oracle(name):
    c = case(name)
    ref = D.oracle_reference(dynamics.model32(c["flat"]), c["qpos"], c["dofs"], c["q"], c["qd"], None)
    end_to_end(c, "the oracle", ref["M"], ref["tau"])


# ---- 3: round trip ---------------------------------------------------------------------------------------------------------------------------------------------
def round_trip_figures(c):
    """-> (worst ||qdd' - qdd|| relative to ||qdd||, worst share of the allowance)"""
    name, hb, dofs, q, qd, qdd, n, M = c["name"], c["hb"], c["dofs"], c["q"], c["qd"], c["qdd"], c["n"], c["M"]
    tau = hb.config_inverse_dynamics(dofs, dev(q), dev(qd), dev(qdd))
    back = f64(hb.config_forward_dynamics(dofs, dev(q), dev(qd), tau))
    beta, s_tau = D.rounding_bound(D.depth(c["flat"], dofs), D.EPS32), float(tau.abs().max())
    x_ref = V.columns(V.solve(M, f64(tau) - c["b"]))
    extra = (V.inv_norm(c["ref"]["M"]) * np.sqrt(n) * 2 * beta * s_tau)[..., None] + c["rel"][..., None] * V.col_norm(x_ref)
    err = V.col_norm(V.columns(back - qdd))
    print(f"dynamics solve {name}, round trip: worst ||qdd' - qdd|| {err.max():.3e} (|qdd| <= {D.QDD_MAX}), allowance {extra.min():.3e} .. {extra.max():.3e}")
    return V.hold_columns(f"{name}, round trip", V.columns(back), V.columns(qdd), np.zeros_like(c["rel"]), extra)


@pytest.mark.parametrize("name", CASES)
def test_round_trip_through_inverse_dynamics(name):
    c = case(name)
    hb, dofs, q = c["hb"], c["dofs"], c["q"]
    round_trip_figures(c)
    g = f64(hb.config_inverse_dynamics(dofs, dev(q)))
    free = f64(hb.config_forward_dynamics(dofs, dev(q)))      # tau = None, qd = None: the free fall of the locked mechanism
    V.hold_columns(f"{name}, -M^-1 gravity torque", V.columns(free), V.columns(V.solve(c["M"], -g)), c["rel"])


# ---- 4: Baxter, both arms in one call ------------------------------------------------------------------------------------------------------------------------
def test_baxter_arms_do_not_see_each_other():
    flat, cfg = T.baxter()
    dofs, B, K = list(range(14)), 2, 33
    hm, hb = make_hip(flat, cfg, B=B)
    hb.set("qpos", np.tile(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel(), (B, 1)).astype(np.float32)); hb.set("qvel", 0); hb.forward()
    q, qd, _ = D.draws(flat, dofs, B, K)
    tau = V.tau_draw(B, K, 14)
    eye = torch.eye(14, device="cuda").expand(B, K, 14, 14)
    Minv, ok = hb.config_mass_solve(dofs, dev(q), eye, return_ok=True)
    assert bool(ok.all())
    assert not Minv[..., :7, 7:].any() and not Minv[..., 7:, :7].any()      # the arm-to-arm blocks: exactly zero
    assert float(Minv[..., :7, :7].abs().amax(dim=(-2, -1)).min()) > 0 and float(Minv[..., 7:, 7:].abs().amax(dim=(-2, -1)).min()) > 0
    M = f64(hb.config_mass_matrix(dofs, dev(q)))
    rel = V.solve_bound(M)      # (kappa_2 of a Baxter arm is in the hundreds: the bound holds as it stands, the 5e-3 condition of the scenes above is not claimed)
    print(f"dynamics solve Baxter: kappa_2(M_dev) <= {V.kappa(M).max():.1f}")
    V.hold_columns("Baxter, M^-1", f64(Minv), V.solve(M, np.broadcast_to(np.eye(14), M.shape)), rel)
    one = hb.config_forward_dynamics(dofs, dev(q), dev(qd), dev(tau))
    qd2, tau2 = qd.copy(), tau.copy()
    qd2[..., 7:] *= -0.5; tau2[..., 7:] += 3.0      # other rates and torques for the second arm ...
    two = hb.config_forward_dynamics(dofs, dev(q), dev(qd2), dev(tau2))
    assert torch.equal(one[..., :7], two[..., :7])      # ... and the first arm's accelerations are the same bits
    assert float((one[..., 7:] - two[..., 7:]).abs().max()) > 0.1


# ---- 5: the controller's float64 lines on the state's own arrays -----------------------------------------------------------------------------------------------
def test_lift_at_the_state_agrees_with_the_plugin_controllers_lines():
    from robosuite_amd.controllers import BatchState

    flat, cfg, hm, hb = T.lift_batch()
    dofs, site = list(range(7)), int(cfg["eef_site"])
    qa = np.asarray(flat.arrays["jnt_qposadr"]).ravel()[[int(np.flatnonzero(np.asarray(flat.arrays["jnt_dofadr"]).ravel() == d)[0]) for d in dofs]]
    q = dev(hb.get("qpos")[:, qa])
    st = BatchState(hb)
    lam, mjt = st.config_opspace(site, dofs, q)      # K = 1, 2-D q
    assert tuple(lam.shape) == (3, 6, 6) and tuple(mjt.shape) == (3, 7, 6) and torch.equal(lam, lam.transpose(-1, -2))
    # TorchOSCPoseController.torques_from, its float64 lines, on the arm block of qM (qM covers every dof) and the arm's columns of site_jacobian
    Mr = st.qM.double()[:, dofs][:, :, dofs]
    Jr = torch.cat([t.double()[:, :, dofs] for t in st.site_jacobian(site)], dim=1)
    Minv = torch.linalg.inv(Mr)
    MiJT = torch.einsum("bij,bkj->bik", Minv, Jr)
    lfi = torch.einsum("bij,bjk->bik", Jr, MiJT)
    Mr, Jr, MiJT, lfi = (t.cpu().numpy() for t in (Mr, Jr, MiJT, lfi))
    Md, Jd = f64(hb.config_mass_matrix(dofs, q)), V.J6(*(f64(t) for t in hb.config_jacobian(site, dofs, q)))
    # M_ref (x - x_ref) = -dM x + dJ^T per column, then lambda_inv - lfi = J_dev (x - x_ref) + dJ x_ref: the observed input differences, no free constant
    rel, minv = V.solve_bound(Md), V.inv_norm(Mr)
    dM, dJ = np.linalg.norm(Md - Mr, 2, axis=(-2, -1)), Jd - Jr
    dx = (minv * dM)[..., None] * V.col_norm(f64(mjt)) + minv[..., None] * np.linalg.norm(dJ, axis=-1)      # [B, 6]
    V.hold_columns("Lift at the state, M^-1 J^T against the controller's", f64(mjt), MiJT, np.zeros_like(rel), dx + rel[..., None] * V.col_norm(MiJT))
    allow = np.linalg.norm(Jd, axis=-1)[..., :, None] * dx[..., None, :] + np.linalg.norm(dJ, axis=-1)[..., :, None] * V.col_norm(MiJT)[..., None, :]
    allow = allow + V.lambda_bound(Md, Jd)[..., None, None]
    err = np.abs(f64(lam) - lfi)
    print(f"dynamics solve Lift at the state, lambda_inv against the controller's: worst entry error {err.max():.3e}, {(err / allow).max():.3e} of its allowance")
    assert (err <= allow).all()


# ---- 6: purity, determinism, the layers, refusals ------------------------------------------------------------------------------------------------------------
def test_pure_repeatable_and_independent_of_position():
    flat, cfg, hm, hb = T.lift_batch()
    dofs, site = list(range(7)), int(cfg["eef_site"])
    q, qd, _ = (dev(x) for x in D.draws(flat, dofs, 3, 13))
    tau, rhs = dev(V.tau_draw(3, 13, 7)), dev(V.rhs_draw(3, 13, 7, 3))
    names = ("qpos", "qvel", "time", "xpos", "xquat", "qM", "qfrc_bias", "qacc", "cdof", "rootcom", "ctrl")
    before = [hb.tensor(n).clone() for n in names]
    calls = lambda q, qd, tau, rhs: (hb.config_forward_dynamics(dofs, q, qd, tau), hb.config_mass_solve(dofs, q, rhs)) + hb.config_opspace(site, dofs, q)      # noqa: E731
    one = calls(q, qd, tau, rhs)
    for n, a in zip(names, before):
        assert torch.equal(a, hb.tensor(n)), n      # every state tensor: the same bits
    two = calls(q, qd, tau, rhs)
    assert all(torch.equal(a, b) for a, b in zip(one, two))      # a repeat call: the same bits
    for k in (0, 5, 12):
        row = calls(q[:, k], qd[:, k], tau[:, k], rhs[:, k])      # K = 1 on that row: another lane, other strides, the same bits
        assert all(torch.equal(a[:, k], b) for a, b in zip(one, row)), k


def test_vec_env_and_batch_state_forms():
    from robosuite_amd.controllers import BatchState
    from robosuite_amd.vec_env import VecEnv

    flat, cfg = R.lift()
    env = VecEnv("Lift", 3, flat, cfg, horizon=50)
    env.reset()
    dofs, site = list(range(7)), int(cfg["eef_site"])
    q, qd, _ = (dev(x) for x in D.draws(flat, dofs, 3, 5))
    tau, rhs = dev(V.tau_draw(3, 5, 7)), dev(V.rhs_draw(3, 5, 7, 2))
    hb = env.env.batch
    st = BatchState(hb)
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))      # noqa: E731
    want = hb.config_forward_dynamics(dofs, q, qd, tau, return_ok=True)
    assert same(env.config_forward_dynamics(q, qd, tau, return_ok=True), want) and same(st.config_forward_dynamics(dofs, q, qd, tau, return_ok=True), want)
    assert torch.equal(env.config_forward_dynamics(q, qd=qd, tau=tau, arm=0), want[0])
    want = hb.config_mass_solve(dofs, q, rhs, return_ok=True)
    assert same(env.config_mass_solve(q, rhs, return_ok=True), want) and same(st.config_mass_solve(dofs, q, rhs, return_ok=True), want)
    want = hb.config_opspace(site, dofs, q, return_ok=True)
    assert same(env.config_opspace(q, return_ok=True), want) and same(st.config_opspace(site, dofs, q, return_ok=True), want)
    assert same(env.config_opspace(q, arm=0, site=site), want[:2])
    with pytest.raises(backend.RsimError, match="CUDA tensor"):
        env.config_forward_dynamics(q.cpu())
    with pytest.raises(backend.RsimError, match="tau must have q's shape"):
        env.config_forward_dynamics(q, tau=tau[:, :2])
    with pytest.raises(backend.RsimError, match="rhs must have shape"):
        env.config_mass_solve(q, rhs[:, :2])
    with pytest.raises(backend.RsimError, match="rsim_config_opspace: site 99 out of range"):
        env.config_opspace(q, site=99)
    with pytest.raises(backend.RsimError, match="listed twice"):
        st.config_mass_solve([0, 0, 1], q[..., :3], rhs[:, :, :3])


def test_refusals_by_name():
    flat, hm, hb, over = T.scene_d_batch(B=3)
    dofs = D.dofs_d(flat, "arm")
    q, qd, _ = (dev(x) for x in D.draws(flat, dofs, 3, 5))
    tau, rhs = dev(V.tau_draw(3, 5, 3)), dev(V.rhs_draw(3, 5, 3, 2))
    site = flat.names["site"].index("tip")
    free_dof = int(np.asarray(flat.arrays["jnt_dofadr"]).ravel()[flat.names["joint"].index("fsj")])
    for call in (lambda d, x: hb.config_forward_dynamics(d, x), lambda d, x: hb.config_mass_solve(d, x, rhs[:, :x.shape[1]]),
                 lambda d, x: hb.config_opspace(site, d, x)):
        with pytest.raises(backend.RsimError, match="free joint"):
            call([free_dof] + dofs[1:], q)
        with pytest.raises(backend.RsimError, match="listed twice"):
            call([dofs[0]] + dofs[:2], q)
        with pytest.raises(backend.RsimError, match="shape"):
            call(dofs, q[:, :0])                                                    # K = 0 at the Python layer
        with pytest.raises(backend.RsimError, match="CUDA tensor"):
            call(dofs, q.cpu())
    ids = (C.c_int32 * 3)(*dofs)
    vp = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    out, ok = torch.empty((3, 5, 3, 16), device="cuda"), torch.empty((3, 5), dtype=torch.int32, device="cuda")
    L, err = hb._L, lambda: backend.lib().rsim_last_error().decode()      # noqa: E731
    assert L.rsim_config_forward_dynamics(hb.ptr, 3, ids, 0, vp(q), None, None, vp(out), None) != 0      # ... and at the C boundary
    assert "rsim_config_forward_dynamics: k 0 < 1" in err()
    assert L.rsim_config_forward_dynamics(hb.ptr, 3, ids, 5, vp(q), None, None, None, vp(ok)) != 0
    assert "rsim_config_forward_dynamics: qdd_dev is NULL" in err()
    for r in (0, 17):
        assert L.rsim_config_mass_solve(hb.ptr, 3, ids, 5, vp(q), r, vp(out), vp(out), None) != 0
        assert f"rsim_config_mass_solve: nrhs {r} out of range (1..16)" in err()
    assert L.rsim_config_mass_solve(hb.ptr, 3, ids, 5, vp(q), 2, None, vp(out), None) != 0
    assert "rsim_config_mass_solve: rhs_dev is NULL" in err()
    assert L.rsim_config_opspace(hb.ptr, site, 3, ids, 5, vp(q), None, None, vp(ok)) != 0
    assert "rsim_config_opspace: lambda_inv_dev and minv_jt_dev are both NULL" in err()
    assert L.rsim_config_opspace(hb.ptr, site, 3, ids, 5, vp(q), vp(out), None, None) == 0      # either output alone, ok optional
    lam_only = out.flatten()[:3 * 5 * 36].reshape(3, 5, 6, 6).clone()
    assert L.rsim_config_opspace(hb.ptr, site, 3, ids, 5, vp(q), None, vp(out), None) == 0
    lam, mjt = hb.config_opspace(site, dofs, q)
    assert torch.equal(lam_only, lam) and torch.equal(out.flatten()[:3 * 5 * 3 * 6].reshape(3, 5, 3, 6), mjt)
    with pytest.raises(backend.RsimError, match="qd must be a CUDA tensor"):
        hb.config_forward_dynamics(dofs, q, qd.cpu())
    with pytest.raises(backend.RsimError, match="tau must have q's shape"):
        hb.config_forward_dynamics(dofs, q, qd, tau[:, :4])
    with pytest.raises(backend.RsimError, match="rhs must be a CUDA tensor"):
        hb.config_mass_solve(dofs, q, rhs.cpu())
    with pytest.raises(backend.RsimError, match="rhs must have shape"):
        hb.config_mass_solve(dofs, q, rhs[:, :, :2])
    with pytest.raises(backend.RsimError, match="rhs must have shape"):
        hb.config_mass_solve(dofs, q, rhs[..., None])
    with pytest.raises(backend.RsimError, match=r"nrhs 17 out of range \(1..16\)"):
        hb.config_mass_solve(dofs, q, torch.zeros((3, 5, 3, 17), device="cuda"))
    with pytest.raises(backend.RsimError, match="rsim_config_opspace: site 99 out of range"):
        hb.config_opspace(99, dofs, q)
    with pytest.raises(backend.RsimError, match="rsim_config_opspace: site -1 out of range"):
        hb.config_opspace(-1, dofs, q)
