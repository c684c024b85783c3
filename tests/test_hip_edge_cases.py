"""-m gpu: edge cases of the HIP path against the oracle -- odd batch sizes, out-of-range actions, joint limits, the cube leaving the table
(plane contacts, free fall), masked resets.  Same tolerances as tests/test_hip_parity.py."""
import numpy as np
import pytest
import torch

from tests.util import load_golden, make_hip, make_oracle

pytestmark = pytest.mark.gpu


def _start(g, flat, od, oc, hb, B, q=None, v=None):
    nq = flat.nq
    s0 = g["states"][0]
    q = s0[1:1 + nq] if q is None else q
    v = np.zeros(flat.nv) if v is None else v
    od.qpos[:] = q; od.qvel[:] = v; od.qacc_warmstart[:] = 0; od.ctrl[:] = 0; od.forward()
    if oc is not None:
        oc.reset(od)
    hb.set("qpos", q[None].repeat(B, 0)); hb.set("qvel", v[None].repeat(B, 0)); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
    hb.forward(); hb.ctrl_reset()


@pytest.mark.parametrize("B", (1, 3, 4097))
def test_batch_sizes_that_are_not_round(B):
    """Every env of a batch of any size gets the same answer as env 0 (one workgroup per env, no cross-env state)."""
    g, cfg, flat = load_golden("seed1_full")
    om, od, oc = make_oracle(flat, cfg)
    hm, hb = make_hip(flat, cfg, B=B)
    _start(g, flat, od, oc, hb, B)
    for t in range(3):
        hb.control_step(torch.tensor(np.repeat(g["actions"][t][None], B, 0), dtype=torch.float32, device="cuda"), 25)
        oc.env_step(od, g["actions"][t], 25)
    q = hb.get("qpos")
    assert np.abs(q[0] - od.qpos).max() < 5e-5
    assert (q == q[0]).all()


def test_out_of_range_actions_are_clipped_like_the_reference():
    """Controller.scale_action clips to [input_min, input_max] first (controller.py:149-168): +-10 behaves as +-1, and the gripper takes only the sign."""
    g, cfg, flat = load_golden("seed1_full")
    hm, hb = make_hip(flat, cfg, B=2)
    om, od, oc = make_oracle(flat, cfg)
    _start(g, flat, od, oc, hb, 2)
    a = np.array([[1, -1, 1, -1, 1, -1, 1], [10, -10, 10, -10, 10, -10, 0.01]], dtype=np.float32)
    for t in range(4):
        hb.control_step(torch.tensor(a, device="cuda"), 25)
    q = hb.get("qpos")
    assert np.array_equal(q[0], q[1])


def test_joint_limits_engage():
    """Arm started next to two joint limits and commanded into them (JOINT_POSITION): limit rows against the oracle."""
    g, cfg, flat = load_golden("ctl_joint_position")
    nq = flat.nq
    om, od, oc = make_oracle(flat, cfg)
    hm, hb = make_hip(flat, cfg, B=2)
    q = g["states"][0][1:1 + nq].copy()
    lo, hi = flat.jnt_range[:7, 0], flat.jnt_range[:7, 1]
    q[3], q[5] = hi[3] - 0.01, hi[5] - 0.01
    _start(g, flat, od, oc, hb, 2, q)
    a = np.array([0, 0, 0, 1, 0, 1, 0, 0.0])
    hit = 0
    for t in range(12):
        hb.control_step(torch.tensor(np.repeat(a[None], 2, 0), dtype=torch.float32, device="cuda"), 25)
        oc.env_step(od, a, 25)
        assert np.abs(hb.get("qpos")[0] - od.qpos).max() < 5e-4 and np.abs(hb.get("qvel")[0] - od.qvel).max() < 5e-3, t
        hit += int(od.qpos[3] > hi[3] - 1e-3 or od.qpos[5] > hi[5] - 1e-3)
    assert hit > 0     # a joint sat on (or slightly past) its soft limit


def test_cube_sliding_off_the_table_and_landing_on_the_floor():
    """Free flight, then plane-box contacts with the floor (a pair type the table-top episodes never exercise)."""
    g, cfg, flat = load_golden("seed1_full")
    nq = flat.nq
    om, od, oc = make_oracle(flat, cfg)
    hm, hb = make_hip(flat, cfg, B=2)
    q = g["states"][0][1:1 + nq].copy()
    q[9:12] = [0.55, 0.0, 0.84]           # beyond the table edge (half extent 0.4), slightly above it
    v = np.zeros(flat.nv); v[9] = 0.6; v[13] = 2.0
    _start(g, flat, od, oc, hb, 2, q, v)
    zero = np.zeros(7)
    seen_floor = False
    for t in range(14):                   # 0.7 s: falls 0.8 m, lands, tumbles
        hb.control_step(torch.tensor(np.repeat(zero[None], 2, 0), dtype=torch.float32, device="cuda"), 25)
        oc.env_step(od, zero, 25)
        assert np.isfinite(hb.get("qvel")).all()
        if t < 7:                         # flight: tight agreement
            assert np.abs(hb.get("qpos")[0] - od.qpos).max() < 1e-4, t
        floor = flat.names["geom"].index("floor")
        seen_floor |= any(c["geom1"] == floor or c["geom2"] == floor for c in od.contacts())
    assert seen_floor and od.qpos[11] < 0.1
    assert abs(hb.get("qpos")[0][11] - od.qpos[11]) < 5e-3       # both came to rest on the floor (tumbling decorrelates the rest of the pose)


def test_masked_reset_touches_only_the_selected_envs():
    g, cfg, flat = load_golden("seed1_full")
    om, od, oc = make_oracle(flat, cfg)
    hm, hb = make_hip(flat, cfg, B=4)
    _start(g, flat, od, oc, hb, 4)
    for t in range(2):
        hb.control_step(torch.tensor(np.repeat(g["actions"][t][None], 4, 0), dtype=torch.float32, device="cuda"), 25)
    before = hb.get("qpos").copy()
    hb.reset(mask=np.array([0, 1, 0, 1], dtype=np.uint8))
    after = hb.get("qpos")
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])
    assert np.allclose(after[1], flat.qpos0, atol=1e-6) and np.allclose(after[3], flat.qpos0, atol=1e-6)
    assert hb.get("time")[1] == 0 and hb.get("time")[0] > 0


@pytest.mark.parametrize("name,tag,model", (("Lift", "seed1_full", "lift_panda"), ("Stack", "seed0_full", "stack_panda"),
                                            ("TwoArmPegInHole", "ctl_joint_position", "peg_baxter"), ("PickPlace", "seed0_full", "pickplace_iiwa")))
def test_long_random_rollouts_stay_finite_on_every_configuration(name, tag, model):
    """150 control steps (3750 substeps) of full-range random actions on 128 differently seeded envs per kernel configuration, with the episode
    horizon inside the run (on-device restart): no env diverges, rewards stay in [0, 1], dones fire exactly at the horizon."""
    from robosuite_amd.vec_env import VecEnv
    g, cfg, flat = load_golden(tag, model)
    if name == "Lift":
        cfg = dict(cfg); cfg.setdefault("obs_keys", ["all"]); cfg.setdefault("obs_dims", [60])
    B = 128
    env = VecEnv(name, B, flat, cfg, seed=0, horizon=100, bank_episodes=2)
    env.reset()
    gen = torch.Generator(device="cuda"); gen.manual_seed(5)
    ndone = 0
    for t in range(150):
        a = torch.rand(B, env.action_dim, device="cuda", generator=gen) * 2 - 1
        obs, rew, done, info = env.step(a)
        ndone += int(done.sum().item())
        if t % 50 == 49:
            assert torch.isfinite(obs).all() and torch.isfinite(rew).all(), t
            assert float(rew.min()) >= 0.0 and float(rew.max()) <= 1.0 + 1e-6
    assert ndone == B                                  # one horizon crossing per env
    assert np.isfinite(env.env.batch.get("qpos")).all() and np.isfinite(env.env.batch.get("qvel")).all()
    # MuJoCo's bad-state guard (RSIM_DIVERGED) must stay silent on every configuration, PickPlace included (the closed Robotiq gripper rammed into
    # the bins with 80 constraint rows used to lose 1 env in 128: constraint forces good to 1 % only in fp32, divided by 5e-5 kg m^2 in the
    # integrator; the Euler step now integrates the solver's acceleration)
    assert int((env.env.batch.get("diverged") > 0).sum()) == 0


def test_contact_and_row_overflow_is_counted_not_silent():
    """MuJoCo's nconmax = 5000 (models/assets/base.xml:5) never truncates; the fused kernel has 16 contact slots and 64 constraint rows in the
    Lift configuration.  A constructed state (cube jammed between the closed finger pads, the hand and the table: 26 contacts, 94 rows on the
    oracle) must come out as the FIRST 16 contacts in detection order, a row count within capacity, finite accelerations -- and a non-zero
    RSIM_OVERFLOW count, which the bench reports as `overflow_envs`."""
    from tests.util import load_golden, make_hip, make_oracle
    g, cfg, flat = load_golden("seed1_full")
    q = np.array([-3.310503761e-03, 9.595607741e-01, -4.905636198e-03, -2.424200342e+00, 9.327601525e-03, 3.760863028e+00, 8.123742675e-01, 5.613262166e-05,
                  -5.613262166e-05, -1.113625582e-01, 4.773980294e-03, 8.007105292e-01, 9.982068450e-01, -2.683816807e-02, 1.416109385e-02, 5.159719647e-02])
    om, od, _ = make_oracle(flat, cfg)
    od.qpos[:] = q; od.qvel[:] = 0; od.qacc_warmstart[:] = 0; od.ctrl[:] = 0; od.forward()
    assert od.ncon > 16 and od.nefc > 64
    hm, hb = make_hip(flat, cfg, B=2)
    assert int(hb.get("overflow").sum()) == 0
    hb.set("qpos", np.stack([q, flat.qpos0.ravel()])); hb.set("qvel", 0); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
    hb.forward()
    ov = hb.get("overflow")
    assert hb.get("ncon")[0] == hb.maxcon == 16 and hb.get("nefc")[0] <= hb.maxefc == 64
    # dropped contacts (and the contact blocks whose rows no longer fit) are counted, for env 0 only; one contact of this jammed state sits on
    # a margin boundary and exists in fp64 only
    assert ov[0] >= od.ncon - 16 - 2 and ov[1] == 0
    # order-preserving truncation: the kernel's 16 contacts are, in order, a subsequence of the head of the oracle's list (the knife-edge
    # contact above may be missing from it)
    it = iter([(b["geom1"], b["geom2"], b["dim"]) for b in od.contacts()[:19]])
    assert all(any(key == o for o in it) for key in [(a["geom1"], a["geom2"], a["dim"]) for a in hb.contacts(0)])
    assert np.isfinite(hb.get("qacc")).all()
    hb.forward()
    assert hb.get("overflow")[0] == 2 * ov[0]                         # the counter accumulates over launches


@pytest.mark.parametrize("groups,dr", ((3, False), (8, False), (4, True)))
def test_stream_groups_do_not_change_any_result(groups, dr):
    """rsim_set_stream_groups: the batch stepped as env blocks on their own HIP streams reaches bit-identical states, observations, rewards and
    episode counters -- through on-device episode resets (horizon 7), a mid-rollout read (which has to wait for every block) and a block count
    that does not divide the batch; dr: with the dynamics re-drawn before every control step (each block re-draws and rebuilds its own constant
    blocks on its own stream)."""
    import json, os
    from robosuite_amd import lift, mjcf
    adir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "assets")
    flat = mjcf.load_model(os.path.join(adir, "lift_panda.rsim")); cfg = json.load(open(os.path.join(adir, "lift_panda.cfg.json")))
    B, T = 250, 20
    ids = np.arange(B)
    tape = torch.tensor(lift.env_actions(ids, T), device="cuda")
    out = []
    for G in (1, groups):
        env = lift.LiftBatch(flat, cfg, ids, seed0=0, horizon=7, bank_episodes=4)
        env.batch.set_stream_groups(G)
        if dr:
            env.batch.dr_save_defaults()
        mid = None
        for t in range(T):
            if dr:
                env.batch.randomize_dynamics(seed=3, step=t)
            env.step(tape[t])
            if t == 9:
                mid = env.batch.get("qpos")
        env.batch.sync()
        out.append({k: env.batch.get(k) for k in ("qpos", "qvel", "obs", "reward", "ep_index", "ep_step", "terminal_obs", "bank_stale")} | {"mid": mid})
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
    assert out[0]["ep_index"].min() >= 2 and out[0]["bank_stale"].sum() == 0


def test_friction_cone_on_the_device_matches_coulomb():
    """The same known answer from mechanics as tests/test_oracle.py, on the fp32 kernel: gravity tilted by theta, cube friction mu = 0.3 -- at rest below
    tan(theta) = mu, sliding with a = g (sin(theta) - mu cos(theta)) above."""
    g, cfg, flat = load_golden("seed0_gentle")
    cube, table = flat.name2id("geom", "cube_g0"), flat.name2id("geom", "table_collision")
    mu = 0.3
    for fac, slides in ((0.5, False), (0.9, False), (1.2, True), (2.0, True)):
        th = np.arctan(fac * mu)
        f2 = flat.copy()
        f2.arrays["gravity"][:] = 9.81 * np.array([np.sin(th), 0.0, -np.cos(th)]); f2.arrays["density"][:] = 0; f2.arrays["viscosity"][:] = 0
        f2.arrays["geom_friction"][cube][0] = mu; f2.arrays["geom_friction"][table][0] = mu
        hm, hb = make_hip(f2, None, B=1)
        hb.set("qpos", g["states"][0][1:1 + flat.nq][None]); hb.set("qvel", 0); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
        vx = []
        for _ in range(150):
            hb.step1()
            c = np.zeros(flat.nu); c[:7] = hb.get("qfrc_bias")[0][:7]; c[7:9] = [0.04, -0.04]
            hb.set("ctrl", c[None])
            hb.step2()
            vx.append(float(hb.get("qvel")[0][9]))
        if not slides:
            assert abs(vx[-1]) < 1e-3 and hb.get("ncon")[0] == 4, (fac, vx[-1])
        else:
            # mean acceleration over the last 50 substeps.  The sliding cube chatters on its four soft corner contacts (0 - 4 of them per substep), so a 0.1 s window
            # carries a few per cent of noise around Coulomb's value: fp64 oracle -2.5 %, this kernel +4 % (round 4) / +6.7 % (round 5 build) at 1.2 x the friction angle
            # (tools/friction_probe.py); well clear of the frictionless g sin(theta) (+240 %) and of sticking
            a = (vx[-1] - vx[-51]) / (50 * 0.002)
            assert a == pytest.approx(9.81 * (np.sin(th) - mu * np.cos(th)), rel=0.09), (fac, a)


def test_gymnasium_vector_shaped_facade():
    """GymVecEnv: reset / step signatures and conventions of gymnasium.vector with the reference GymWrapper's flattening (object keys, then robot keys),
    autoreset with the finished episode's last observation in info["final_observation"]."""
    from robosuite_amd.vec_env import GymVecEnv, VecEnv
    g, cfg, flat = load_golden("seed0_full", "stack_panda")
    B = 8
    venv = VecEnv("Stack", B, flat, cfg, seed=0, horizon=3, bank_episodes=4)
    genv = GymVecEnv(venv)
    obs, info = genv.reset(seed=0)
    assert info == {} and tuple(obs.shape) == (B, venv.obs_dim) == genv.observation_space.shape and genv.single_action_space.shape == (venv.action_dim,)
    raw = venv.env.obs()
    nobj = sum(cfg["obs_dims"][i] for i, k in enumerate(cfg["obs_keys"]) if not k.startswith("robot0_"))
    k0 = next(k for k in cfg["obs_keys"] if not k.startswith("robot0_"))
    assert torch.equal(obs[:, :cfg["obs_dims"][cfg["obs_keys"].index(k0)]], venv.key(raw, k0)) and nobj > 0     # object-state first
    a = torch.zeros(B, venv.action_dim, device="cuda")
    for t in range(3):
        obs, rew, term, trunc, info = genv.step(a)
        assert tuple(rew.shape) == (B,) and term.dtype == torch.bool and not trunc.any()
    assert term.all() and info["_final_observation"].all() and tuple(info["final_observation"].shape) == tuple(obs.shape)
    assert not torch.equal(info["final_observation"], obs)                 # obs is the next episode's reset observation
    with pytest.raises(TypeError):
        genv.reset(seed="0")


def _lift_assets():
    import json, os
    from robosuite_amd import mjcf
    adir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "assets")
    return mjcf.load_model(os.path.join(adir, "lift_panda.rsim")), json.load(open(os.path.join(adir, "lift_panda.cfg.json")))


def test_asynchronous_ring_upkeep_keeps_every_reset_a_fresh_draw():
    """The upkeep thread (reset_bank.py: asynchronous poll of the episode counters + pinned-staging refill on a side stream) keeps the ring ahead
    of the envs without the stepping thread ever reading the device: episode k of env i is still episode_setup(seed, i, k) after several ring
    revolutions, no reset found a stale slot, and step() spent (next to) no time on the upkeep."""
    from robosuite_amd import lift
    flat, cfg = _lift_assets()
    ids = np.array([2, 9, 300, 2047, 4095])
    H, E, T = 40, 3, 40 * 7
    env = lift.LiftBatch(flat, cfg, ids, seed0=5, horizon=H, bank_episodes=E)
    env.bank_poll_steps = 8
    acts = torch.tensor(lift.env_actions(ids, T, scale=0.3), device="cuda")
    for t in range(T):
        env.step(acts[t])
        if (t + 1) % H == 0:
            k = (t + 1) // H
            env.batch.sync()
            assert env.batch.get("ep_index").tolist() == [k] * len(ids)
            sizes, qpos = lift.episode_setup(5, ids, k)
            assert np.array_equal(env.batch.get("qpos"), qpos.astype(np.float32)), k
    env.bank_quiesce()
    st = env.bank_stats()
    assert int(env.batch.get("bank_stale").sum()) == 0
    assert st["polls"] >= 7 and st["rows"] >= 7 * len(ids) - len(ids) and env._bank_thread is not None
    assert st["tick_ms_per_1000_steps"] < 50.0, st       # the stepping thread only counts steps and sets an event


def test_reset_after_the_ring_has_moved_on_starts_the_episode_streams_again():
    """VecEnv.reset() re-installs the ring (round-2 review): after envs have run past their horizon a reset() must put episode 0 back and the
    next on-device reset must be episode 1 again, not whatever the ring held; a different seed re-keys the streams."""
    from robosuite_amd import lift
    flat, cfg = _lift_assets()
    env = lift.LiftVecEnv(5, seed=2, horizon=3, bank_episodes=2)
    a = torch.zeros(5, 7, device="cuda")
    for t in range(3 * 3 + 1):
        env.step(a)
    assert env.env.batch.get("ep_index").tolist() == [3] * 5
    env.reset()
    q0 = lift.episode_setup(2, np.arange(5), 0)[1].astype(np.float32)
    assert np.array_equal(env.env.batch.get("qpos"), q0) and env.env.batch.get("ep_index").tolist() == [0] * 5
    for t in range(3):
        env.step(a)
    q1 = lift.episode_setup(2, np.arange(5), 1)[1].astype(np.float32)
    assert np.array_equal(env.env.batch.get("qpos"), q1)
    for t in range(3):
        env.step(a)
    assert np.array_equal(env.env.batch.get("qpos"), lift.episode_setup(2, np.arange(5), 2)[1].astype(np.float32))
    assert int(env.env.batch.get("bank_stale").sum()) == 0
    env.reset(seed=11)
    assert np.array_equal(env.env.batch.get("qpos"), lift.episode_setup(11, np.arange(5), 0)[1].astype(np.float32))
    for t in range(3):
        env.step(a)
    assert np.array_equal(env.env.batch.get("qpos"), lift.episode_setup(11, np.arange(5), 1)[1].astype(np.float32))


def _contact_rich_rollout(B, T, warm="all", groups=1, keep=False, env_vars=None):
    """Lift envs under full-range random actions (hands on the table: the MPR- and Newton-heavy states).  warm: "all" = separating-direction and
    portal warm start of the convex narrow phase (the default build), "exact" = separating direction only, "none" = every run cold."""
    import os
    from robosuite_amd import lift
    flat, cfg = _lift_assets()
    ids = np.arange(B)
    tape = torch.tensor(lift.env_actions(ids, T), device="cuda")
    var = {"none": "RSIM_NO_MPR_WARMSTART", "exact": "RSIM_NO_MPR_PORTAL_WARMSTART"}.get(warm)
    env_vars = dict(env_vars or {})
    if var:
        env_vars[var] = "1"
    os.environ.update(env_vars)
    try:
        env = lift.LiftBatch(flat, cfg, ids, seed0=0, horizon=60, bank_episodes=3)
    finally:
        for k in env_vars:
            os.environ.pop(k, None)
    env.batch.set_stream_groups(groups)
    for t in range(T):
        env.step(tape[t])
    env.batch.sync()
    out = {k: env.batch.get(k) for k in ("qpos", "qvel", "obs", "reward", "ep_index", "ep_step", "diverged")}
    return (out, env) if keep else out


def test_mpr_separating_direction_warm_start_does_not_change_the_contact_set():
    """The convex narrow phase first tries the separating direction the pair's previous run ended on (rsim_step.hip convex_convex); separation
    along any direction proves the shapes disjoint, so every contact -- and with it every state -- is what the cold run produces: bitwise, over
    130 contact-rich control steps with episode resets."""
    a, b = _contact_rich_rollout(384, 130, warm="exact"), _contact_rich_rollout(384, 130, warm="none")
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    assert a["ep_index"].min() == 2 and a["diverged"].sum() == 0


def test_broadphase_pair_list_gives_the_candidates_of_the_full_broadphase():
    """collision() tests only the pairs whose bounding spheres were within RSIM_BP_REACH of touching when the list was built, for as long as no
    geom centre has moved half that far (rsim_step.hip, "Active pair list").  Every pair left out still fails the sphere test, so the candidates,
    contacts and states are those of testing every pair every substep (RSIM_BP_REACH=0): bitwise, over 130 contact-rich control steps with
    episode resets inside the launches, and for a reach so small that the list is rebuilt all the time."""
    full = _contact_rich_rollout(384, 130, warm="exact", env_vars={"RSIM_BP_REACH": "0"})
    for reach in (None, "0.005", "0.3"):
        a = _contact_rich_rollout(384, 130, warm="exact", env_vars={} if reach is None else {"RSIM_BP_REACH": reach})
        for k in a:
            assert np.array_equal(a[k], full[k]), (reach, k)


def test_mpr_portal_warm_start_reaches_the_same_contacts():
    """Pairs in contact restart MPR from the directions of their previous portal.  That is another path to the same facet of the Minkowski
    difference: same pairs, same depth and normal, the contact point within the rounding-level slide along the contact face that any two portals
    on one facet differ by.  Checked on the states a contact-rich rollout reaches: forward() with the records as the rollout left them against
    forward() after the positions were written back (which clears the records: a cold run)."""
    out, env = _contact_rich_rollout(1024, 58, warm="all", keep=True)
    b = env.batch
    st = {k: b.get(k) for k in ("qpos", "qvel", "qacc_warmstart", "ctrl")}
    b.forward()
    warm = dict(ncon=b.get("ncon"), con=b.get("contact"), qacc=b.get("qacc"))
    for k, v in st.items():
        b.set(k, v)                                  # rsim_set_array(RSIM_QPOS) clears the warm-start records
    b.forward()
    cold = dict(ncon=b.get("ncon"), con=b.get("contact"), qacc=b.get("qacc"))
    assert np.array_equal(warm["ncon"], cold["ncon"]) and int((warm["ncon"] > 4).sum()) >= 10      # envs with finger / hand contacts beside the cube's four
    worst = dict(dist=0.0, ang=0.0, pos=0.0, qacc=0.0)
    for e in np.nonzero(warm["ncon"] > 0)[0]:
        n = int(warm["ncon"][e])
        w, c = warm["con"][e][:n].astype(np.float64), cold["con"][e][:n].astype(np.float64)
        assert np.array_equal(w[:, 13:16], c[:, 13:16]), e                                           # geom pairs and dimensions, in order
        worst["dist"] = max(worst["dist"], float(np.abs(w[:, 0] - c[:, 0]).max()))
        worst["ang"] = max(worst["ang"], float(np.degrees(np.arccos(np.clip((w[:, 4:7] * c[:, 4:7]).sum(1), -1, 1))).max()))
        worst["pos"] = max(worst["pos"], float(np.abs(w[:, 1:4] - c[:, 1:4]).max()))
        worst["qacc"] = max(worst["qacc"], float(np.abs(warm["qacc"][e] - cold["qacc"][e]).max() / max(1.0, np.abs(cold["qacc"][e]).max())))
    print("portal warm start vs cold run on the same states:", worst)
    assert worst["dist"] < 5e-6 and worst["ang"] < 0.1 and worst["pos"] < 2e-3 and worst["qacc"] < 5e-3, worst


def test_alternating_half_batches_equal_the_whole_batch():
    """vec_env.AlternatingVecEnv: two half-batches on their own rsim batches / streams, stepped alternately with the host waiting for a half's step t
    before it issues that half's step t + 1.  Env i is env i of one big batch (seeding by global env id): observations, rewards, done flags and
    terminal records equal the lockstep VecEnv's bitwise, through on-device episode restarts."""
    from robosuite_amd.vec_env import AlternatingVecEnv, VecEnv
    flat, cfg = _lift_assets()
    B, T, H = 96, 23, 9
    whole = VecEnv("Lift", B, flat, cfg, seed=5, horizon=H, bank_episodes=3)
    alt = AlternatingVecEnv("Lift", B, flat, cfg, seed=5, horizon=H, bank_episodes=3)
    from robosuite_amd import lift
    tape = torch.tensor(lift.env_actions(np.arange(B), T), device="cuda")
    o_w = whole.reset()
    o_a = alt.reset()
    h = B // 2
    assert torch.equal(o_w[:h], o_a[0]) and torch.equal(o_w[h:], o_a[1])
    ref = []
    for t in range(T):
        o, r, d, info = whole.step(tape[t])
        whole.env.batch.sync()
        ref.append((o.clone(), r.clone(), d.clone(), info["terminal_obs"].clone()))
    for k, sl in ((0, slice(0, h)), (1, slice(h, B))):
        alt.step_half(k, tape[0][sl])
    for t in range(T):
        for k, sl in ((0, slice(0, h)), (1, slice(h, B))):
            o, r, d, info = alt.wait_half(k)
            ro, rr, rd, rt = ref[t]
            assert torch.equal(o, ro[sl]) and torch.equal(r, rr[sl]) and torch.equal(d, rd[sl]), (t, k)
            if bool(d.any()):
                assert torch.equal(info["terminal_obs"][d.bool()], rt[sl][d.bool()]), (t, k)
            if t + 1 < T:
                alt.step_half(k, tape[t + 1][sl])
    assert sum(int(r[2].sum()) for r in ref) >= 2 * B      # every env restarted at least twice


def _jammed_lift_state():
    """Cube jammed between the closed finger pads, the hand and the table: 26 contacts / 94 constraint rows on the oracle (16 / 64 fit the Lift configuration)."""
    return np.array([-3.310503761e-03, 9.595607741e-01, -4.905636198e-03, -2.424200342e+00, 9.327601525e-03, 3.760863028e+00, 8.123742675e-01, 5.613262166e-05,
                     -5.613262166e-05, -1.113625582e-01, 4.773980294e-03, 8.007105292e-01, 9.982068450e-01, -2.683816807e-02, 1.416109385e-02, 5.159719647e-02])


def test_capacity_tiers_step_an_env_beyond_the_native_capacity_without_dropping_a_contact(monkeypatch):
    """MuJoCo never drops a contact (nconmax = 5000, models/assets/base.xml:5).  rsim_control_step hands an env whose substep needs more than the native
    16 contacts / 64 rows to the wide body (32 / 128) compiled into the same control-step kernel: in the substep in which it happens the env carries on in
    the wide body of its own workgroup from the state the earlier substeps left (fused hand-over); from the next step on the wide body steps it from the
    start until its demand has dropped.  Checked on the round-3 overflow state: RSIM_OVERFLOW stays 0, RSIM_CAP_NEED shows the demand, the states after three control steps
    agree with the fp64 oracle (which holds 64 contacts) as closely as an ordinary contact state does -- and differ from what the truncating build
    (RSIM_NO_TIERS) computes; an env that never leaves the native capacity is bitwise what it is without tiers."""
    from tests.util import load_golden, make_hip, make_oracle
    g, cfg, flat = load_golden("seed1_full")
    q, q0 = _jammed_lift_state(), flat.qpos0.ravel()
    om, od, oc = make_oracle(flat, cfg)
    od.qpos[:] = q; od.qvel[:] = 0; od.qacc_warmstart[:] = 0; od.ctrl[:] = 0; od.forward(); oc.reset(od)
    assert od.ncon > 16 and od.nefc > 64
    a = np.array([0.05, -0.02, -0.3, 0.0, 0.0, 0.0, 1.0])     # press down, fingers closing

    def run(no_tiers):
        if no_tiers:
            monkeypatch.setenv("RSIM_NO_TIERS", "1")
        else:
            monkeypatch.delenv("RSIM_NO_TIERS", raising=False)
        hm, hb = make_hip(flat, cfg, B=3)
        hb.set("qpos", np.stack([q, q0, q])); hb.set("qvel", 0); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
        hb.forward(); hb.ctrl_reset()
        hb.set("overflow", 0)          # forward() is a debug entry: native capacity, drops counted (test above); from here on only control steps
        out = []
        act = torch.tensor(np.repeat(a[None], 3, 0), dtype=torch.float32, device="cuda")
        for t in range(3):
            hb.control_step(act, 25)
            out.append((hb.get("qpos").copy(), hb.get("qvel").copy()))
        return hb, out

    hb, tiered = run(False)
    need, ov = hb.get("cap_need"), hb.get("overflow")
    assert need[0, 0] > 16 and need[0, 1] > 64 and need[1, 0] <= 16 and need[1, 1] <= 64, need
    assert ov.tolist() == [0, 0, 0] and int(hb.get("diverged").sum()) == 0
    assert np.array_equal(tiered[-1][0][0], tiered[-1][0][2])                       # the same state twice: the same result, whatever the list order
    hb2, trunc = run(True)
    assert hb2.get("overflow")[0] > 0 and hb2.get("overflow")[1] == 0
    assert np.array_equal(trunc[-1][0][1], tiered[-1][0][1]) and np.array_equal(trunc[-1][1][1], tiered[-1][1][1])   # the env inside the native capacity
    errs = []
    for t in range(3):
        oc.env_step(od, a, 25)
        errs.append((np.abs(tiered[t][0][0] - od.qpos).max(), np.abs(tiered[t][1][0] - od.qvel).max(), np.abs(trunc[t][0][0] - od.qpos).max()))
    print("jammed Lift state, 3 control steps vs the fp64 oracle: tiered |dq| |dv|, truncating build |dq|:", [tuple(f"{x:.1e}" for x in e) for e in errs])
    # measured: 3e-5 / 1e-4 after the first control step (the redo path), 1e-4 / 1e-2 after the second (the env on the wide pass's list); the jam then
    # lets go (the cube squirts out from under the fingers) and the two trajectories separate like any chaotic contact event
    assert errs[0][0] < 2e-4 and errs[0][1] < 2e-3 and errs[1][0] < 1e-3, errs
    assert errs[0][2] > 50 * errs[0][0], errs          # dropping 10 of 26 contacts is a different problem: 1e-2 after one control step


def _stack_assets():
    import json, os
    from robosuite_amd import mjcf
    adir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "assets")
    return mjcf.load_model(os.path.join(adir, "stack_panda.rsim")), json.load(open(os.path.join(adir, "stack_panda.cfg.json")))


@pytest.mark.parametrize("task", ("lift", "stack"))
def test_fused_tier_hand_over_in_mid_step_carries_the_step_on(monkeypatch, task):
    """Round 6: the tier above the Lift and Stack configurations is a second body inside their control-step kernel; an env that outgrows the native capacity at
    substep k carries on in the wide body from that substep, on the LDS-resident state (qpos, qvel, warm start, actuator ctrl, controller state, time, episode flags).
    RSIM_FORCE_HANDOVER=k makes every env hand over at substep k whatever its demand: the control step must then end where the native body alone takes it
    (the two bodies differ in row slots and the memory J lives in, not in the algorithm), at every k, including with a fresh controller (needs_reset) and
    across an episode end; the demand counters, observation record and reward come out the same.  tier_stats() proves that the hand-overs took place:
    every env-step of a forced run is committed by the wide body, and every one that started on the native tier got there by a hand-over."""
    from robosuite_amd import lift, stack
    flat, cfg = (_lift_assets if task == "lift" else _stack_assets)()
    # T0: a control step by which the envs are contact-rich (hand at the table, cubes pushed around / pressed together).  Stack (configuration 1) is the only
    # fused build with J, M and the contact block all in the per-env global buffer DBatch.jg, at other offsets in the two bodies (M at Jg + 64 * 33 native,
    # Jg + 128 * 33 wide): 64 envs make the neighbouring envs' jg regions live at once, so a stride or offset slip between the bodies shows up as cross-env
    # corruption rather than noise.  Its episodes run the Stack workload's own action streams (as test_stack_4096_reached_states does).
    cls, n, T0 = {"lift": (lift.LiftBatch, 24, 60), "stack": (stack.StackBatch, 64, 80)}[task]
    ids = np.arange(n)
    tape = torch.tensor(lift.env_actions(ids, T0 + 4), device="cuda")

    def run(force):
        monkeypatch.delenv("RSIM_FORCE_HANDOVER", raising=False)
        env = cls(flat, cfg, ids, seed0=0, horizon=T0 + 2, bank_episodes=3)   # the episode ends inside the compared steps: on-device reset + fresh controllers
        b = env.batch
        for t in range(T0):
            env.step(tape[t])
        b.sync()
        out, on_tier = [], 0
        t0 = b.tier_stats()
        for t in range(T0, T0 + 4):
            on_tier += int(b.tier_snapshot().sum())      # envs the wide body steps from the start (demand of the step before): no hand-over for them
            if force is not None:
                monkeypatch.setenv("RSIM_FORCE_HANDOVER", str(force[t - T0]))
            b.set("cap_need", 0)
            env.step(tape[t])
            b.sync()
            out.append({k: b.get(k).copy() for k in ("qpos", "qvel", "qacc_warmstart", "ctrl", "time", "cstate", "obs", "reward", "ep_step", "ep_index", "done", "cap_need", "overflow", "diverged")})
        monkeypatch.delenv("RSIM_FORCE_HANDOVER", raising=False)
        t1 = b.tier_stats()
        env.bank_quiesce(); env._bank_stop()
        return out, (t1[0] - t0[0], t1[1] - t0[1]), on_tier

    ref, ref_stats, _ = run(None)
    need = np.stack([r["cap_need"] for r in ref])
    print(f"{task}, {n} envs, control steps {T0}..{T0 + 3} without forcing: envs with contacts {(need[..., 0] > 0).sum(1).tolist()}, largest demand "
          f"(contacts, rows) {need.max(1).tolist()}, wide-tier env-steps / hand-overs {ref_stats}")
    assert ref[1]["done"].all() and not ref[0]["done"].any()          # step T0 + 1 ends every episode
    for force in ([7, 7, 7, 7], [1, 24, 12, 3], [0, 0, 0, 0]):
        got, stats, on_tier = run(force)
        print(f"forced {force}: wide-tier env-steps {stats[0]}, hand-overs {stats[1]} ({on_tier} env-steps on the wide tier from the start)")
        assert stats[0] == 4 * n and stats[1] == 4 * n - on_tier, (force, stats, on_tier)     # every env-step went through the wide body ...
        assert on_tier <= n // 4, (force, on_tier)                                            # ... and most of them through the hand-over
        for t in range(4):
            for k in ("ep_step", "ep_index", "done", "overflow", "diverged"):
                assert np.array_equal(got[t][k], ref[t][k]), (force, t, k)
            assert np.array_equal(got[t]["time"], ref[t]["time"]), (force, t)
            dq, dv = np.abs(got[t]["qpos"] - ref[t]["qpos"]).max(), np.abs(got[t]["qvel"] - ref[t]["qvel"]).max()
            dc, do = np.abs(got[t]["cstate"] - ref[t]["cstate"]).max(), np.abs(got[t]["obs"] - ref[t]["obs"]).max()
            print(f"forced hand-over at substep {force[t]}, control step {t}: |dq| {dq:.1e} |dv| {dv:.1e} |dcstate| {dc:.1e} |dobs| {do:.1e}")
            # the two bodies solve the same problem with rows in other lanes: fp32 noise, growing a little over chaotic contact steps
            assert dq < 2e-4 * (t + 1) and dv < 5e-3 * (t + 1) and dc < 1e-3 * (t + 1), (force, t, dq, dv, dc)
            assert np.abs(got[t]["reward"] - ref[t]["reward"]).max() < 1e-3
        assert np.array_equal(got[0]["cap_need"], ref[0]["cap_need"])       # same contacts found in the first compared step (identical state going in)


def test_fused_tier_hand_over_with_two_osc_arm_parts(monkeypatch):
    """The 64 x 16 build (Baxter class) carries its tier as a second body too.  Its hand-over has more to carry: 64 floats of controller state (two OSC arm parts).
    The reference-recorded Baxter / OSC_POSE fixture, every control step handed over at substep 9, tracks the oracle loop and the fixture at the tolerances of the
    plain run (tests/test_hip_parity.py::test_baxter_two_osc_arm_parts_track_the_reference_loop)."""
    from oracle.oracle import env_step_parts
    from tests.util import load_golden, make_hip, make_oracle_parts
    g, cfg, flat = load_golden("ctl_osc_pose", "peg_baxter")
    nq = flat.nq
    om, od, parts = make_oracle_parts(flat, cfg)
    hm, hb = make_hip(flat, cfg, B=3)
    s0 = g["states"][0]
    od.qpos[:] = s0[1:1 + nq]; od.qvel[:] = s0[1 + nq:]; od.qacc_warmstart[:] = 0; od.forward()
    for c, _ in parts:
        c.reset(od)
    hb.set("qpos", s0[1:1 + nq][None].repeat(3, 0)); hb.set("qvel", s0[1 + nq:][None].repeat(3, 0)); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
    hb.forward(); hb.ctrl_reset()
    monkeypatch.setenv("RSIM_FORCE_HANDOVER", "9")
    t0 = hb.tier_stats()
    for t in range(len(g["actions"])):
        hb.control_step(torch.tensor(np.repeat(g["actions"][t][None], 3, 0), dtype=torch.float32, device="cuda"), 25)
        env_step_parts(od, parts, g["actions"][t], 25)
        hq, hv = hb.get("qpos")[0], hb.get("qvel")[0]
        assert np.abs(hq - od.qpos).max() < 5e-4 and np.abs(hv - od.qvel).max() < 5e-3, t
        assert np.abs(hq - g["states"][t + 1][1:1 + nq]).max() < 5e-4 and np.abs(hv - g["states"][t + 1][1 + nq:]).max() < 5e-3, t
        assert np.abs(hb.get("ctrl")[0] - g["ctrl"][t]).max() < 2e-3 * max(1.0, np.abs(g["ctrl"][t]).max()), t
    t1 = hb.tier_stats()
    monkeypatch.delenv("RSIM_FORCE_HANDOVER")
    assert t1[1] - t0[1] == 3 * len(g["actions"])          # every env of every step really went through the hand-over
    assert np.array_equal(hb.get("qpos")[0], hb.get("qpos")[2]) and int(hb.get("overflow").sum()) == 0


def test_contact_onset_hint_changes_the_dispatch_order_and_nothing_else(monkeypatch):
    """Round 6: the dispatch-order key of an env is its duration, raised by half when one of its convex pairs ended the last substep within RSIM_NEAR_THRESH of touching
    (a contact about to start is what a duration cannot predict).  It must be ORDERING ONLY: the same rollout with the hint off, at its default and with a net so wide
    that every env is flagged ends in bitwise the same states, rewards and demand counters."""
    from robosuite_amd import lift
    flat, cfg = _lift_assets()
    ids = np.arange(96)
    T = 45
    tape = torch.tensor(lift.env_actions(ids, T), device="cuda")
    out = []
    for thr in ("0", None, "10"):
        if thr is None:
            monkeypatch.delenv("RSIM_NEAR_THRESH", raising=False)
        else:
            monkeypatch.setenv("RSIM_NEAR_THRESH", thr)
        env = lift.LiftBatch(flat, cfg, ids, seed0=0, horizon=0)       # the threshold is read when the batch is created
        for t in range(T):
            env.step(tape[t])
        b = env.batch
        b.sync()
        out.append({k: b.get(k).copy() for k in ("qpos", "qvel", "qacc_warmstart", "ctrl", "cstate", "obs", "reward", "cap_need")})
    monkeypatch.delenv("RSIM_NEAR_THRESH", raising=False)
    assert np.abs(out[0]["qvel"]).max() > 0.05 and int((out[0]["cap_need"][:, 0] > 4).sum()) > 10      # a rollout with contacts, not a trivial one
    for o in out[1:]:
        for k in out[0]:
            assert np.array_equal(o[k], out[0][k]), k


def test_capacity_tiers_with_per_env_model_parameters_and_stream_groups():
    """The wide configuration reads an env's OWN constant block (per-episode cube sizes: built on demand right before the wide pass steps the env);
    with stream groups every env block runs its own native pass, wide pass and redo pass on its own stream.  Same envs, same results."""
    import json, os
    from robosuite_amd import lift, mjcf
    adir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "assets")
    flat = mjcf.load_model(os.path.join(adir, "lift_panda.rsim")); cfg = json.load(open(os.path.join(adir, "lift_panda.cfg.json")))
    ids = np.array([7, 3, 7, 11, 3, 5])
    q = _jammed_lift_state()
    res = []
    for G in (1, 3):
        env = lift.LiftBatch(flat, cfg, ids, seed0=0, horizon=0)          # per-env cube sizes (env 0 and 2, 1 and 4 share theirs)
        if G > 1:
            env.batch.set_stream_groups(G)
        b = env.batch
        qq = b.get("qpos"); qq[[0, 2, 4]] = q
        b.set("qpos", qq); b.set("qvel", 0); b.set("qacc_warmstart", 0); b.set("ctrl", 0); b.forward(); b.ctrl_reset()
        b.set("overflow", 0)           # the debug entry forward() keeps the native capacity and counts its drops
        act = torch.zeros(len(ids), 7, device="cuda"); act[:, 2] = -0.3; act[:, 6] = 1.0
        for t in range(4):
            env.step(act)
        need = b.get("cap_need")
        assert (need[[0, 2, 4], 1] > 64).all() and (need[[1, 3, 5], 1] <= 64).all() and int(b.get("overflow").sum()) == 0, need
        res.append((b.get("qpos").copy(), b.get("qvel").copy()))
        assert np.isfinite(res[-1][0]).all() and np.array_equal(res[-1][0][0], res[-1][0][2])
        assert not np.array_equal(res[-1][0][0], res[-1][0][4])            # another cube size: another block was built and read
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])


def test_reset_observation_of_an_env_that_ends_its_episode_on_the_wide_tier():
    """Round-4 advisor finding: the reset-observation pass that follows a control step ran as a native tier pass and skipped every env whose tier was 1,
    so an env that hit its horizon while the wide configuration stepped it kept the TERMINAL record in RSIM_OBS.  Horizon 2: step 1 takes the jammed envs
    through the redo list, step 2 steps them from the wide pass's list and ends every episode; RSIM_OBS must then be what rsim_observe computes on the
    reset state (MujocoEnv.reset(): forward + observables, base.py:298-347), for the tier-1 envs as for the others, on one stream and with stream groups."""
    from robosuite_amd import lift
    flat, cfg = _lift_assets()
    ids = np.array([7, 3, 7, 11, 3, 5])
    q = _jammed_lift_state()
    for G in (1, 3):
        env = lift.LiftBatch(flat, cfg, ids, seed0=0, horizon=2, bank_episodes=3)
        if G > 1:
            env.batch.set_stream_groups(G)
        b = env.batch
        qq = b.get("qpos"); qq[[0, 2, 4]] = q
        b.set("qpos", qq); b.set("qvel", 0); b.set("qacc_warmstart", 0); b.set("ctrl", 0); b.forward(); b.ctrl_reset()
        b.set("overflow", 0)
        act = torch.zeros(len(ids), 7, device="cuda"); act[:, 2] = -0.3; act[:, 6] = 1.0
        env.step(act)
        assert b.get("done").tolist() == [0] * len(ids)
        env.step(act)
        b.sync()
        need = b.get("cap_need")
        assert (need[[0, 2, 4], 1] > 64).all() and (need[[1, 3, 5], 1] <= 64).all() and int(b.get("overflow").sum()) == 0, need
        assert b.get("done").tolist() == [1] * len(ids) and b.get("ep_index").tolist() == [1] * len(ids)
        assert np.array_equal(b.get("qpos"), lift.episode_setup(0, ids, 1)[1].astype(np.float32))
        obs, term = b.get("obs").copy(), b.get("terminal_obs").copy()
        b.observe()
        ref = b.get("obs").copy()
        assert np.abs(obs - ref).max() < 1e-6, (G, np.abs(obs - ref).max(axis=1))
        assert (np.abs(obs - term).max(axis=1) > 1e-3).all()          # the terminal record went to RSIM_TERMINAL_OBS, not into RSIM_OBS
        assert int(b.get("overflow").sum()) == 0


def test_reading_derived_arrays_between_fused_steps_changes_nothing():
    """Round-4 advisor finding: a read of a derived array after a fused control step refreshes it with a debug forward; that forward used to rewrite the
    narrow phase's warm-start records and the warm start of the solver and to count into RSIM_OVERFLOW / RSIM_CAP_NEED, so a rollout depended on whether
    the host had looked.  Two rollouts of the same contact-rich envs, one of them reading positions, contacts, forces, M and a Jacobian after every step:
    bitwise the same states, the same demand and drop counters."""
    from robosuite_amd import lift
    flat, cfg = _lift_assets()
    ids = np.arange(6)
    T = 40
    tape = torch.tensor(lift.env_actions(ids, T), device="cuda")
    out = []
    for look in (False, True):
        env = lift.LiftBatch(flat, cfg, ids, seed0=0, horizon=0)
        b = env.batch
        for t in range(T):
            env.step(tape[t])
            if look:
                b.get("xpos"); b.get("efc_force"); b.get("qacc"); b.full_M(1); b.contacts_abi(2); b.contacts(3)
                b.jac_site(4, 0)
        b.sync()
        out.append({k: b.get(k).copy() for k in ("qpos", "qvel", "qacc_warmstart", "ctrl", "time", "overflow", "cap_need")})
    assert out[1]["cap_need"][:, 0].max() >= 3          # hands on the table: there is a narrow phase to disturb
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


def test_full_M_and_contacts_exports_of_the_c_abi():
    """rsim_full_M (mj_fullM, controllers/parts/controller.py:226-227) and rsim_contacts (sim.data.contact[:ncon]) against the array fields they are views of,
    and against the oracle; after a FUSED control step both describe the current state (the derived arrays are refreshed on read)."""
    from tests.util import load_golden, make_hip, make_oracle
    g, cfg, flat = load_golden("seed1_full")
    nq = flat.nq
    hm, hb = make_hip(flat, cfg, B=2)
    s = g["states"][30]
    hb.set("qpos", s[1:1 + nq][None].repeat(2, 0)); hb.set("qvel", s[1 + nq:][None].repeat(2, 0)); hb.set("qacc_warmstart", 0); hb.set("ctrl", 0)
    hb.forward(); hb.ctrl_reset()
    om, od, _ = make_oracle(flat, cfg)
    od.qpos[:] = s[1:1 + nq]; od.qvel[:] = s[1 + nq:]; od.forward()
    M = hb.full_M(1)
    assert M.shape == (flat.nv, flat.nv) and np.array_equal(M.astype(np.float32), hb.get("qM")[1]) and np.abs(M - od.full_M()).max() < 1e-5 * np.abs(M).max()
    ca, cb = hb.contacts_abi(0), hb.contacts(0)
    assert len(ca) == len(cb) == od.ncon > 0
    for a, b, o in zip(ca, cb, od.contacts()):
        assert (a["geom1"], a["geom2"], a["dim"], a["efc_address"]) == (b["geom1"], b["geom2"], b["dim"], b["efc_address"]) == (o["geom1"], o["geom2"], o["dim"], o["efc_address"])
        assert a["dist"] == b["dist"] and np.array_equal(a["frame"], b["frame"]) and abs(a["dist"] - o["dist"]) < 1e-6
    hb.control_step(torch.zeros(2, 7, device="cuda"), 25)
    q1 = hb.get("qpos")[0].astype(np.float64)
    od.qpos[:] = q1; od.qvel[:] = hb.get("qvel")[0]; od.forward()
    assert np.abs(hb.full_M(0) - od.full_M()).max() < 1e-5 * np.abs(od.full_M()).max()      # of the state AFTER the control step
    with pytest.raises(Exception):
        hb.full_M(5)
