"""Vectorised counterpart of `suite.make(env_name, robots=...)` + `GymWrapper` for the tasks the fused kernel carries.

    env = VecEnv("Stack", n_envs=4096, flat=..., cfg=...)       # Lift | Stack | TwoArmPegInHole | PickPlace
    obs = env.reset()                                           # device tensor [n_envs, obs_dim], the reference's per-key record concatenated
    obs, reward, done, info = env.step(actions)                 # actions: CUDA float32 [n_envs, action_dim] in [-1, 1]
    flat = env.flat_obs(obs)                                    # GymWrapper layout (wrappers/gym_wrapper.py:45-163): object-state + robot proprio keys
    cube = env.key(obs, "cubeA_pos")                            # one observable by the reference's key name

Semantics follow the reference loop (environments/base.py:277-347, 467-521): `done` is reported on the control step that reaches `horizon`,
the env restarts on the device from its next pre-drawn reset (hard reset draws in the reference's RNG order) and the next `step` continues
the new episode.  Everything returned aliases device memory owned by the backend.

Off by default, episodes can also end before the horizon, with the same on-device restart and `done`:
    env = VecEnv(..., terminate_on_success=True, min_episode_steps=5)    # the task's success check ends the episode (from its 5th step on)
    env = VecEnv(..., terminate_on_diverged=True)                        # an env the bad-state guard had to reset starts a new episode from a drawn reset
    obs = env.end_episodes(mask)                                         # the caller's own condition (CUDA bool tensor [n_envs]), between two steps
info["end_reason"] (int32: 0 running, 1 horizon, 2 success, 3 diverged, 4 requested) then says why an env reported `done`.
"""
from __future__ import annotations

import numpy as np

from . import lift, peg_in_hole, pick_place, stack

TASKS = {"Lift": lift.LiftBatch, "Stack": stack.StackBatch, "TwoArmPegInHole": peg_in_hole.PegBatch, "PickPlace": pick_place.PickPlaceBatch}
# single-object mode 2 of PickPlace (pick_place.py:810-847): the model / task constants of the env's own fixture carry single_object_mode and object_id
_SINGLE_OBJECT = {"PickPlaceMilk": 0, "PickPlaceBread": 1, "PickPlaceCereal": 2, "PickPlaceCan": 3}   # object_to_id, pick_place.py:218
TASKS.update({n: pick_place.PickPlaceBatch for n in _SINGLE_OBJECT})
TASKS["PickPlaceSingle"] = pick_place.PickPlaceBatch     # single_object_mode = 1: the object is drawn at every reset (pick_place.py:800-807)


class VecEnv:
    def __init__(self, env_name: str, n_envs: int, flat, cfg, device: int = 0, seed: int = 0, horizon: int = 500, env_ids=None, bank_episodes: int = 4, stream_groups: int = 1,
                 terminate_on_success: bool = False, terminate_on_diverged: bool = False, min_episode_steps: int = 1):
        if env_name not in TASKS:
            raise ValueError(f"{env_name!r} has no on-device task epilogue (have {sorted(TASKS)})")
        ids = np.arange(n_envs) if env_ids is None else np.asarray(env_ids)
        if env_name in _SINGLE_OBJECT:
            # PickPlaceMilk / Bread / Cereal / Can are PickPlace with single_object_mode = 2 and the named object (pick_place.py:810-847): a cfg that
            # does not say so would silently run the four-object task under a single-object name
            t = cfg.get("task", {})
            if int(t.get("single_object_mode", 0)) != 2 or int(t.get("object_id", -1)) != _SINGLE_OBJECT[env_name]:
                raise ValueError(f"{env_name}: cfg['task'] must carry single_object_mode = 2 and object_id = {_SINGLE_OBJECT[env_name]} "
                                 f"(got {t.get('single_object_mode')}, {t.get('object_id')}); build the cfg from a {env_name} env")
        if env_name == "PickPlaceSingle" and int(cfg.get("task", {}).get("single_object_mode", 0)) != 1:
            raise ValueError("PickPlaceSingle: cfg['task'] must carry single_object_mode = 1; build the cfg from a PickPlaceSingle env")
        self.env_name = env_name
        self.env = TASKS[env_name](flat, cfg, ids, device=device, seed0=seed, horizon=horizon, bank_episodes=bank_episodes)
        self.n_envs, self.horizon, self.bank_episodes = len(ids), horizon, bank_episodes
        if stream_groups > 1:   # env blocks stepped on their own HIP streams (rsim_set_stream_groups): same results, no whole-batch tail per step
            self.env.batch.set_stream_groups(min(int(stream_groups), self.n_envs))
        self.action_dim, self.obs_dim = self.env.model.action_dim, self.env.model.nobs
        # early episode end (include/rsim.h rsim_set_early_end): nothing is armed, launched or reported unless asked for
        self._early = (bool(terminate_on_success), bool(terminate_on_diverged), int(min_episode_steps))
        self.early_end_armed, self._ended_on_request = self._early[0] or self._early[1], False
        if self.early_end_armed:
            if not bank_episodes:
                raise ValueError("terminate_on_success / terminate_on_diverged need the reset ring (bank_episodes >= 2): an episode that ends restarts from a pre-drawn reset")
            self.env.set_early_end(*self._early)
        keys, dims = cfg["obs_keys"], cfg["obs_dims"]
        off = np.cumsum([0] + list(dims))
        self.obs_slices = {k: slice(int(off[i]), int(off[i + 1])) for i, k in enumerate(keys)}
        self._object_keys = [k for k in keys if not k.startswith("robot0_")]
        self._proprio_keys = [k for k in keys if k.startswith("robot0_")]

    @property
    def action_spec(self):
        return -np.ones(self.action_dim), np.ones(self.action_dim)

    def reset(self, seed=None):
        """Every env back to episode 0 of its stream (with `seed`: of the streams keyed by that seed, env i = default_rng(seed + i)).  The reset ring is re-installed for episodes 0 .. E-1: it has moved on by then, and resets
        read from slots that still held later episodes would silently break `episode k of env i = episode_setup(seed, i, k)`."""
        e = self.env
        e._bank_stop()      # the upkeep thread draws from the same per-env generators (EpisodeStreams): it must be gone before they are re-keyed / replayed
        if seed is not None and int(seed) != e.seed0:
            e.seed0, e._streams = int(seed), None
        e.batch.set("qfrc_applied", 0.0); e.batch.set("xfrc_applied", 0.0)   # mj_resetData: episodes start without external forces (before the reset's forward)
        e.reset(block=0)
        b = e.batch
        b.set("ep_step", 0); b.set("ep_index", 0); b.set("done", 0)
        if self.bank_episodes:
            e.install_reset_bank(self.bank_episodes)
        if self.early_end_armed or self._ended_on_request:
            b.set("end_reason", 0)
        if self.early_end_armed:
            e.set_early_end(*self._early)      # re-armed: guard hits of the episodes before the reset end nothing
        b.observe()
        return e.obs()

    def step(self, actions):
        self.env.step(actions)
        return self.env.obs(), self.env.reward(), self.env.batch.tensor("done"), self._info()

    def _info(self):
        # gym auto-reset convention: for an env whose episode just ended, `obs` is already the reset observation of its next episode and the
        # last record of the finished one is in info["terminal_obs"] (rows of envs that did not finish are stale)
        info = {"success": self.env.success(), "terminal_obs": self.env.batch.tensor("terminal_obs")}
        if self.early_end_armed:
            info["end_reason"] = self.env.batch.tensor("end_reason")
        elif self._ended_on_request:           # no rule armed: the control step maintains `done` alone, and `done` then means the horizon
            info["end_reason"] = self.env.batch.tensor("done").clone()
        return info

    def end_episodes(self, mask):
        """End now the running episode of every env flagged in `mask` (CUDA bool / uint8 tensor [n_envs]) -- the caller's own termination condition,
        evaluated between two steps.  Those envs restart on the device from their next pre-drawn reset, exactly as at the horizon; the returned
        observation tensor holds their reset observation (their last record moves to info["terminal_obs"] of the next step's info, `done` reads 1 and
        `end_reason` 4 until their next step); every other env is untouched.  Needs the reset ring (bank_episodes >= 2)."""
        if not self.bank_episodes:
            raise ValueError("end_episodes needs the reset ring (bank_episodes >= 2)")
        self.env.end_episodes(mask)
        self._ended_on_request = True
        return self.env.obs()

    def sensor(self, name: str):
        """sim.data.sensordata of the named sensor for every env, [n_envs, dim]: a device tensor aliasing the batch.  The fused `step` does not compute
        sensors; the first read after it runs one forward pass on the current state (and waits for it), as robosuite's sim.forward() before such a read."""
        s = self.env.batch.sensor(name)
        self.env.batch.sync()
        return s

    # ---- geometric queries (include/rsim.h rsim_ray / rsim_render_depth): explicit calls, never part of `step`
    def cameras(self, xml: str | None = None):
        """{name: raycast.Camera} of the fixed cameras of the env's MJCF: of `xml`, or of the XML the model was compiled from when it is at hand (the shipped
        assets carry none: hand `render_depth` a raycast.Camera then)."""
        from . import raycast

        flat = self.env.model.flat
        xml = xml if xml is not None else getattr(flat, "xml", None)
        if xml is None:
            raise ValueError("cameras: this model carries no MJCF; pass the XML, or build a raycast.Camera(body, pos, quat, fovy) yourself")
        return raycast.cameras_from_xml(xml, flat)

    def raycast(self, origins, dirs, geomgroup=0, static=True, bodyexclude=-1):
        """mj_ray for every env: origins / dirs [n_envs, N, 3] device tensors -> (dist [n_envs, N], -1 = nothing hit; geomid [n_envs, N]).  The first query after
        a fused `step` runs one forward pass on the current state, as robosuite's sim.forward() before such a read."""
        return self.env.batch.raycast(origins, dirs, geomgroup=geomgroup, static=static, bodyexclude=bodyexclude)

    def render_depth(self, camera, height, width, segmentation=False, convention="opengl", **opts):
        """Metric depth image of every env, [n_envs, H, W] (what robosuite's get_real_depth_map makes of a depth observation; +inf where nothing is hit), and
        with segmentation=True the `element` segmentation (geom ids, -1 = nothing; robosuite's camera_segmentations="element").  camera: a raycast.Camera,
        or the name of a fixed camera when the model's MJCF is at hand.  convention: "opengl" hands the BOTTOM row first, as robosuite's default image
        convention does; "opencv" the top row first.  Colour, `instance` / `class` segmentation, tracking cameras and heightfields are not carried."""
        if convention not in ("opengl", "opencv"):
            raise ValueError(f"convention must be 'opengl' or 'opencv', got {convention!r}")
        if isinstance(camera, str):
            cams = self.cameras()
            if camera not in cams:
                raise KeyError(f"no fixed camera named {camera!r} (have {sorted(cams)})")
            camera = cams[camera]
        out = self.env.batch.render_depth(camera, height, width, segmentation=segmentation, **opts)
        if convention == "opencv":
            return out
        return tuple(o.flip(1) for o in out) if segmentation else out.flip(1)

    def _geom_ids(self, pairs):
        names = self.env.model.flat.names["geom"]
        out = []
        for pr in pairs:
            if len(pr) != 2:
                raise ValueError(f"geom_distance: a pair is two geoms, got {pr!r}")
            ids = []
            for g in pr:
                if isinstance(g, str):
                    if g not in names:
                        raise KeyError(f"no geom named {g!r}")
                    g = names.index(g)
                ids.append(int(g))
            out.append(ids)
        return np.asarray(out, dtype=np.int32).reshape(-1, 2)

    def geom_distance(self, pairs, distmax=1.0, fromto=True, signed=False, pen=None, **opts):
        """mj_geomDistance for every env: pairs is a list of (geom, geom), each a geom name or a model geom id -> (dist [n_envs, P], fromto [n_envs, P, 6] or
        None, status [n_envs, P]) device tensors (HipBatch.geom_distance: status codes, the convex-hull and overlap rules).  The first query after a fused
        `step` runs one forward pass on the current state, as `raycast` does.  signed=True: overlapping boxes, cylinders, ellipsoids and meshes (and a
        sphere or capsule in one of them) come back with dist = minus the penetration depth, witnesses and status 0 instead of (0, one point, status 2); pen:
        the descent's options (HipBatch.geom_distance)."""
        so = dict(opts, signed=True, pen=pen) if signed else opts
        return self.env.batch.geom_distance(self._geom_ids(pairs), distmax=distmax, fromto=fromto, **so)

    def body_distance(self, bodies_a, bodies_b, distmax=1.0, signed=False, pen=None, **opts):
        """The smallest distance between two sets of bodies (names or ids) per env: all geom pairs (a geom of A, a geom of B) are queried and reduced with
        torch.min.  -> (min dist [n_envs], its fromto [n_envs, 6], its pair index [n_envs], the pair list int32 [P, 2]).  GEOMS THE QUERY REFUSES ARE
        SKIPPED: mesh geoms whose hull vertices the model does not hold (visual-only meshes), heightfields, a geom against itself, plane against plane
        (distance.body_pairs).  With every pair beyond distmax the result is (distmax, zeros, 0).  signed=True, pen: as geom_distance -- the minimum then is
        the deepest overlap where bodies overlap, not 0."""
        import torch

        from . import distance as _dist

        flat = self.env.model.flat
        bn = flat.names["body"]

        def ids(bodies):
            bodies = [bodies] if isinstance(bodies, (str, int, np.integer)) else list(bodies)
            for b in bodies:
                if isinstance(b, str) and b not in bn:
                    raise KeyError(f"no body named {b!r}")
            return [bn.index(b) if isinstance(b, str) else int(b) for b in bodies]

        pairs = _dist.body_pairs(flat, ids(bodies_a), ids(bodies_b))
        dist, ft, _ = self.env.batch.geom_distance(pairs, distmax=distmax, fromto=True, **(dict(opts, signed=True, pen=pen) if signed else opts))
        d, k = torch.min(dist, dim=1)
        return d, ft[torch.arange(ft.shape[0], device=ft.device), k], k, pairs

    def solve_ik(self, pos, quat=None, arm=0, q_init=None, **opts):
        """Which arm joint positions put the gripper site at this pose?  pos [n_envs, K, 3] / quat [n_envs, K, 4] (wxyz; None: position only) device tensors,
        2-D for K = 1; q_init [n_envs, K, n] start vectors (None: the current joint positions) -> (q, err, iters, converged) (HipBatch.solve_ik).  Site and
        dofs are those of the env's controller description: `eef_site` and the arm's `dof_idx`; arm=1: the second arm of a two-arm OSC description.  A query:
        the simulation state is not touched -- hand `q` to a JOINT_POSITION action, or write it yourself."""
        from .backend import ctrl_desc

        d = ctrl_desc(self.env.cfg)
        if arm == 0:
            site, dofs = int(d.eef_site), [int(d.dof_idx[i]) for i in range(d.ndof) if d.part_of[i] == 0]
        elif arm == 1 and d.narm == 2:
            site, dofs = int(d.eef_site2), [int(d.dof_idx[8 + i]) for i in range(d.ndof2)]
        else:
            raise ValueError(f"solve_ik: the controller description has no arm {arm}")
        return self.env.batch.solve_ik(site, dofs, pos, quat=quat, q_init=q_init, **opts)

    def solve_ik_avoid(self, pos, quat=None, arm=0, q_init=None, pairs=None, d_safe=0.05, attach=None, held=None, rel=None, signed=False, pen=None, **opts):
        """Which arm joint positions put the gripper site at this pose AND stand clear of the scene?  solve_ik with the gradient of config_collision_cost as a
        secondary task in the null space of the pose task -> (q, err, iters, converged, finished, cost, nnear, noverlap) (HipBatch.solve_ik_avoid).  finished =
        converged and cost <= cost_tol, by default 1/2 (d_safe / 2)^2: every listed pair is then at least d_safe / 2 apart.  Site and dofs: as solve_ik; pairs,
        attach / held / rel: as config_clearance; opts: avoid_gain, cost_tol, check_every, chunks and solve_ik's.  What repairs a grazing IK solution:

            pairs = [p for p in env.batch.config_pairs(dofs) if not parent_child(p)]      # a pair that can never leave d_safe never lets a problem finish
            q, err, it, ok, free, cost, nnear, nover = env.solve_ik_avoid(pos, quat, pairs=pairs, q_init=starts)      # K > 1 starts: an overlap gives no push

        signed=True: an overlapping pair enters every evaluation with its negative distance and pushes, so a start that touches or sits in an obstacle -- the
        robot's current configuration, often -- moves out (HipBatch.solve_ik_avoid); pen: the descent's options.
        """
        from .backend import ctrl_desc

        d = ctrl_desc(self.env.cfg)
        if arm == 0:
            site, dofs = int(d.eef_site), [int(d.dof_idx[i]) for i in range(d.ndof) if d.part_of[i] == 0]
        elif arm == 1 and d.narm == 2:
            site, dofs = int(d.eef_site2), [int(d.dof_idx[8 + i]) for i in range(d.ndof2)]
        else:
            raise ValueError(f"solve_ik_avoid: the controller description has no arm {arm}")
        ids = None if pairs is None else self._geom_ids(pairs)
        return self.env.batch.solve_ik_avoid(site, dofs, pos, quat=quat, q_init=q_init, pairs=ids, d_safe=d_safe,
                                             attach=self._attach_ids("solve_ik_avoid", attach, arm), held=held, rel=rel, signed=signed, pen=pen, **opts)

    def _arm_dofs(self, who, arm):
        from .backend import ctrl_desc

        d = ctrl_desc(self.env.cfg)
        first = [int(d.dof_idx[i]) for i in range(d.ndof) if d.part_of[i] == 0]
        if arm == 0:
            return first
        if arm in (1, "both") and d.narm == 2:
            second = [int(d.dof_idx[8 + i]) for i in range(d.ndof2)]
            return second if arm == 1 else first + second
        raise ValueError(f"{who}: the controller description has no arm {arm!r}")

    def _attach_ids(self, who, attach, arm):
        """attach = [(body, carrier), ...], names or model body ids; carrier None: the body of the arm's `eef_site` -> [(body id, carrier id), ...] or None"""
        from .backend import ctrl_desc

        if attach is None:
            return None
        flat = self.env.model.flat
        names = flat.names["body"]

        def one(b):
            if isinstance(b, str):
                if b not in names:
                    raise KeyError(f"no body named {b!r}")
                return names.index(b)
            return int(b)

        out = []
        for pr in attach:
            if len(pr) != 2:
                raise ValueError(f"{who}: an attachment is (body, carrier), got {pr!r}")
            body, carrier = pr
            if carrier is None:
                d = ctrl_desc(self.env.cfg)
                if arm not in (0, 1) or (arm == 1 and d.narm != 2):
                    raise ValueError(f"{who}: carrier=None needs one arm's eef_site, got arm {arm!r}")
                site = int(d.eef_site) if arm == 0 else int(d.eef_site2)
                carrier = int(np.asarray(flat.arrays["site_bodyid"]).ravel()[site])
            out.append((one(body), one(carrier)))
        return out

    def config_fk(self, q, arm=0, attach=None, held=None, rel=None):
        """Body poses at candidate arm joint vectors, away from the state: q [n_envs, K, n] (2-D for K = 1) device tensor of the arm's joint positions ->
        (xpos [n_envs, K, nbody, 3], xquat [n_envs, K, nbody, 4]) of all bodies (HipBatch.config_fk).  The dofs are the arm's `dof_idx` of the env's
        controller description; arm=1: the second arm of a two-arm description, arm="both": the two concatenated.  attach / held / rel: carried objects, as
        config_clearance."""
        return self.env.batch.config_fk(self._arm_dofs("config_fk", arm), q, attach=self._attach_ids("config_fk", attach, arm), held=held, rel=rel)

    def config_clearance(self, q, arm=0, pairs=None, distmax=1.0, attach=None, held=None, rel=None, signed=False, pen=None, **opts):
        """Is this arm configuration free, and by how much?  q [n_envs, K, n] (2-D for K = 1) candidate joint positions of the arm -> (dist, pair, fromto,
        status) per candidate: the smallest distance over `pairs`, the index into the list of the pair that attains it, its nearest points and its status
        (HipBatch.config_clearance: the status codes, the convex-hull and overlap rules).  pairs: a list of (geom, geom), names or model geom ids; None: the
        model's collision pairs the arm's joints can change (HipBatch.config_pairs).  Every joint that is not the arm's -- fingers, objects, the other arm --
        is held where it is.  The simulation state is not touched.  arm: as config_fk.  With solve_ik:

            q, err, it, ok = env.solve_ik(pos, quat)
            d, pair, ft, st = env.config_clearance(q)
            free = ok & (d > margin)

        A GRASPED OBJECT MOVES WITH THE CANDIDATE ONLY IF THE CALL SAYS SO: attach = [(body, carrier), ...], names or model body ids, carrier None meaning the
        body of the arm's `eef_site`; held = bool tensor [n_envs] or [n_envs, n] (None: held in every env -- the caller decides what is grasped); rel =
        [n_envs, n, 7] pose of the body in the carrier's frame (None: as it sits now).  Then the object rides on the carrier in the envs that hold it, drops out
        against the fingers that hold it and comes in against the table, the bin and the other arm (HipBatch.config_clearance):

            d, pair, ft, st = env.config_clearance(q, attach=[("cube_main", None)], held=grasped)

        signed=True: a colliding candidate reports its deepest listed pair, dist < 0 with that pair's witnesses, instead of 0 with status 2: two colliding
        candidates can be ranked (HipBatch.config_clearance); pen: the descent's options.
        """
        ids = None if pairs is None else self._geom_ids(pairs)
        return self.env.batch.config_clearance(self._arm_dofs("config_clearance", arm), q, pairs=ids, distmax=distmax,
                                               attach=self._attach_ids("config_clearance", attach, arm), held=held, rel=rel, signed=signed, pen=pen, **opts)

    def config_clearance_grad(self, q, arm=0, pairs=None, distmax=1.0, attach=None, held=None, rel=None, signed=False, pen=None, **opts):
        """Which way does this arm configuration move away from the scene?  config_clearance with one more result: -> (dist, pair, fromto, status, grad), grad
        [n_envs, K, n] the derivative of dist with respect to the arm's joints for the pair that attains the minimum (HipBatch.config_clearance_grad: the
        formula, the zero rules -- far, overlap, |dist| < 1e-7 -- and the two limits).  arm, pairs, attach / held / rel: as config_clearance.  A step of
        q + step * grad raises the clearance of that pair; the gradient jumps where the nearest pair switches -- collision_cost does not.  signed=True: a
        colliding candidate has the gradient of its deepest pair's negative distance instead of zeros (HipBatch.config_clearance_grad); pen: the descent's
        options."""
        ids = None if pairs is None else self._geom_ids(pairs)
        return self.env.batch.config_clearance_grad(self._arm_dofs("config_clearance_grad", arm), q, pairs=ids, distmax=distmax,
                                                    attach=self._attach_ids("config_clearance_grad", attach, arm), held=held, rel=rel, signed=signed, pen=pen,
                                                    **opts)

    def config_collision_cost(self, q, d_safe=0.05, arm=0, pairs=None, attach=None, held=None, rel=None, signed=False, pen=None, **opts):
        """The smooth collision cost of arm configurations and its gradient: -> (cost, grad, nnear, noverlap) (HipBatch.config_collision_cost): the sum of
        1/2 (d_safe - d)^2 over the listed pairs closer than d_safe.  arm, pairs, attach / held / rel: as config_clearance.  signed=True: an overlapping pair
        enters with its negative distance and pushes (HipBatch.config_collision_cost); pen: the descent's options."""
        ids = None if pairs is None else self._geom_ids(pairs)
        opts = dict(opts, signed=True, pen=pen) if signed else opts
        return self.env.batch.config_collision_cost(self._arm_dofs("config_collision_cost", arm), q, pairs=ids, d_safe=d_safe,
                                                    attach=self._attach_ids("config_collision_cost", attach, arm), held=held, rel=rel, **opts)

    def collision_cost(self, q, d_safe=0.05, arm=0, signed=False, pen=None, **opts):
        """config_collision_cost's cost as a DIFFERENTIABLE torch value: backward is grad_out[..., None] * grad, the device's analytic gradient --

            q.requires_grad_(True)
            env.collision_cost(q, 0.05).sum().backward()      # q.grad is filled

        First order only (no second derivatives); the cost is C1, so a first-order optimiser on [n_envs, K, n] tensors sees a continuous gradient.
        signed=True, pen: as config_collision_cost -- the gradient then leads out of an overlap instead of vanishing in it."""
        opts = dict(opts, signed=True, pen=pen) if signed else opts
        return _collision_cost_fn().apply(q, self, float(d_safe), arm, opts)

    def config_sweep(self, q0, q1, arm=0, pairs=None, distmax=1.0, attach=None, held=None, rel=None, **opts):
        """Is the arm motion from q0 to q1 free?  q0, q1 [n_envs, K, n] (2-D for K = 1) ends of K joint-space segments per env, interpolated linearly ->
        (status, t, dist, t_min, pair, fromto, steps) per segment (HipBatch.config_sweep: 0 FREE, 1 HIT, 2 UNDECIDED; the motion is certified to keep more
        than `margin` of clearance on [0, t)).  arm, pairs: as config_clearance; opts: margin, slack, max_steps, fromto, tol, max_iters.  Every joint that is
        not the arm's is held where it is; a grasped object moves with the motion only if the call says so (attach / held / rel, as config_clearance: the
        motion bound then covers the carried bodies).  The simulation state is not touched.  One motion bound serves the
        whole list: a listed pair that stays within margin + slack whatever the arm does (the Panda's link0 / link1 geoms, 1.0 mm apart) decides every segment
        at its first sample -- pass `pairs` without it."""
        ids = None if pairs is None else self._geom_ids(pairs)
        return self.env.batch.config_sweep(self._arm_dofs("config_sweep", arm), q0, q1, pairs=ids, distmax=distmax,
                                           attach=self._attach_ids("config_sweep", attach, arm), held=held, rel=rel, **opts)

    def path_clearance(self, waypoints, arm=0, pairs=None, distmax=1.0, attach=None, held=None, rel=None, **opts):
        """Is this joint-space path free?  waypoints [n_envs, K, W, n]: K paths per env of W >= 2 arm joint vectors, joined by straight joint-space segments
        -> (free bool [n_envs, K], first_segment int64, t, dist float32, pair int32).  One config_sweep call over the K (W - 1) segments, reduced in torch: a
        path is free only if EVERY segment is FREE; otherwise first_segment is the first segment that is not (HIT or UNDECIDED) and t, dist, pair are that
        segment's (the path is certified up to parameter t of it).  A free path reads first_segment -1, t 1 and the smallest dist over its segments with that
        segment's pair.  arm, pairs, attach, held, rel, opts: as config_sweep."""
        import torch

        if not (isinstance(waypoints, torch.Tensor) and waypoints.dim() == 4 and waypoints.shape[2] >= 2):
            raise ValueError(f"path_clearance: waypoints must be a tensor [n_envs, K, W, n] with W >= 2, got {tuple(getattr(waypoints, 'shape', ()))}")
        B, K, W, n = waypoints.shape
        q0, q1 = waypoints[:, :, :-1].reshape(B, K * (W - 1), n), waypoints[:, :, 1:].reshape(B, K * (W - 1), n)
        st, t, dist, _, pair, _, _ = self.config_sweep(q0, q1, arm=arm, pairs=pairs, distmax=distmax, attach=attach, held=held, rel=rel, **dict(opts, fromto=False))
        st, t, dist, pair = (x.reshape(B, K, W - 1) for x in (st, t, dist, pair))
        bad = (st & 3) != 0
        free = ~bad.any(dim=2)
        seg = torch.where(free, dist.argmin(dim=2), bad.int().argmax(dim=2))      # (argmax of a 0 / 1 tensor: the first 1)
        pick = lambda x: x.gather(2, seg[..., None])[..., 0]                        # noqa: E731
        return free, torch.where(free, torch.full_like(seg, -1), seg), pick(t), pick(dist), pick(pair)

    def _arm_site(self, who, arm, site):
        """site None: the arm's `eef_site` (arm 0 or 1); a name or a model site id otherwise"""
        from .backend import ctrl_desc

        if site is None:
            d = ctrl_desc(self.env.cfg)
            if arm == 0:
                return int(d.eef_site)
            if arm == 1 and d.narm == 2:
                return int(d.eef_site2)
            raise ValueError(f"{who}: site=None needs one arm's eef_site, got arm {arm!r}")
        if isinstance(site, str):
            names = self.env.model.flat.names["site"]
            if site not in names:
                raise KeyError(f"no site named {site!r}")
            return names.index(site)
        return int(site)

    def config_inverse_dynamics(self, q, qd=None, qdd=None, arm=0, attach=None, held=None, rel=None):
        """Can the arm hold or execute this?  q (and qd, qdd, each None for zeros) [n_envs, K, n] (2-D for K = 1) candidate joint positions, velocities and
        accelerations of the arm -> tau [n_envs, K, n], the joint torques that produce qdd at (q, qd):  M qdd + Coriolis / centrifugal + gravity + joint
        damping, M with the armature (HipBatch.config_inverse_dynamics).  Every joint that is not the arm's -- fingers, objects, the other arm -- is held
        where it is, at rest; the hand and fingers ride along as load.  The simulation state is not touched.  arm: as config_fk.  With solve_ik:

            q, err, it, ok = env.solve_ik(pos, quat)
            holdable = ok & (env.config_gravity_torque(q).abs() <= limit).all(-1)

        THE PAYLOAD OF A GRASPED OBJECT counts only if the call says so, as in config_clearance: attach = [(body, carrier), ...] by name or id (carrier None:
        the body of the arm's eef_site), held [n_envs] or [n_envs, n] (None: all held), rel [n_envs, n, 7] (None: the env's current poses).  In the envs that
        hold it the object is rigid load on its carrier, with the env's own mass and inertia; an env that does not returns the empty-hand bits:

            tau = env.config_gravity_torque(q, attach=[("cube_main", None)], held=grasped)

        The same three arguments mean the same on config_gravity_torque, config_mass_matrix, config_jacobian, config_forward_dynamics, config_mass_solve,
        config_opspace and path_torques.  NOT included: tendon, fluid, friction loss, actuator, contact, equality and applied forces; grasp forces."""
        return self.env.batch.config_inverse_dynamics(self._arm_dofs("config_inverse_dynamics", arm), q, qd=qd, qdd=qdd, attach=self._attach_ids("config_inverse_dynamics", attach, arm), held=held, rel=rel)

    def config_gravity_torque(self, q, arm=0, attach=None, held=None, rel=None):
        """The torques that hold the arm still at q: config_inverse_dynamics at zero velocity and acceleration (JOINT_TORQUE feed-forward).  attach / held /
        rel: with the object in hand."""
        return self.config_inverse_dynamics(q, arm=arm, attach=attach, held=held, rel=rel)

    def config_mass_matrix(self, q, arm=0, attach=None, held=None, rel=None):
        """The joint-space inertia of the arm at candidate joint vectors -> M [n_envs, K, n, n] (HipBatch.config_mass_matrix): every other joint locked,
        armature on the diagonal, symmetric bit for bit.  arm: as config_fk; with arm="both" the arm-to-arm blocks are exactly zero."""
        return self.env.batch.config_mass_matrix(self._arm_dofs("config_mass_matrix", arm), q, attach=self._attach_ids("config_mass_matrix", attach, arm), held=held, rel=rel)

    def config_jacobian(self, q, arm=0, site=None, attach=None, held=None, rel=None):
        """mj_jacSite at candidate arm joint vectors -> (jacp, jacr) [n_envs, K, 3, n] in the arm's columns (HipBatch.config_jacobian).  site: a name or a
        model site id; None: the arm's `eef_site`.  arm: as config_fk (site=None needs arm 0 or 1).  With attach the site may sit on the carried object."""
        return self.env.batch.config_jacobian(self._arm_site("config_jacobian", arm, site), self._arm_dofs("config_jacobian", arm), q, attach=self._attach_ids("config_jacobian", attach, arm), held=held, rel=rel)

    def config_forward_dynamics(self, q, qd=None, tau=None, arm=0, return_ok=False, attach=None, held=None, rel=None):
        """What acceleration does this torque give here?  q (and qd, tau, each None for zeros) [n_envs, K, n] (2-D for K = 1) candidate joint positions,
        velocities and joint torques of the arm -> qdd [n_envs, K, n] = M(q)^-1 (tau - Coriolis / centrifugal - gravity - joint damping)
        (HipBatch.config_forward_dynamics): the exact inverse of config_inverse_dynamics, with its conventions and its limits -- every joint that is not the
        arm's is locked, and no tendon, fluid, friction-loss, actuator, contact, equality or applied force acts.  return_ok=True: -> (qdd, ok bool
        [n_envs, K]); where ok is False M was not positive definite in fp32 and qdd is NaN.  arm: as config_fk."""
        return self.env.batch.config_forward_dynamics(self._arm_dofs("config_forward_dynamics", arm), q, qd=qd, tau=tau, return_ok=return_ok, attach=self._attach_ids("config_forward_dynamics", attach, arm), held=held, rel=rel)

    def config_mass_solve(self, q, rhs, arm=0, return_ok=False, attach=None, held=None, rel=None):
        """M(q)^-1 rhs at candidate arm joint vectors: rhs [n_envs, K, n, r] (r <= 16) or [n_envs, K, n] -> x of rhs's shape (HipBatch.config_mass_solve)."""
        return self.env.batch.config_mass_solve(self._arm_dofs("config_mass_solve", arm), q, rhs, return_ok=return_ok, attach=self._attach_ids("config_mass_solve", attach, arm), held=held, rel=rel)

    def config_opspace(self, q, arm=0, site=None, return_ok=False, attach=None, held=None, rel=None):
        """What is the end effector's apparent inertia here?  -> (lambda_inv [n_envs, K, 6, 6], minv_jt [n_envs, K, n, 6]) at candidate arm joint vectors
        (HipBatch.config_opspace): with J = [jacp; jacr] of config_jacobian, minv_jt = M^-1 J^T and lambda_inv = J M^-1 J^T, symmetric bit for bit.  The
        inertia itself takes a pseudo-inverse, as robosuite does it: Lambda = torch.linalg.pinv(lambda_inv), Jbar = minv_jt @ Lambda.  site, arm: as
        config_jacobian."""
        return self.env.batch.config_opspace(self._arm_site("config_opspace", arm, site), self._arm_dofs("config_opspace", arm), q, return_ok=return_ok, attach=self._attach_ids("config_opspace", attach, arm), held=held, rel=rel)

    def config_inverse_dynamics_grad(self, q, qd=None, qdd=None, arm=0):
        """config_inverse_dynamics and its analytic first derivatives at candidate arm joint vectors -> (tau [n_envs, K, n], dtau_dq, dtau_dqd
        [n_envs, K, n, n]), entry [i, j] = d tau_i / d q_j (resp. qd_j) (HipBatch.config_inverse_dynamics_grad); d tau / d qdd is config_mass_matrix.
        tau is config_inverse_dynamics's, bit for bit.  arm: as config_fk.  No attach."""
        return self.env.batch.config_inverse_dynamics_grad(self._arm_dofs("config_inverse_dynamics_grad", arm), q, qd=qd, qdd=qdd)

    def config_inverse_dynamics_jvp(self, q, qd, qdd, dq=None, dqd=None, dqdd=None, arm=0):
        """The derivative of config_inverse_dynamics at (q, qd, qdd) along one direction (dq, dqd, dqdd) per candidate, each None for zeros -> dtau
        [n_envs, K, n], in one tangent walk on the device (HipBatch.config_inverse_dynamics_jvp)."""
        return self.env.batch.config_inverse_dynamics_jvp(self._arm_dofs("config_inverse_dynamics_jvp", arm), q, qd, qdd, dq=dq, dqd=dqd, dqdd=dqdd)

    def config_forward_dynamics_grad(self, q, qd=None, tau=None, arm=0, return_ok=False):
        """The linearisation qdd = f(q, qd, tau) of the arm at candidates, for iLQR / MPC -> (qdd [n_envs, K, n], dqdd_dq, dqdd_dqd [n_envs, K, n, n])
        (HipBatch.config_forward_dynamics_grad; return_ok=True: ok behind them).  qdd and ok are config_forward_dynamics's, bit for bit; d qdd / d tau is
        M^-1: config_mass_solve(q, identity).  No attach."""
        return self.env.batch.config_forward_dynamics_grad(self._arm_dofs("config_forward_dynamics_grad", arm), q, qd=qd, tau=tau, return_ok=return_ok)

    def inverse_dynamics(self, q, qd=None, qdd=None, arm=0):
        """config_inverse_dynamics as a DIFFERENTIABLE torch value: forward returns the plain call's bits; backward contracts the output's gradient with the
        device's analytic blocks, g_q = g . dtau_dq, g_qd = g . dtau_dqd, g_qdd = M g --

            q.requires_grad_(True)
            env.inverse_dynamics(q, qd, qdd).square().sum().backward()      # q.grad is filled

        The blocks are computed only if q or qd needs a gradient, config_mass_matrix only if qdd does; nothing is computed for an input that needs none.
        First order only (no second derivatives).  No attach."""
        return _inverse_dynamics_fn().apply(self, arm, q, qd, qdd)

    def path_torques(self, waypoints, dt, arm=0, attach=None, held=None, rel=None, differentiable=False):
        """The torques along joint-space paths: is the motion executable, not merely collision-free?  waypoints [n_envs, K, W, n]: K paths per env of W arm
        joint vectors `dt` seconds apart -> tau [n_envs, K, W, n].  Velocities are central differences of the waypoints, one-sided at the two ends, and
        accelerations the same differences of the velocities, formed in torch; then ONE config_inverse_dynamics call on the K W candidates.  Compare
        tau.abs().amax(2) with the actuators' limits.  attach / held / rel: the torques with the object in hand, as config_inverse_dynamics.
        differentiable=True: the one device call goes through inverse_dynamics, so path_torques(w, dt, differentiable=True).square().sum().backward() fills
        w.grad -- the effort cost of a trajectory optimiser, beside collision_cost.  It does not carry attach."""
        import torch

        if not (isinstance(waypoints, torch.Tensor) and waypoints.dim() == 4 and waypoints.shape[2] >= 2):
            raise ValueError(f"path_torques: waypoints must be a tensor [n_envs, K, W, n] with W >= 2, got {tuple(getattr(waypoints, 'shape', ()))}")
        if not dt > 0:
            raise ValueError(f"path_torques: dt {dt!r} is not > 0")
        if differentiable and attach is not None:
            raise ValueError("path_torques: differentiable=True does not carry attach (the derivatives of the dynamics have no attached form)")
        B, K, W, n = waypoints.shape
        w = waypoints.float()
        qd = torch.gradient(w, spacing=float(dt), dim=2)[0]
        qdd = torch.gradient(qd, spacing=float(dt), dim=2)[0]
        flat = lambda x: x.reshape(B, K * W, n)      # noqa: E731
        if differentiable:
            return self.inverse_dynamics(flat(w), flat(qd), flat(qdd), arm=arm).reshape(B, K, W, n)
        return self.config_inverse_dynamics(flat(w), qd=flat(qd), qdd=flat(qdd), arm=arm, attach=attach, held=held, rel=rel).reshape(B, K, W, n)

    def enable_applied_forces(self, on: bool = True):
        """Honour `qfrc_applied` and `xfrc_applied` in `step` (off by default: the control step then reads neither).  An env that reports `done`
        has both rows zeroed for its next episode, in the same step, so a force written after seeing `done` acts on the new episode."""
        self.env.batch.set_applied_forces(on)

    @property
    def qfrc_applied(self):
        """mjData.qfrc_applied of every env, [n_envs, nv]: a device tensor aliasing the batch; an in-place write on the current stream lands before the next `step`."""
        return self.env.batch.tensor("qfrc_applied")

    @property
    def xfrc_applied(self):
        """mjData.xfrc_applied of every env, [n_envs, nbody, 6] (force, torque; world frame, at the body COM): a device tensor aliasing the batch."""
        return self.env.batch.tensor("xfrc_applied")

    def set_body_wrench(self, body_name: str, wrench, envs=None):
        """xfrc_applied[envs, body] = wrench (6 values: force then torque, world frame, at the body COM; or one row of 6 per selected env).
        Takes effect in `step` once `enable_applied_forces()` was called."""
        import torch

        bid = body_wrench_id(self.env.model, body_name)
        x = self.xfrc_applied
        w = torch.as_tensor(wrench, dtype=torch.float32, device=x.device)
        idx = slice(None) if envs is None else torch.as_tensor(envs, dtype=torch.long, device=x.device)
        n = self.n_envs if envs is None else int(idx.numel())
        if tuple(w.shape) not in ((6,), (n, 6)):
            raise ValueError(f"set_body_wrench: wrench must have shape (6,) or ({n}, 6), got {tuple(w.shape)}")
        x[idx, bid] = w

    def key(self, obs, name: str):
        return obs[:, self.obs_slices[name]]

    def flat_obs(self, obs, keys=None):
        """GymWrapper default: ["object-state", "robot0_proprio-state"] = object keys then robot keys; or an explicit list of observable keys."""
        import torch

        keys = self._object_keys + self._proprio_keys if keys is None else keys
        return torch.cat([obs[:, self.obs_slices[k]] for k in keys], dim=1)


_COST_FN = None


def _collision_cost_fn():
    """the torch.autograd.Function behind VecEnv.collision_cost (built on first use: this module does not import torch)"""
    global _COST_FN
    if _COST_FN is None:
        import torch

        class CollisionCost(torch.autograd.Function):
            @staticmethod
            def forward(ctx, q, env, d_safe, arm, opts):
                cost, grad, _, _ = env.config_collision_cost(q.detach(), d_safe, arm=arm, **opts)
                ctx.save_for_backward(grad)
                return cost

            @staticmethod
            def backward(ctx, grad_out):
                (grad,) = ctx.saved_tensors
                return grad_out[..., None] * grad, None, None, None, None

        _COST_FN = CollisionCost
    return _COST_FN


_ID_FN = None


def _inverse_dynamics_fn():
    """the torch.autograd.Function behind VecEnv.inverse_dynamics (built on first use: this module does not import torch)"""
    global _ID_FN
    if _ID_FN is None:
        import torch

        class InverseDynamics(torch.autograd.Function):
            @staticmethod
            def forward(ctx, env, arm, q, qd, qdd):
                det = lambda x: None if x is None else x.detach()      # noqa: E731
                need_q, need_qd, need_qdd = ctx.needs_input_grad[2:5]
                if need_q or need_qd:
                    tau, gq, gv = env.config_inverse_dynamics_grad(det(q), det(qd), det(qdd), arm=arm)
                else:
                    tau, gq, gv = env.config_inverse_dynamics(det(q), det(qd), det(qdd), arm=arm), None, None
                M = env.config_mass_matrix(det(q), arm=arm) if need_qdd else None
                ctx.save_for_backward(gq if need_q else None, gv if need_qd else None, M)
                return tau

            @staticmethod
            def backward(ctx, g):
                gq, gv, M = ctx.saved_tensors
                vjp = lambda J: None if J is None else torch.einsum("...i,...ij->...j", g, J)      # noqa: E731
                return None, None, vjp(gq), vjp(gv), vjp(M)      # (M is symmetric bit for bit: g . M = M g)

        _ID_FN = InverseDynamics
    return _ID_FN


def gym_flags(end_reason):
    """(terminated, truncated) of gymnasium for RSIM_END_REASON values: success (2) and a requested end (4) terminate, the horizon (1) and the bad-state
    guard (3) truncate.  Works on torch tensors and numpy arrays."""
    return (end_reason == 2) | (end_reason == 4), (end_reason == 1) | (end_reason == 3)


def body_wrench_id(model, body_name: str) -> int:
    """Index of `body_name` for xfrc_applied: raises on an unknown name (where mj_name2id would give -1)."""
    bid = model.name2id("body", body_name)
    if bid < 0:
        raise KeyError(f"no body named {body_name!r} in the model")
    return bid


class AlternatingVecEnv:
    """The batch as two halves stepped alternately -- the "alternating sampler" of RL frameworks, closed-loop compatible:

        env = AlternatingVecEnv("Lift", 4096, flat, cfg)
        obs = env.reset()                                # [obs of half 0, obs of half 1]
        for k in (0, 1): env.step_half(k, policy(obs[k]))
        while training:
            for k in (0, 1):
                o, r, d, info = env.wait_half(k)         # half k's step has completed: its observations are final
                env.step_half(k, policy(o))              # its next step is enqueued while the OTHER half is still stepping

    A lockstep launch of all envs ends when its slowest env does, with the chip half empty for the last third of it; here that
    drain is filled by the other half's launch, and a half's step t + 1 still depends only on its own step t.  Each half is a VecEnv of its own
    (its own rsim batch and HIP stream); env i behaves exactly as env i of one big batch (per-env seeding by GLOBAL env id).
    Measured by `bench.py` as `config.double_buffered` (Lift 4096: 1.33 M env-steps/s against 1.13 M lockstep on the same box)."""

    def __init__(self, env_name: str, n_envs: int, flat, cfg, env_ids=None, **kw):
        ids = np.arange(n_envs) if env_ids is None else np.asarray(env_ids)
        h = len(ids) // 2
        if h < 1:
            raise ValueError("AlternatingVecEnv needs at least two envs")
        self.halves = [VecEnv(env_name, h, flat, cfg, env_ids=ids[:h], **kw), VecEnv(env_name, len(ids) - h, flat, cfg, env_ids=ids[h:], **kw)]
        self.n_envs, self.action_dim, self.obs_dim = len(ids), self.halves[0].action_dim, self.halves[0].obs_dim

    def reset(self, seed=None):
        return [e.reset(seed=seed) for e in self.halves]

    def step_half(self, k: int, actions):
        """Enqueue one control step of half k (returns at once)."""
        self.halves[k].env.step(actions)

    def wait_half(self, k: int):
        """Block until half k's last enqueued step has completed; (obs, reward, done, info) of that step, device tensors."""
        e = self.halves[k]
        e.env.batch.sync()
        return e.env.obs(), e.env.reward(), e.env.batch.tensor("done"), e._info()

    def end_episodes(self, mask):
        """VecEnv.end_episodes over both halves (mask: [n_envs], half 0's envs first); returns [obs of half 0, obs of half 1]."""
        h = self.halves[0].n_envs
        return [self.halves[0].end_episodes(mask[:h]), self.halves[1].end_episodes(mask[h:])]


class _Box:
    """Stand-in for gymnasium.spaces.Box when gymnasium is not installed (same attribute names)."""

    def __init__(self, low, high, shape, dtype=np.float32):
        self.low, self.high, self.shape, self.dtype = np.broadcast_to(np.asarray(low, dtype=dtype), shape), np.broadcast_to(np.asarray(high, dtype=dtype), shape), tuple(shape), dtype


def _box(low, high, shape):
    try:
        from gymnasium import spaces

        return spaces.Box(low=np.broadcast_to(np.float32(low), shape).copy(), high=np.broadcast_to(np.float32(high), shape).copy(), dtype=np.float32)
    except ImportError:
        return _Box(low, high, shape)


class GymVecEnv:
    """gymnasium.vector-shaped face of VecEnv, with the conventions of the reference's single-env GymWrapper (wrappers/gym_wrapper.py:45-163):
    flattened observation = the chosen keys concatenated (default `object-state` then `robot0_proprio-state`), reward range (0, reward_scale),
    the horizon reports `terminated` (the reference passes its `done` there) and `truncated` is always False.  With an early-end rule armed on the VecEnv
    gymnasium's distinction applies instead: `terminated` = the task ended the episode (success, or the caller's request),
    `truncated` = it was cut short (horizon, bad-state guard).  Episodes restart on the device:
    after a terminated step `obs` is already the reset observation (gymnasium's autoreset) and info["final_observation"] holds the last record of
    the finished episode for the envs flagged in info["_final_observation"]."""

    def __init__(self, env: VecEnv, keys=None):
        self.env, self.keys = env, keys
        self.num_envs = env.n_envs
        dim = int(env.flat_obs(env.env.obs(), keys).shape[1]) if keys is not None else env.obs_dim
        lo, hi = env.action_spec
        self.single_observation_space, self.single_action_space = _box(-np.inf, np.inf, (dim,)), _box(lo[0], hi[0], (env.action_dim,))
        self.observation_space, self.action_space = _box(-np.inf, np.inf, (self.num_envs, dim)), _box(lo[0], hi[0], (self.num_envs, env.action_dim))

    def reset(self, seed=None, options=None):
        if seed is not None and not isinstance(seed, int):
            raise TypeError("Seed must be an integer type!")      # gym_wrapper.py:139-143
        # the reference's wrapper seeds numpy's global generator with it (gym_wrapper.py:136-143); the batched envs have one generator each, so a
        # seed re-keys them: env i's episode stream becomes default_rng(seed + i).  Same seed -> same episodes, another seed -> other episodes.
        return self.env.flat_obs(self.env.reset(seed=seed), self.keys), {}

    def step(self, actions):
        import torch

        obs, reward, done, info = self.env.step(actions)
        ended = done.to(torch.bool)
        if getattr(self.env, "early_end_armed", False):
            term, trunc = gym_flags(info["end_reason"])
        else:                                    # as ever: the horizon is passed on as `terminated`
            term, trunc = ended, torch.zeros_like(ended)
        out = {"success": info["success"], "final_observation": self.env.flat_obs(info["terminal_obs"], self.keys), "_final_observation": ended}
        if "end_reason" in info:
            out["end_reason"] = info["end_reason"]
        return self.env.flat_obs(obs, self.keys), reward, term, trunc, out

    def close(self):
        pass
