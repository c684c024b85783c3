"""Ray casting on the device (csrc/rsim_ray.hip) against the fp64 host mirror (robosuite_amd/raycast.py) on the state read back from the device: ray
queries, depth / segmentation images, the rangefinder sensor, every filter, per-env geometry.

On well-conditioned rays the geom id must be equal and the distance error |t - t_ref| / max(1, t_ref) stay under BOUND: four times the worst value one GPU
run measured per scene (profiles/raycast_parity.txt; the margin is for one box, one run and pose-dependent rounding).  A ray is ill-conditioned, and left
out, when the mirror alone says so (raycast.well_conditioned: tilted by 1e-4 rad in four directions it changes geom, or its distance moves by more than
1 %); at most 10 % of a scene's rays may be left out (asserted here and, on the mirror alone, in tests/test_raycast_host.py)."""
import numpy as np
import pytest
import torch

from robosuite_amd import backend, mjcf, raycast
from tests import raycast_scenes as S
from tests.util import make_hip

pytestmark = pytest.mark.gpu

# worst measured error per scene (profiles/raycast_parity.txt) x 4
MEASURED = {"A": 4.785e-6, "B": 7.763e-6, "C": 5.337e-6, "rangefinder": 2.486e-7}
BOUND = {k: 4 * v for k, v in MEASURED.items()}
WORST = {}      # scene -> worst error seen in this run (printed by every check: `pytest -s` shows the figures)


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device="cuda")


def check(scene, flat, xp, xq, o, d, t, g, cap=True, **opts):
    """one env: device (t, g) against the mirror on the well-conditioned rays; returns the number of rays left out"""
    t_ref, g_ref = raycast.cast(flat, xp, xq, o, d, **opts)
    ok = raycast.well_conditioned(flat, xp, xq, o, d, **opts)
    err = S.rel_err(t, t_ref)[ok]
    worst = float(err.max()) if ok.any() else 0.0
    WORST[scene] = max(WORST.get(scene, 0.0), worst)
    print(f"raycast parity scene {scene}: {int(ok.sum())}/{len(ok)} rays, worst {worst:.3e} (bound {BOUND[scene]:.1e})")
    off = np.flatnonzero(ok & (np.asarray(g) != g_ref))
    assert len(off) == 0, (scene, [(int(i), int(np.asarray(g)[i]), float(np.asarray(t)[i]), int(g_ref[i]), float(t_ref[i])) for i in off[:8]])      # (ray, device geom, t, mirror geom, t)
    assert worst <= BOUND[scene], (scene, worst)
    if cap:
        assert (~ok).sum() <= 0.10 * len(ok), (scene, int((~ok).sum()), len(ok))
    return int((~ok).sum())


# ---- Scene A: one geom of each type ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_a(tmp_path_factory):
    xml, adir = S.scene_a(tmp_path_factory.mktemp("raycast_a"))
    flat = mjcf.compile_mjcf(xml, asset_dir=adir)
    hm, hb = make_hip(flat, None, B=3)
    hb.set("qpos", S.scene_a_qpos(flat).astype(np.float32))
    hb.forward()
    return flat, hm, hb, hb.get("xpos").astype(np.float64), hb.get("xquat").astype(np.float64)


@pytest.mark.parametrize("n", (1, 63, 65, 257))
def test_ray_queries_scene_a(scene_a, n):
    flat, hm, hb, xp, xq = scene_a
    rays = [S.seeded_rays(flat, xp[e], xq[e], n, seed=100 + e) for e in range(3)]
    o, d = np.stack([r[0] for r in rays]), np.stack([r[1] for r in rays])
    dist, gid = hb.raycast(_dev(o), _dev(d))
    assert dist.shape == gid.shape == (3, n) and dist.dtype == torch.float32 and gid.dtype == torch.int32
    dist, gid = dist.cpu().numpy(), gid.cpu().numpy()
    o32, d32 = o.astype(np.float32).astype(np.float64), d.astype(np.float32).astype(np.float64)      # the rays as the device saw them
    for e in range(3):
        check("A", flat, xp[e], xq[e], o32[e], d32[e], dist[e], gid[e], cap=n >= 63)
    if n == 257:
        assert (gid < 0).any() and (dist[gid < 0] == -1).all() and set(np.unique(gid[gid >= 0])) >= set(range(7))      # misses read (-1, -1); every type is hit


def test_every_filter_scene_a(scene_a):
    flat, hm, hb, xp, xq = scene_a
    rays = [S.seeded_rays(flat, xp[e], xq[e], 65, seed=200 + e) for e in range(3)]
    o, d = np.stack([r[0] for r in rays]).astype(np.float32), np.stack([r[1] for r in rays]).astype(np.float32)
    fb = flat.names["body"].index("fb")
    seen = []
    for opts in (dict(geomgroup=0b001), dict(geomgroup=0b100), dict(static=False), dict(bodyexclude=fb), dict(geomgroup=0b101, static=False, bodyexclude=fb)):
        dist, gid = hb.raycast(_dev(o), _dev(d), **opts)
        dist, gid = dist.cpu().numpy(), gid.cpu().numpy()
        for e in range(3):
            check("A", flat, xp[e], xq[e], o[e].astype(np.float64), d[e].astype(np.float64), dist[e], gid[e], cap=False, **opts)
        seen.append(set(np.unique(gid).tolist()))
    names = {n: i for i, n in enumerate(flat.names["geom"])}
    assert names["sph"] not in seen[0] and seen[1] <= {-1, names["sph"]} and names["floor"] not in seen[2] and names["box"] not in seen[3]
    assert all(names["ghost"] not in s for s in seen)                   # alpha 0 never counts


def test_per_env_box_size(tmp_path):
    xml, adir = S.scene_a(tmp_path)
    flat = mjcf.compile_mjcf(xml, asset_dir=adir)
    hm, hb = make_hip(flat, None, B=2, per_env=True)
    g = flat.names["geom"].index("box")
    size = hb.param_get("geom_size")
    size[1, g] = size[1, g] * [2.0, 0.5, 1.5]
    hb.param_set("geom_size", size[1:2], env0=1)
    hb.forward()
    xp, xq = hb.get("xpos").astype(np.float64), hb.get("xquat").astype(np.float64)
    live = hb.param_get("geom_size")
    assert np.allclose(live[1, g], size[1, g]) and not np.allclose(live[0, g], live[1, g])
    c, R = S.geom_world(flat, xp[0], xq[0])
    rng = np.random.default_rng(3)
    tgt = c[g] + (rng.uniform(-1, 1, (65, 3)) * live[1, g] * 1.2) @ R[g].T        # points in and around the LARGER box
    o = np.broadcast_to(c[g] + np.array([0.3, -0.6, 0.9]), tgt.shape).astype(np.float32)
    d = (tgt - o).astype(np.float32)
    dist, gid = hb.raycast(_dev(np.stack([o, o])), _dev(np.stack([d, d])))
    dist, gid = dist.cpu().numpy(), gid.cpu().numpy()
    for e in range(2):
        check("A", flat, xp[e], xq[e], o.astype(np.float64), d.astype(np.float64), dist[e], gid[e], cap=False, params={"geom_size": live[e]})
    assert (gid[0] == g).sum() != (gid[1] == g).sum() and (gid[1] == g).sum() >= 10      # the two envs see boxes of different sizes


# ---- Scene B: more geoms than one staging chunk ---------------------------------------------------------------------------------------------------------
def test_ray_queries_scene_b_past_one_chunk():
    flat = mjcf.compile_mjcf(S.scene_b_xml())
    hm, hb = make_hip(flat, None, B=2)
    hb.set("qpos", np.array([[0.3, -0.2, 0.5, 0.1], [-0.4, 0.6, 0.0, 0.9]], dtype=np.float32))
    hb.forward()
    xp, xq = hb.get("xpos").astype(np.float64), hb.get("xquat").astype(np.float64)
    rays = [S.seeded_rays(flat, xp[e], xq[e], 257, seed=5 + e) for e in range(2)]
    o, d = np.stack([r[0] for r in rays]).astype(np.float32), np.stack([r[1] for r in rays]).astype(np.float32)
    dist, gid = hb.raycast(_dev(o), _dev(d))
    dist, gid = dist.cpu().numpy(), gid.cpu().numpy()
    for e in range(2):
        check("B", flat, xp[e], xq[e], o[e].astype(np.float64), d[e].astype(np.float64), dist[e], gid[e])
    assert gid.max() >= 64 and (gid < 64).any()


# ---- Scene C: Lift, mesh hulls, cameras -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene_c():
    flat, cfg = S.lift()
    hm, hb = make_hip(flat, cfg, B=2)
    hb.set("qpos", np.tile(S.lift_init_qpos(flat, cfg), (2, 1)).astype(np.float32))
    hb.forward(); hb.ctrl_reset()
    q0 = hb.get("qpos")
    a = torch.zeros((2, hm.action_dim), device="cuda"); a[:, 0] = 0.8; a[:, 2] = -0.6; a[:, 4] = 0.5
    hb.control_step(a, 25)
    q1 = hb.get("qpos")
    q = np.stack([q0[0], q1[1]])            # the two envs one control step apart
    assert np.abs(q[0] - q[1]).max() > 1e-3
    hb.set("qpos", q); hb.set("qvel", 0)
    hb.forward()
    return flat, cfg, hm, hb, hb.get("xpos").astype(np.float64), hb.get("xquat").astype(np.float64)


@pytest.mark.parametrize("cam", ("front", "hand"))
@pytest.mark.parametrize("H,W,fovy", [(5, 7, 45.0), (5, 7, 90.0), (24, 32, 45.0), (24, 32, 90.0)])
def test_render_depth_scene_c(scene_c, cam, H, W, fovy):
    flat, cfg, hm, hb, xp, xq = scene_c
    camera = S.lift_cameras(flat)[cam]
    camera = raycast.Camera(camera.body, camera.pos, camera.quat, fovy)
    depth, seg = hb.render_depth(camera, H, W, segmentation=True)
    only = hb.render_depth(camera, H, W)
    assert depth.shape == seg.shape == (2, H, W) and torch.equal(only, depth)
    depth, seg = depth.cpu().numpy(), seg.cpu().numpy()
    assert np.isinf(depth[seg < 0]).all() and np.isfinite(depth[seg >= 0]).all() and (seg >= 0).any()
    cam32 = raycast.Camera(camera.body, tuple(np.float32(camera.pos).astype(float)), tuple(np.float32(camera.quat).astype(float)), fovy)
    for e in range(2):
        o, d = raycast.pixel_rays(cam32, xp[e], xq[e], H, W)
        check("C", flat, xp[e], xq[e], o, d, np.where(seg[e] >= 0, depth[e], -1.0).ravel(), seg[e].ravel())
    if cam == "front" and (H, W, fovy) == (24, 32, 45.0):
        gt = np.asarray(flat.arrays["geom_type"]).ravel()
        assert (gt[seg[seg >= 0]] == mjcf.GEOM_MESH).sum() >= 20 and not np.array_equal(seg[0], seg[1])     # the robot's hulls are in view, and the arm moved


def test_ray_queries_scene_c(scene_c):
    flat, cfg, hm, hb, xp, xq = scene_c
    rays = [S.seeded_rays(flat, xp[e], xq[e], 257, seed=300 + e, reach=1.2) for e in range(2)]
    o, d = np.stack([r[0] for r in rays]).astype(np.float32), np.stack([r[1] for r in rays]).astype(np.float32)
    dist, gid = hb.raycast(_dev(o), _dev(d), geomgroup=0b011)
    dist, gid = dist.cpu().numpy(), gid.cpu().numpy()
    for e in range(2):
        check("C", flat, xp[e], xq[e], o[e].astype(np.float64), d[e].astype(np.float64), dist[e], gid[e], geomgroup=0b011)


# ---- the rangefinder sensor --------------------------------------------------------------------------------------------------------------------------------
def test_rangefinder_scene_a(scene_a):
    flat, hm, hb, xp, xq = scene_a
    adr, dim, carried = hm.sensor_slice("rf_tip")
    assert dim == 1 and carried and all(c for _, _, c, _ in hm.sensor_status())
    row = hb.get("sensordata")
    for e in range(3):
        ref = raycast.rangefinder_values(flat, xp[e], xq[e])[flat.names["sensor"].index("rf_tip")]
        err = float(S.rel_err(row[e, adr], ref))
        print(f"rangefinder scene A env {e}: {row[e, adr]:.7f} vs {ref:.7f}, error {err:.3e}")
        assert ref > 0 and err <= BOUND["rangefinder"]
    fp = hm.sensor_slice("fp_tip")[0]
    assert np.abs(row[:, fp:fp + 3]).max() > 0.1                        # the k_sensors entries beside it are still written


def test_rangefinder_on_a_moving_site_after_forward_and_control_step():
    flat0, cfg = S.lift()
    site = flat0.names["site"].index("gripper0_right_grip_site")
    flat = S.add_rangefinder(flat0, "grip_range", site)
    hm, hb = make_hip(flat, cfg, B=2)
    assert hm.sensor_slice("grip_range")[2] and hm.int("nsensor_zero") == 0
    adr = hm.sensor_slice("grip_range")[0]
    idx = flat.names["sensor"].index("grip_range")

    def both():
        row = hb.get("sensordata")                                      # (after a fused step: brings the derived arrays up to the current state first)
        xp, xq = hb.get("xpos").astype(np.float64), hb.get("xquat").astype(np.float64)
        out = []
        for e in range(2):
            ref = raycast.rangefinder_values(flat, xp[e], xq[e])[idx]
            err = float(S.rel_err(row[e, adr], ref))
            print(f"rangefinder Lift env {e}: {row[e, adr]:.7f} vs {ref:.7f}, error {err:.3e}")
            assert ref > 0 and err <= BOUND["rangefinder"]
            out.append(ref)
        return out

    hb.forward(); hb.ctrl_reset()
    first = both()
    a = torch.zeros((2, hm.action_dim), device="cuda"); a[0, 2] = -0.8; a[1, 2] = 0.8      # env 0 moves down, env 1 up
    for _ in range(3):
        hb.control_step(a, 25)
    moved = both()
    assert abs(moved[0] - first[0]) > 0.005 and abs(moved[1] - first[1]) > 0.005 and abs(moved[0] - moved[1]) > 0.005      # the site moved, and differently per env
    assert np.isclose(hb.sensor("grip_range").cpu().numpy()[:, 0], hb.get("sensordata")[:, adr]).all()


# ---- the boundary ----------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_fail_by_name(scene_a):
    import ctypes as C

    flat, hm, hb, xp, xq = scene_a
    L = backend.lib()
    o = torch.zeros((3, 4, 3), device="cuda"); t = torch.zeros((3, 4), device="cuda")
    opts = backend.RayOpts(0, 1, -1)
    P = lambda x: C.c_void_p(x.data_ptr())
    for args, word in (((hb.ptr, None, P(o), 4, C.byref(opts), P(t), None), b"origin_dev"), ((hb.ptr, P(o), P(o), 4, None, P(t), None), b"opts"),
                       ((hb.ptr, P(o), P(o), 4, C.byref(opts), None, None), b"dist_dev"), ((hb.ptr, P(o), P(o), 0, C.byref(opts), P(t), None), b"n_per_env"),
                       ((hb.ptr, P(o), P(o), 4, C.byref(backend.RayOpts(0, 1, 99)), P(t), None), b"bodyexclude")):
        assert L.rsim_ray(*args) != 0 and word in L.rsim_last_error(), word
    cam = lambda body=0, fovy=45.0: backend.CameraDesc(body, (C.c_float * 3)(0, 0, 2), (C.c_float * 4)(1, 0, 0, 0), fovy)
    img = torch.zeros((3, 4, 4), device="cuda")
    for args, word in (((hb.ptr, None, 4, 4, C.byref(opts), P(img), None), b"camera is NULL"), ((hb.ptr, C.byref(cam(body=77)), 4, 4, C.byref(opts), P(img), None), b"camera body 77"),
                       ((hb.ptr, C.byref(cam(fovy=180.0)), 4, 4, C.byref(opts), P(img), None), b"fovy"), ((hb.ptr, C.byref(cam(fovy=0.0)), 4, 4, C.byref(opts), P(img), None), b"fovy"),
                       ((hb.ptr, C.byref(cam()), 0, 4, C.byref(opts), P(img), None), b"image size"), ((hb.ptr, C.byref(cam()), 4, 4, C.byref(opts), None, None), b"depth_dev")):
        assert L.rsim_render_depth(*args) != 0 and word in L.rsim_last_error(), word
    with pytest.raises(backend.RsimError):
        hb.raycast(o[:, :, :2], o[:, :, :2])


def test_vecenv_and_batchstate_calls():
    from robosuite_amd.controllers import BatchState
    from robosuite_amd.vec_env import VecEnv

    flat, cfg = S.lift()
    env = VecEnv("Lift", 2, flat, cfg, horizon=50)
    env.reset()
    env.step(torch.zeros((2, env.action_dim), device="cuda"))
    cam = S.lift_cameras(flat)["front"]
    gl, seg_gl = env.render_depth(cam, 6, 8, segmentation=True)          # robosuite's default convention: the bottom row first
    cv, seg_cv = env.render_depth(cam, 6, 8, segmentation=True, convention="opencv")
    assert torch.equal(gl.flip(1), cv) and torch.equal(seg_gl.flip(1), seg_cv) and not torch.equal(gl, cv)
    want = env.env.batch.render_depth(cam, 6, 8)
    assert torch.equal(cv, want)
    o = torch.tensor([0.0, 0.0, 2.0], device="cuda").expand(2, 1, 3); d = torch.tensor([0.0, 0.0, -1.0], device="cuda").expand(2, 1, 3)
    t, g = env.raycast(o, d)
    assert (t > 0).all() and (g >= 0).all()
    st = BatchState(env.env.batch)
    t2, g2 = st.raycast(o, d)
    assert torch.equal(t, t2) and torch.equal(g, g2) and torch.equal(st.render_depth(cam, 6, 8), want)
    with pytest.raises(ValueError):
        env.render_depth(cam, 6, 8, convention="d3d")
    with pytest.raises(ValueError, match="no MJCF"):
        env.render_depth("frontview", 6, 8)
