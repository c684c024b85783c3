"""The fp64 mirror of the swept clearance query (robosuite_amd/sweep.py) against brute force.  CPU only.

  * the motion bound, the test of the derivation: solid points of every listed geom -- its centre and the mirror's support points (distance.support_full)
    along +- its three local axes, which are points fixed in the geom -- are followed over 257 uniform t; between neighbouring samples the worst displacement of
    a point of geom1 plus that of geom2 is <= L dt for every listed pair, with no allowance beyond 1e-12.  Scene T, two envs, six segments each per dof list
    (a dozen per list; the fingers are slides held off their reference position); also the chain with its own slide s1 held off its reference, and q0 == q1.
  * the certificate: FREE => the dense minimum of clearance.clearance over sweep_scenes.DENSE uniform samples is > margin; HIT at t => every dense sample in
    [0, t) is > margin and the clearance at q(t) is <= margin + slack.  All three statuses occur (UNDECIDED with max_steps small).
  * the thin wall (sweep_scenes.thin_wall): both ends and eight uniform samples between them read free by a centimetre, from this same mirror's clearance;
    sweep() reports HIT, with t where a dense scan finds the bar within margin + slack of the wall.
  * the condition for the GPU tests: with the seeds of sweep_scenes.segments the mirror decides every segment of the shapes tests/test_sweep.py runs
    on scene T within max_steps / 2 = 128 samples.  Worst step count of the mirror over those 331 segments: 119 (the device, same seeds: 119)."""
import numpy as np
import pytest

from robosuite_amd import clearance, distance, mjcf, sweep
from tests import clearance_scenes as S
from tests import sweep_scenes as W

B, K = 2, 6
GPU_SHAPES = ((3, 5), (65, 3), (2, 70))      # tests/test_sweep.py SHAPES


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    flat = S.scene_t(tmp_path_factory.mktemp("sweep_t"))
    return flat, S.f32(S.scene_t_qpos(flat, B)), clearance._model32(flat)


def solid_points(flat, xp, xq, geoms):
    """{geom: [7, 3]} world positions of the geom's centre and of its support points along +- its local axes (planes: none, they never move).  The support
    points are taken in the geom's own frame, where the axes are exact, and carried to the world as points fixed in the geom: asked along the world image
    of an axis, a box would answer with another corner whenever rounding tips a zero component the other way."""
    out = {}
    for g, G in distance.world_geoms(flat, xp, xq, geoms, S.params32(flat)).items():
        if G["type"] == mjcf.GEOM_PLANE:
            continue
        own = distance.make_geom(G["type"], G["size"], (0.0, 0.0, 0.0), np.eye(3), G["verts"])
        local = [(0.0, 0.0, 0.0)] + [distance.support_full(own, tuple(s * float(i == k) for i in range(3))) for k in range(3) for s in (1.0, -1.0)]
        out[g] = np.asarray(G["pos"]) + np.asarray(local) @ G["R"].T
    return out


def worst_pair_displacement(flat, m32, qpos, dofs, q0, q1, pairs, n=257):
    """max over neighbouring samples and listed pairs of (worst point displacement of geom1 + of geom2)"""
    geoms = sorted(set(int(g) for g in pairs.ravel()))
    prev, worst = None, 0.0
    for t in np.linspace(0.0, 1.0, n):
        xp, xq = clearance.fk(flat, qpos, dofs, W.at(q0, q1, t), model32=m32)
        cur = solid_points(flat, xp, xq, geoms)
        if prev is not None:
            d = {g: float(np.linalg.norm(cur[g] - prev[g], axis=1).max()) for g in cur}
            worst = max(worst, max(d.get(int(a), 0.0) + d.get(int(b), 0.0) for a, b in pairs))
        prev = cur
    return worst


@pytest.mark.parametrize("which", ("arm", "all"))
def test_motion_bound_holds_against_dense_displacements(scene, which):
    flat, qpos, m32 = scene
    dofs = S.dofs_t(flat, which)
    pairs = clearance.default_pairs(flat, dofs)
    q0, q1 = W.segments(flat, dofs, B, K)
    ratio = 0.0
    for e in range(B):
        for k in range(K):
            L = sweep.motion_bound(flat, qpos[e], dofs, q0[e, k], q1[e, k], pairs)
            got = worst_pair_displacement(flat, m32, qpos[e], dofs, q0[e, k], q1[e, k], pairs)
            assert got <= L / 256 + 1e-12, (e, k, got * 256, L)
            ratio = max(ratio, got * 256 / L)
    print(f"motion bound, dofs {which}: the worst dense displacement rate reaches {ratio:.3f} of L")
    assert ratio > 0.05      # (a bound that no motion comes near would be no test)


def test_motion_bound_with_a_held_slide_off_its_reference(scene):
    flat, qpos, m32 = scene
    dofs = S.dofs_of(flat, ("h0", "h2"))      # s1, between them, is held where the env has it
    j = flat.names["joint"].index("s1")
    qa = int(np.asarray(flat.arrays["jnt_qposadr"]).ravel()[j])
    pairs = clearance.default_pairs(flat, dofs)
    q0, q1 = W.segments(flat, dofs, B, K)
    for e in range(B):
        x = qpos[e, qa] - float(np.asarray(flat.arrays["qpos0"]).ravel()[qa])
        assert abs(x) > 0.01      # the slide's displacement lengthens the arm the first hinge swings
        for k in range(3):
            L = sweep.motion_bound(flat, qpos[e], dofs, q0[e, k], q1[e, k], pairs)
            assert worst_pair_displacement(flat, m32, qpos[e], dofs, q0[e, k], q1[e, k], pairs) <= L / 256 + 1e-12, (e, k)
            at_ref = qpos[e].copy(); at_ref[qa] -= x
            if x > 0:
                assert sweep.motion_bound(flat, at_ref, dofs, q0[e, k], q1[e, k], pairs) < L      # ... and the bound knows it


def test_no_motion_has_bound_zero_and_one_sample_decides(scene):
    flat, qpos, _ = scene
    dofs = S.dofs_t(flat, "all")
    q0, _ = W.segments(flat, dofs, B, K)
    seen = set()
    for e in range(B):
        for k in range(K):
            assert sweep.motion_bound(flat, qpos[e], dofs, q0[e, k], q0[e, k]) == 0.0
            st, t, d, tm, pair, ft, steps = sweep.sweep(flat, qpos[e], dofs, q0[e, k], q0[e, k], distmax=S.DISTMAX_T)
            ref = clearance.clearance(flat, qpos[e], dofs, q0[e, k], distmax=S.DISTMAX_T)
            assert steps == 1 and tm == 0.0 and (d, pair) == ref[:2] and np.array_equal(ft, ref[2])
            assert (st, t) == ((sweep.HIT, 0.0) if ref[0] <= 1e-3 else (sweep.FREE, 1.0))
            seen.add(st)
    assert seen == {sweep.FREE, sweep.HIT}


def dense_clearance(flat, m32, qpos, dofs, q0, q1, pairs, ts, distmax):
    return np.array([clearance.clearance(flat, qpos, dofs, W.at(q0, q1, t), pairs, distmax, poses=clearance.fk(flat, qpos, dofs, W.at(q0, q1, t), model32=m32))[0]
                     for t in ts])


@pytest.mark.parametrize("which,margin", (("arm", 0.0), ("all", 0.01)))
def test_certificate_against_dense_sampling(scene, which, margin):
    flat, qpos, m32 = scene
    dofs = S.dofs_t(flat, which)
    pairs = clearance.default_pairs(flat, dofs)
    q0, q1 = W.segments(flat, dofs, B, K)
    slack = sweep.DEFAULTS["slack"]
    seen = set()
    for e in range(B):
        for k in range(K):
            st, t, d, tm, pair, ft, steps = sweep.sweep(flat, qpos[e], dofs, q0[e, k], q1[e, k], pairs, distmax=S.DISTMAX_T, margin=margin)
            seen.add(st)
            assert st in (sweep.FREE, sweep.HIT) and 1 <= steps <= sweep.DEFAULTS["max_steps"] and 0.0 <= tm <= t <= 1.0
            ts = np.linspace(0.0, 1.0, W.DENSE)
            if st == sweep.FREE:
                assert t == 1.0
                c = dense_clearance(flat, m32, qpos[e], dofs, q0[e, k], q1[e, k], pairs, ts, S.DISTMAX_T)
                assert c.min() > margin, (e, k, c.min())
            else:
                c = dense_clearance(flat, m32, qpos[e], dofs, q0[e, k], q1[e, k], pairs, ts[ts < t], S.DISTMAX_T)
                assert len(c) == 0 or c.min() > margin, (e, k, t, c.min())
                here = clearance.clearance(flat, qpos[e], dofs, W.at(q0[e, k], q1[e, k], t), pairs, S.DISTMAX_T)
                assert here[0] <= margin + slack and (d, pair, tm) == (here[0], here[1], t)      # the last sample is the closest one
            # a short leash: three samples decide only what is decided at once or far from everything
            st3, t3, _, _, _, _, steps3 = sweep.sweep(flat, qpos[e], dofs, q0[e, k], q1[e, k], pairs, distmax=S.DISTMAX_T, margin=margin, max_steps=3)
            seen.add(st3)
            assert steps3 <= 3 and (st3 == st if steps <= 3 else (st3 == sweep.UNDECIDED and steps3 == 3 and t3 < t))
    assert seen == {sweep.FREE, sweep.HIT, sweep.UNDECIDED}


def test_thin_wall_is_hit_where_uniform_samples_read_free():
    flat, dofs, pairs, q0, q1 = W.thin_wall()
    qpos = np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel()
    m32 = clearance._model32(flat)
    uniform = np.linspace(0.0, 1.0, W.THIN_WALL_SAMPLES + 2)      # both ends and the eight between them
    c = dense_clearance(flat, m32, qpos, dofs, q0, q1, pairs, uniform, 1.0)
    assert c.min() >= W.THIN_WALL_FREE_BY, c      # sampling calls this motion free
    st, t, d, tm, pair, ft, steps = sweep.sweep(flat, qpos, dofs, q0, q1, pairs)
    ts = np.linspace(0.0, 1.0, 4001)
    near = ts[dense_clearance(flat, m32, qpos, dofs, q0, q1, pairs, ts, 1.0) <= sweep.DEFAULTS["slack"]]
    print(f"thin wall: HIT at t = {t:.5f} after {steps} samples, dist {d:.2e}; a scan of 4001 samples is within slack on [{near[0]:.5f}, {near[-1]:.5f}]")
    assert st == sweep.HIT and pair == 0 and 0.0 <= d <= sweep.DEFAULTS["slack"]
    assert near[0] - 1 / 4000 <= t <= near[-1]      # inside the crossing: no earlier than the bar's flank can reach the wall's face, no later than its far face
    assert uniform[4] < t < uniform[5]               # ... which lies between two of the samples that read free


def test_refusals_by_name(scene):
    flat, qpos, _ = scene
    dofs = S.dofs_t(flat, "arm")
    q0, q1 = W.segments(flat, dofs, 1, 1)
    for kw, word in ((dict(slack=0.0), "slack"), (dict(margin=-1e-3), "margin"), (dict(max_steps=0), "max_steps"), (dict(max_steps=4097), "max_steps"),
                     (dict(distmax=0.011, margin=0.01), "distmax")):
        with pytest.raises(sweep.SweepError, match=word):
            sweep.sweep(flat, qpos[0], dofs, q0[0, 0], q1[0, 0], **kw)
    # a plane on a moved body: the floor's twin on the first link
    xml = S.SCENE_T_XML.replace('<geom name="g_cap"', '<geom name="g_pl" type="plane" size="1 1 0.1"/><geom name="g_cap"')
    import os, tempfile
    from tests import raycast_scenes as R
    with tempfile.TemporaryDirectory() as tmp:
        R.write_obj(os.path.join(tmp, "poly.obj"), R.POLY_VERTS)
        flat2 = mjcf.compile_mjcf(xml, asset_dir=tmp)
    g = flat2.names["geom"].index
    with pytest.raises(sweep.SweepError, match="plane geom"):
        sweep.motion_bound(flat2, S.scene_t_qpos(flat2, 1)[0], S.dofs_t(flat2, "arm"), q0[0, 0], q1[0, 0], [[g("g_pl"), g("wbox")]])


def test_condition_for_the_gpu_tests(scene):
    """the mirror decides every segment tests/test_sweep.py runs on scene T within max_steps / 2 samples; FREE and HIT both occur in every shape"""
    flat = scene[0]
    dofs = S.dofs_t(flat, "all")
    pairs = clearance.default_pairs(flat, dofs)
    Bm = max(b for b, _ in GPU_SHAPES)
    qpos = S.f32(S.scene_t_qpos(flat, Bm))
    done = {}
    for Bs, Ks in GPU_SHAPES:
        q0, q1 = W.segments(flat, dofs, Bs, Ks)
        seen = set()
        for e in range(Bs):
            for k in range(Ks):
                if (e, k) not in done:      # (segment (env, k) is the same draw in every shape)
                    r = sweep.sweep(flat, qpos[e], dofs, q0[e, k], q1[e, k], pairs, distmax=S.DISTMAX_T)
                    done[e, k] = (r[0], r[6])
                seen.add(done[e, k][0])
        assert seen == {sweep.FREE, sweep.HIT}, (Bs, Ks, seen)
    worst = max(s for _, s in done.values())
    print(f"the mirror's worst step count over {len(done)} segments: {worst}")
    assert worst <= sweep.DEFAULTS["max_steps"] // 2
