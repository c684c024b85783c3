"""solve_ik_avoid(signed=True) on the device (csrc/rsim_pen_query.hip k_ika_cost_signed (_att) in front of the unchanged k_ika_step; include/rsim.h
rsim_ik_site_avoid_signed) on the sunk starts of tests/signed_query_scenes.py: 20 envs x 4 starts whose start vector sits 2 to 5 mm inside the scene with the
target already reached.  The reference is the fp64 mirror robosuite_amd/ik_avoid.py (signed=True), never a second device run, except where bits are compared.

  1. ONE UPDATE from every sunk start (max_iters = 1, both tolerances 0): q_out within BOUND["step"] of ik_avoid.update fed with the DEVICE's own signed cost
     gradient at the start -- the step arithmetic, apart from the distance layer.
  2. END TO END: on the cases the mirror is held to (ik_avoid.held_to, signed=True) the device reports converged and finished, and the MIRROR's smallest signed
     distance at the device's q_out is at least d_safe / 2 minus the fp32 distance bound of tests/test_clearance.py; at most CAP of the cases are left out.
  3. THE FEATURE: where the device's unsigned config_collision_cost at the start has nnear == noverlap > 0, the unsigned solve_ik_avoid finishes none and moves
     none by more than 1e-4 rad; the signed call finishes all of them that are held.
  4. BITS: cost / nnear / noverlap equal config_collision_cost(q_out, signed=True) with the same chunks; check_every = 3 returns check_every = 0's bits; with
     avoid_gain = 0 and cost_tol = inf the signed call's q, err, iters are the unsigned call's; a repeat call; rsim_ik_avoid_tables is unchanged."""
import numpy as np
import pytest
import torch

from robosuite_amd import ik_avoid
from tests import clearance_scenes as S
from tests import signed_query_scenes as SQ
from tests import test_clearance as TC
from tests import test_signed_queries as TS
from tests.util import make_hip

pytestmark = pytest.mark.gpu
DIST_BOUND = TC.BOUND["T"]["dist"]
CHUNKS = 3
dev = TC.dev
np_ = TS.np_
_CACHE = {}


def batch():
    if "b" not in _CACHE:
        c = SQ.cases()
        hm, hb = make_hip(c["flat"], None, B=SQ.B)
        hb.set("qpos", c["qpos"].astype(np.float32))
        hb.forward()
        _CACHE["b"] = dict(c=c, hm=hm, hb=hb, pos=dev(c["pos"]), qi=dev(c["q_init"]))
    return _CACHE["b"]


def solve(s, **kw):
    c = s["c"]
    return s["hb"].solve_ik_avoid(c["site"], c["dofs"], s["pos"], None, s["qi"], pairs=c["pairs"], chunks=CHUNKS, **dict(SQ.OPTS, **kw))


def step_figure(s):
    """worst |q_out - ik_avoid.update(g = the device's signed gradient at the start)| per entry after ONE update; asserted: every problem made one"""
    c, hb = s["c"], s["hb"]
    o = dict(SQ.OPTS, max_iters=1, pos_tol=0.0, rot_tol=0.0)
    q, err, it, conv, fin = np_(solve(s, signed=True, **o))[:5]
    assert (it == 1).all() and not fin.any()
    g = hb.config_collision_cost(c["dofs"], s["qi"], pairs=c["pairs"], d_safe=SQ.D_SAFE, chunks=CHUNKS, signed=True)[1].cpu().numpy().astype(np.float64)
    assert (np.abs(g).max(axis=2) > 0).all()      # every sunk start is pushed
    worst = moved = 0.0
    for e in range(SQ.B):
        for k in range(SQ.K):
            q0 = c["q_init"][e, k]
            ref = ik_avoid.update(c["flat"], c["qpos"][e], c["site"], c["dofs"], q0, q0, c["pos"][e, k], None, c["pairs"], g=g[e, k], signed=True, **o)
            worst, moved = max(worst, np.abs(q[e, k] - ref).max()), max(moved, np.abs(ref - q0).max())
    return float(worst), float(moved)


def figures():
    """the MEASURED figure of this file, from one run (tools/signed_queries_parity.py)"""
    return {"step": step_figure(batch())[0]}


def test_one_update_from_every_sunk_start():
    worst, moved = step_figure(batch())
    print(f"signed ik avoid, one update from {SQ.B * SQ.K} sunk starts: worst |q_out - formula| {worst:.3e} rad (bound {TS.bound('step'):.1e}); steps up to {moved:.3f} rad")
    assert worst <= TS.bound("step")


def test_sunk_starts_end_to_end_and_the_feature():
    s = batch()
    c, hb = s["c"], s["hb"]
    flat, dofs, pairs = c["flat"], c["dofs"], c["pairs"]
    held = SQ.held(c)
    assert (~held).sum() <= SQ.CAP * held.size
    plain = solve(s)
    tables = hb.ik_avoid_tables()
    out = solve(s, signed=True)
    assert hb.ik_avoid_tables() == tables      # the same (site, dofs) key: nothing new
    q, err, it, conv, fin, cost, nnear, nover = np_(out)
    params = S.params32(flat)
    at_out = np.array([[SQ.smallest(flat, c["qpos"][e], dofs, q[e, k].astype(np.float64), pairs, params)[0] if held[e, k] else np.nan for k in range(SQ.K)] for e in range(SQ.B)])
    print(f"sunk starts: {int(held.sum())}/{held.size} held, the device finished {int(fin.sum())} ({int(fin[held].sum())} of the held); the mirror's smallest signed distance "
          f"at q_out of the held cases {np.nanmin(at_out):.4f} .. {np.nanmax(at_out):.4f} m (start: {c['depth'].min():.4f} .. {c['depth'].max():.4f}); median iterations "
          f"{np.median(it[held]):.0f}")
    assert conv[held].all() and fin[held].all()
    assert (at_out[held] >= 0.5 * SQ.D_SAFE - DIST_BOUND).all()
    assert (cost[fin] <= ik_avoid.options(**SQ.OPTS)["cost_tol"]).all() and (nover[fin] == 0).all()
    # the feature: the starts at which every near pair of the unsigned cost is a general overlap
    _, ug, un, uo = np_(hb.config_collision_cost(dofs, s["qi"], pairs=pairs, d_safe=SQ.D_SAFE, chunks=CHUNKS))
    stuck = (un == uo) & (uo > 0)
    pq, _, pit, _, pfin = np_(plain)[:5]
    print(f"{int(stuck.sum())} starts with unsigned nnear == noverlap > 0: the unsigned call finishes {int(pfin[stuck].sum())} and moves them by at most "
          f"{np.abs(pq - c['q_init'])[stuck].max():.1e} rad; the signed call finishes {int(fin[stuck].sum())} ({int((stuck & held).sum())} are held)")
    assert stuck.sum() >= held.size // 2 and not ug[stuck].any()
    assert not pfin[stuck].any() and np.abs(pq - c["q_init"])[stuck].max() <= 1e-4
    assert fin[stuck & held].all()


def test_bit_identities():
    s = batch()
    c, hb = s["c"], s["hb"]
    out = solve(s, signed=True)
    again = solve(s, signed=True)
    every3 = solve(s, signed=True, check_every=3)
    for x, y, z in zip(out, again, every3):
        assert torch.equal(x, y) and torch.equal(x, z)
    fin = out[4].cpu().numpy()
    assert 0 < fin.sum()
    cost, _, nnear, nover = hb.config_collision_cost(c["dofs"], out[0], pairs=c["pairs"], d_safe=SQ.D_SAFE, chunks=CHUNKS, signed=True)
    assert torch.equal(cost, out[5]) and torch.equal(nnear, out[6]) and torch.equal(nover, out[7])
    off = dict(avoid_gain=0.0, cost_tol=float("inf"))
    a, b = solve(s, signed=True, **off), solve(s, **off)
    assert all(torch.equal(x, y) for x, y in zip(a[:3], b[:3]))
    assert bool((a[7] >= b[7]).all()) and bool((a[7] > 0).all())      # ... while the counts differ: dist < 0 against status 2
