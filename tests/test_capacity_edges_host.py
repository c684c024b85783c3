"""The generated capacity-edge models (tests/capacity_models.py) on the host: which compiled configuration serves each, that one dof / body / tree / qpos
entry beyond the largest is refused and not truncated, and that the fp64 oracle stays inside the conditions the GPU tests (tests/test_capacity_edges.py)
rely on.  No GPU; the configuration choice needs the built library."""
import os

import numpy as np
import pytest

from robosuite_amd import backend, mjcf
from tests import capacity_models as cm
from tests.util import make_oracle

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "robosuite_amd", "librsim_hip.so")
pytestmark = pytest.mark.skipif(not os.path.exists(LIB), reason="needs the built library")

CASES = [(n, True) for n in cm.COMPOSITIONS] + [(n, False) for n in cm.TOP_EDGES]


@pytest.mark.parametrize("name,chain_last", CASES)
def test_configuration_is_chosen_by_the_models_size(name, chain_last):
    want, kw, nv, nq, njnt, nbody = cm.COMPOSITIONS[name]
    _, flat = cm.build(name, chain_last)
    assert (flat.nv, flat.nq, len(flat.jnt_type)) == (nv, nq, njnt) and (nbody is None or flat.nbody == nbody)
    hm = backend.HipModel(flat)
    cid, lim = hm.kernel_config()
    assert cid == want, (name, cid)
    assert flat.nbody <= lim["nbody"] and njnt <= lim["njnt"] and nv <= lim["nv"] and nq <= lim["nv"] + 8 and flat.nu <= 16
    assert hm.int("ncgeom") <= lim["ncgeom"] and hm.int("nsite") <= lim["nsite"] and len(flat.arrays["pair_geom1"]) <= lim["npair"]
    assert kw["n_free"] + 1 <= lim["ntree"]
    # the edge the row is named for
    if name.endswith("_top") or "_top_" in name:
        assert nv == lim["nv"]
    if nbody in (32, 64):
        assert nbody == lim["nbody"]
    # the welds sit in the chain: the 64-body models are trees deeper than 32 (a sixth pointer-jumping round of the kinematics), the others are not
    par, depth = np.asarray(flat.arrays["body_parentid"]).ravel(), [0] * flat.nbody
    for b in range(1, flat.nbody):
        depth[b] = depth[int(par[b])] + 1
    assert (max(depth) > 32) == (nbody == 64) and hm.int("nbody") == flat.nbody
    if name.startswith("cfg4_top"):
        assert kw["n_free"] + 1 == lim["ntree"] == 8 and nq > 64


def test_the_dof_ranges_of_the_configurations_meet_without_a_gap():
    """Bottom edge of a configuration = top edge of the one below + 1 dof: 16 | 17 .. 32 | 33 .. 48 | 49 .. 64."""
    nv = {n: cm.COMPOSITIONS[n][2] for n in cm.COMPOSITIONS}
    assert (nv["cfg0_top"], nv["cfg1_bottom"], nv["cfg1_top"], nv["cfg3_bottom"], nv["cfg3_top"], nv["cfg4_bottom"], nv["cfg4_top"]) == (16, 17, 32, 33, 48, 49, 64)


@pytest.mark.parametrize("name", list(cm.REFUSED))
def test_one_beyond_the_largest_configuration_is_refused(name):
    """nv 65, nbody 65, nine articulated trees: rsim_model_create refuses what the 64-bit body / dof masks cannot hold, rsim_model_config answers -1 for the
    rest (rsim_batch_create fails on that answer: the GPU twin asserts it).  nq 73 at nv 64 takes ball joints, which the 64 x 64 build does not carry: there
    the nq limit cannot be reached without them and the model is refused for its ball joints.  The nq limit itself (nq <= nv + 8: `qpos[NV + 8]` in LDS) is held
    on the 32 x 32 build, which carries ball joints: nq 41 at nv 32 fits every other limit of it and is refused, nq 40 (cfg1_nq40) is served."""
    flat = mjcf.compile_mjcf(cm.model_xml(**cm.REFUSED[name]))
    want = {"nv65": dict(nv=65), "nbody65": dict(nbody=65, nv=64), "trees9": dict(nv=58), "nq73": dict(nv=64, nq=73), "nq41": dict(nv=32, nq=41)}[name]
    for k, v in want.items():
        assert getattr(flat, k) == v, (name, k)
    if name in ("nv65", "nbody65"):
        with pytest.raises(backend.RsimError, match="> 64"):
            backend.HipModel(flat)
    else:
        hm = backend.HipModel(flat)
        # everything but the one count fits the largest configuration
        assert flat.nv <= 64 and flat.nbody <= 64 and len(flat.jnt_type) <= 32 and (flat.nq > 72 or cm.REFUSED[name]["n_free"] + 1 > 8 or name == "nq41")
        assert hm.kernel_config()[0] == -1
        if name == "nq41":
            # nq is the one count beyond the build that serves the same chain with one ball joint fewer
            lim = backend.HipModel(cm.build("cfg1_nq40")[1]).kernel_config()[1]
            assert lim["tendons"] & 64 and flat.nq == lim["nv"] + 9 and flat.nv == lim["nv"] and flat.nbody <= lim["nbody"] and len(flat.jnt_type) <= lim["njnt"] and flat.nu <= 16
            assert hm.int("nsite") <= lim["nsite"] and hm.int("ncgeom") <= lim["ncgeom"] and lim["ntree"] >= 1
            one_fewer = dict(cm.REFUSED[name], n_ball=8)
            assert backend.HipModel(mjcf.compile_mjcf(cm.model_xml(**one_fewer))).kernel_config()[0] == 1


@pytest.mark.parametrize("name,chain_last", CASES)
def test_the_oracle_stays_inside_the_conditions_of_the_gpu_tests(name, chain_last):
    """25 and 50 substeps from the seeded start state: finite, moderate velocities, contacts on every free body's side of the scene, limit rows, and
    contact / row counts within the configuration's capacity with room to spare (so that no GPU case is decided by truncation)."""
    want, kw, *_ = cm.COMPOSITIONS[name]
    _, flat = cm.build(name, chain_last)
    lim = backend.HipModel(flat).kernel_config()[1]
    om, od, _ = make_oracle(flat)
    q, v = cm.start_state(flat, 1)
    od.qpos[:] = q; od.qvel[:] = v; od.qacc_warmstart[:] = 0; od.ctrl[:] = 0; od.forward()
    seen_limit, states = False, []
    for k in range(51):
        if k in (0, 25, 50):
            assert np.isfinite(od.qpos).all() and np.isfinite(od.qvel).all() and np.abs(od.qvel).max() < 20.0
            assert kw["n_free"] <= od.ncon <= lim["ncon"] - 4 and od.nefc <= lim["nefc"] - 4, (k, od.ncon, od.nefc)
            seen_limit |= od.nefc > 3 * od.ncon     # elliptic condim-3 contacts carry three rows each: anything beyond is a joint limit
            states.append((od.qpos.copy(), od.qvel.copy()))
        od.step()
    if name in cm.TOP_COUNTS:
        # the counts the GPU cases at the top edges compare on (one forward evaluation of each state, as there)
        got = []
        for sq, sv in states:
            od.qpos[:] = sq; od.qvel[:] = sv; od.qacc_warmstart[:] = 0; od.ctrl[:] = 0; od.forward()
            got.append((od.ncon, od.nefc))
        assert got == cm.TOP_COUNTS[name][0 if chain_last else 1], got
    assert seen_limit or kw["n_hinge"] < 10       # (one limited hinge in the seven of cfg4_bottom, and the draw leaves it free)


def test_the_overflow_pile_has_forty_contacts_each_a_millimetre_deep():
    flat = mjcf.compile_mjcf(cm.overflow_xml())
    hm = backend.HipModel(flat)
    cid, lim = hm.kernel_config()
    assert (flat.nv, cid, lim["ncon"]) == (64, 4, 32)
    om, od, _ = make_oracle(flat)
    od.qpos[:] = flat.qpos0; od.qvel[:] = 0; od.qacc_warmstart[:] = 0; od.ctrl[:] = 0; od.forward()
    assert (od.ncon, od.nefc) == (40, 120)
    assert np.abs(np.array([c["dist"] for c in od.contacts()]) + 1e-3).max() < 1e-12
