"""A convex pair that produced a contact leaves "touched" and the contact's depth in its warm-start record (flag 4), and its next visit, if that depth was
over 1e-5 m (Sim::MPR_TOUCH_DEPTH: grazing pairs keep the pretest, see the comment above the pretest block), skips the primitive pretest -- a separating-axis try on the box's or cylinder's best axis: frame algebra and one support pair -- and starts MPR's cold run at once
(rsim_step.hip Sim::convex_convex).  The cold run is the one the pretest-first path falls through to: same v0, same first direction, same loops.  So a
build that writes the flag and does not act on it (-DRSIM_MPR_PRETEST_ALWAYS) must step to the same state BIT FOR BIT.  The bound is equality.

What the two builds may differ in is not in the dumps: the separating direction stored in the substep a contact breaks and near_sep (the dispatch-order key).
The MPR warm record itself (DBatch.mprc) is no field of tools/cand_desc_states.py OUT, so no dumped array is left out.

Each build runs in a child process of its own (one process binds one library: RSIM_LIB)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "robosuite_amd", "csrc")
LIB = os.path.join(ROOT, "robosuite_amd", "librsim_hip.so")
VARIANT = os.path.join(ROOT, "robosuite_amd", "librsim_hip_pretest.so")


def _source_key():
    h = hashlib.sha256()
    for f in ("rsim_step.hip", "rsim_vec.h", "rsim_internal.h", "rsim_api.cpp", "Makefile", os.path.join("..", "..", "include", "rsim.h")):
        h.update(open(os.path.join(CSRC, f), "rb").read())
    return h.hexdigest()


@pytest.fixture(scope="module")
def variant():
    """librsim_hip_pretest.so: configurations 0 (Lift, and the small models) and 1 (Stack) compiled with -DRSIM_MPR_PRETEST_ALWAYS, everything else shared with
    the default build.  Built on first use (two compilations side by side, a few minutes) and kept, keyed to the sources it was built from."""
    key_file = VARIANT + ".key"
    if not (os.path.exists(VARIANT) and os.path.exists(key_file) and open(key_file).read().strip() == _source_key()):
        r = subprocess.run(["bash", os.path.join(ROOT, "tools", "build_variant_flags.sh"), "pretest", "-DRSIM_MPR_PRETEST_ALWAYS", "0", "1"], capture_output=True, text=True, timeout=1800)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        open(key_file, "w").write(_source_key() + "\n")
    return VARIANT


def _states(lib, case, tmp_path):
    out = str(tmp_path / f"{case}_{os.path.basename(lib)}.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "mpr_touch_states.py"), case, out], env=dict(os.environ, RSIM_LIB=lib), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


def _assert_bitwise(a, b):
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def _dumps(a):
    return sorted(int(k[len("ncon_"):]) for k in a.files if k.startswith("ncon_"))


@pytest.mark.gpu
def test_lift_steps_to_the_same_bits_with_the_pretest_before_every_cold_run(variant, tmp_path):
    """Configuration 0, eight envs along the recorded Lift trajectory, six control steps: contacts in every dump (the same pairs touch from one dump to the
    next: fingers and cube on the table), so their visits took the skip."""
    a, b = _states(LIB, "lift", tmp_path), _states(variant, "lift", tmp_path)
    for s in _dumps(a):
        print("lift ncon", s, a[f"ncon_{s}"].tolist())
    assert all((a[f"ncon_{s}"] > 0).all() for s in _dumps(a)) and len(_dumps(a)) == 6
    assert int(a["diverged_5"].sum()) == 0 and all(np.isfinite(a[k]).all() for k in a.files if a[k].dtype.kind == "f")
    _assert_bitwise(a, b)


@pytest.mark.gpu
def test_over_capacity_stack_steps_to_the_same_bits_with_the_pretest_before_every_cold_run(variant, tmp_path):
    """Configuration 1, sixteen Stack envs whose control step outgrows the native body: both bodies of the kernel run their narrow phase; contacts in every
    env at every dump."""
    a, b = _states(LIB, "stack_over", tmp_path), _states(variant, "stack_over", tmp_path)
    for s in _dumps(a):
        print("stack_over ncon", s, a[f"ncon_{s}"].tolist())
    assert all((a[f"ncon_{s}"] > 0).all() for s in _dumps(a)) and len(_dumps(a)) == 3
    assert int(a["diverged_2"].sum()) == 0 and int(a["overflow_2"].sum()) == 0
    _assert_bitwise(a, b)


@pytest.mark.gpu
def test_more_candidates_than_lanes_step_to_the_same_bits_with_the_pretest_before_every_cold_run(variant, tmp_path):
    """About a hundred candidate pairs of spheres, ellipsoids, capsules, cylinders and boxes per substep, few of which touch; candidates beyond the 64 lanes
    carry no record and always take the pretest.  Forty substeps, compared every ten; contacts in every env over the first two dumps (the clusters then drift apart)."""
    a, b = _states(LIB, "crowd", tmp_path), _states(variant, "crowd", tmp_path)
    for s in _dumps(a):
        print("crowd ncon", s, a[f"ncon_{s}"].tolist())
    assert (a["ncon_0"] > 0).all() and (a["ncon_1"] > 0).all() and len(_dumps(a)) == 4
    assert a["mpr_per_env_substep_0"][0] > 0 and all(np.isfinite(a[k]).all() for k in a.files if a[k].dtype.kind == "f")
    _assert_bitwise(a, b)


@pytest.mark.gpu
def test_a_hull_pressed_onto_a_cylinder_and_pulled_off_steps_to_the_same_bits(variant, tmp_path):
    """tools/mpr_touch_states.py press: a 42-vertex hull flies into the side of a cylinder and is pulled off again by a spring, eight envs, forty substeps dumped
    every ten.  Contact at substeps 10 and 20 (the visits in between took the skip), none at 30 and 40: the substep in which the contact breaks is the one in
    which the skipping build leaves through the cold run's own exit and the other through the pretest, and everything after it is downstream of both."""
    a, b = _states(LIB, "press", tmp_path), _states(variant, "press", tmp_path)
    for s in _dumps(a):
        print("press ncon", s, a[f"ncon_{s}"].tolist(), "x", a[f"qpos_{s}"][:, 0].tolist())
    assert _dumps(a) == [0, 1, 2, 3]
    assert (a["ncon_0"] > 0).all() and (a["ncon_1"] > 0).all() and (a["ncon_3"] == 0).all()
    assert all(np.isfinite(a[k]).all() for k in a.files if a[k].dtype.kind == "f")
    _assert_bitwise(a, b)
