"""Host rehearsal of the M^-1 kernel's fp32 core (robosuite_amd/csrc/rsim_dyn_solve_core.h: the in-place Cholesky and the substitutions k_dyn_solve runs per
candidate on its own words of LDS) under AddressSanitizer + UndefinedBehaviorSanitizer: tests/san/dyn_solve_driver.cpp is built with g++ and run as a
subprocess, on blocks of 64 candidates laid out [word][lane] and allocated at exactly the kernel's LDS size.  Pass = the sanitizers report nothing, every
candidate returns, and the program's fp32 results agree with numpy's fp64 solve ON THE SAME fp32 INPUTS within the bound of the solve
(tests/dynamics_solve_scenes.py: Higham's backward error of Cholesky, by reasoning, not from a run).

  * scene D's M, bias and J (the fp64 statement, rounded to fp32) at (5, 13), arm and all dofs, and the 16-hinge chain's 16 x 16 M at (2, 5);
  * the not-positive-definite path, exercised ONLY here, not on the GPU: an indefinite matrix and a NaN matrix among good ones each give ok = 0 and NaN
    outputs, and every other candidate's results are the same bits as without them.
Nothing sanitized is loaded into Python."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests import clearance_scenes as S
from tests import dynamics_scenes as D
from tests import dynamics_solve_scenes as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(ROOT, "tests", "san", "dyn_solve_driver.cpp")
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


def build(out_dir):
    """the driver under both sanitizers -> (path, None) or (None, the compiler's complaint)"""
    out = os.path.join(str(out_dir), "dyn_solve_san")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", DRIVER, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    return (out, None) if r.returncode == 0 else (None, r.stderr or "")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out, err = build(tmp_path_factory.mktemp("dyn_solve_san"))
    if out is None and "asan" in err.lower() and "cannot find" in err:
        pytest.skip("libasan / libubsan not installed")
    assert out is not None, err[-3000:]
    return out


def run(exe, tmp, M, bias, tau, rhs, jacp, jacr):
    """arrays with one leading candidate axis [N, ...] -> dict(ok, qdd, x, minv_jt, lambda_inv)"""
    N, n = bias.shape
    r = rhs.shape[-1]
    f32 = lambda a: np.ascontiguousarray(a, dtype="<f4").tobytes()      # noqa: E731
    blob = struct.pack("<4i", N, n, r, int(tau is not None)) + f32(M) + f32(bias) + (f32(tau) if tau is not None else b"") + f32(rhs) + f32(jacp) + f32(jacr)
    fin, fout = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(fin, "wb") as f:
        f.write(blob)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300, env=ENV)
    assert p.returncode == 0 and not p.stderr.strip(), (p.stdout[-300:], p.stderr[-4000:])       # no sanitizer finding, no crash
    assert f"candidates: {N} of {N}" in p.stdout                                                  # every candidate returned
    raw = open(fout, "rb").read()
    assert len(raw) == 4 * N * (1 + n + n * r + 6 * n + 36)
    ok = np.frombuffer(raw, dtype="<i4", count=N)
    rest = np.frombuffer(raw, dtype="<f4", offset=4 * N)
    qdd, x, mjt, lam = np.split(rest, np.cumsum([N * n, N * n * r, N * n * 6]))
    return dict(ok=ok, qdd=qdd.reshape(N, n), x=x.reshape(N, n, r), minv_jt=mjt.reshape(N, n, 6), lambda_inv=lam.reshape(N, 6, 6))


def f32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def scene_d_inputs(which, B=5, K=13):
    """scene D's fp32-rounded M, bias and J from the fp64 statement, flattened to [B K, ...]"""
    flat = D.scene_d()
    dofs, site = D.dofs_d(flat, which), flat.names["site"].index("f1_s" if which == "all" else "tip")
    qpos = S.f32(D.scene_d_qpos(flat, B)).astype(np.float64)
    q, qd, _ = D.draws(flat, dofs, B, K)
    ref = D.reference(flat, qpos, dofs, q, qd, None, site)
    n = len(dofs)
    return (f32(ref["M"]).reshape(B * K, n, n), f32(ref["tau"]).reshape(B * K, n), V.tau_draw(B, K, n).reshape(B * K, n), V.rhs_draw(B, K, n, 5).reshape(B * K, n, 5),
            f32(ref["jacp"]).reshape(B * K, 3, n), f32(ref["jacr"]).reshape(B * K, 3, n))


def chain_inputs(B=2, K=5):
    flat, dofs = V.chain16()
    qpos = np.tile(np.asarray(flat.arrays["qpos0"], dtype=np.float64).ravel(), (B, 1))
    q, qd, _ = D.draws(flat, dofs, B, K)
    ref = D.reference(flat, qpos, dofs, q, qd, None, int(flat.nsite) - 1)
    return (f32(ref["M"]).reshape(B * K, 16, 16), f32(ref["tau"]).reshape(B * K, 16), V.tau_draw(B, K, 16).reshape(B * K, 16),
            V.rhs_draw(B, K, 16, 16).reshape(B * K, 16, 16), f32(ref["jacp"]).reshape(B * K, 3, 16), f32(ref["jacr"]).reshape(B * K, 3, 16))


def hold(what, got, M, bias, tau, rhs, jacp, jacr):
    """the program's results against numpy's fp64 solve on the same inputs, within the bound of the solve -> {name: (worst relative error, share of the bound)}"""
    rel = V.solve_bound(M)
    assert rel.max() < V.LIMIT, (what, rel.max())      # the condition: a bound that says something
    assert got["ok"].all()
    J = V.J6(jacp, jacr)
    JT = np.swapaxes(J, -1, -2)
    t = np.zeros_like(bias) if tau is None else tau
    fig = {"forward_dynamics": V.hold_columns(f"{what}, host, forward dynamics", V.columns(got["qdd"]), V.columns(V.solve(M, t - bias)), rel),
           "mass_solve": V.hold_columns(f"{what}, host, mass solve", got["x"], V.solve(M, rhs), rel),
           "minv_jt": V.hold_columns(f"{what}, host, M^-1 J^T", got["minv_jt"], V.solve(M, JT), rel)}
    lam_err, lam_bound = np.abs(got["lambda_inv"].astype(np.float64) - J @ V.solve(M, JT)).max(axis=(-2, -1)), V.lambda_bound(M, J)
    print(f"dynamics solve {what}, host, lambda_inv: worst entry error {lam_err.max():.3e}, {(lam_err / lam_bound).max():.3e} of its bound")
    assert (lam_err <= lam_bound).all()
    assert np.array_equal(got["lambda_inv"], np.swapaxes(got["lambda_inv"], -1, -2))      # one product per unordered pair
    fig["lambda_inv"] = (float(lam_err.max()), float((lam_err / lam_bound).max()))
    return fig


@pytest.mark.parametrize("which", ("arm", "all"))
def test_scene_d_under_sanitizers(exe, tmp_path, which):
    args = scene_d_inputs(which)
    hold(f"scene D {which}", run(exe, tmp_path, *args), *args)


def test_sixteen_by_sixteen_under_sanitizers(exe, tmp_path):
    args = chain_inputs()
    hold("16-hinge chain", run(exe, tmp_path, *args), *args)


def test_absent_tau_is_zeros_under_sanitizers(exe, tmp_path):
    M, bias, tau, rhs, jacp, jacr = scene_d_inputs("arm", B=2, K=3)
    got = run(exe, tmp_path, M, bias, None, rhs, jacp, jacr)
    V.hold_columns("scene D arm, host, tau absent", V.columns(got["qdd"]), V.columns(V.solve(M, -bias)), V.solve_bound(M))


def test_not_positive_definite_candidates_are_flagged_and_alone(exe, tmp_path):
    M, bias, tau, rhs, jacp, jacr = (a.copy() for a in scene_d_inputs("all"))
    good = run(exe, tmp_path, M, bias, tau, rhs, jacp, jacr)
    indefinite, nan, late = 7, 40, 64      # two lanes of the first block and the single live lane of the second
    M[indefinite, 2, 2] = -M[indefinite, 2, 2]                      # a negative pivot in the middle of the factorisation
    M[nan] = np.nan
    M[late, 5, 5] = 0.0                                             # a last pivot that is not > 0
    bad = run(exe, tmp_path, M, bias, tau, rhs, jacp, jacr)
    flagged = np.zeros(len(bias), dtype=bool)
    flagged[[indefinite, nan, late]] = True
    assert np.array_equal(bad["ok"] == 0, flagged)
    for k in ("qdd", "x", "minv_jt", "lambda_inv"):
        assert np.isnan(bad[k][flagged]).all(), k                                                  # every output word of a flagged candidate: NaN
        assert np.array_equal(bad[k][~flagged].view(np.uint32), good[k][~flagged].view(np.uint32)), k      # every other candidate: the same bits
