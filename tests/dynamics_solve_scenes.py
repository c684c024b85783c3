"""Bounds, draws and fp64 references shared by tests/test_dynamics_solve.py (GPU, the kernel), tests/test_dynamics_solve_core_host.py (CPU, the fp32 core under
sanitizers), tests/test_dynamics_solve_host.py (CPU, the fp64 statement) and tools/dyn_solve_parity.py.  Scenes and candidate draws are
tests/dynamics_scenes.py's, unchanged.

THE BOUND OF THE SOLVE, by reasoning, not from a run.  For one candidate with the fp32 matrix M (n x n) handed to the factorisation and a right-hand side b, the
computed x against x_ref = M^-1 b in exact arithmetic, in the 2-norm per column:

    ||x - x_ref|| <= 2 kappa_2(M) (n (3n + 1) + 2) 2^-24 ||x_ref||

Higham (Accuracy and Stability of Numerical Algorithms, thm 10.4): the computed solution solves (M + dM) x = b with |dM| <= gamma_{3n+1} |R^T| |R|, and
|| |R^T| |R| ||_2 <= n ||M||_2, so ||dM||_2 <= n (3n + 1) u ||M||_2 to first order; forming the right-hand side (tau - bias) is one more rounding, u ||b||,
carried as + 2 u with the first; x - x_ref = -M^-1 (dM x - db) gives kappa_2 times that, and the factor 2 covers the first-order truncation (x for x_ref,
gamma_k for k u).  For lambda_inv = J x, entrywise, n more roundings in the product against ||J||_2 ||x||:

    max |lambda_inv - J x_ref| <= 2 (kappa_2 n (3n + 1) + n + 2) 2^-24 ||J||_2^2 ||M^-1||_2
"""
import numpy as np

from tests import dynamics_scenes as D

EPS32 = D.EPS32
SEED_TAU, SEED_RHS = 613, 614
TAU_MAX = 20.0      # N m (N): the torque draws are uniform in +- this
LIMIT = 5e-3        # every candidate's relative bound must stay below this: a condition on the scenes, asserted from the references alone


def kappa(M):
    return np.linalg.cond(np.asarray(M, dtype=np.float64))


def inv_norm(M):
    """||M^-1||_2 of symmetric positive definite M [..., n, n]"""
    return 1.0 / np.linalg.eigvalsh(np.asarray(M, dtype=np.float64))[..., 0]


def solve_bound(M):
    """the relative bound of the solve per candidate, from M [..., n, n] alone -> [...]"""
    n = M.shape[-1]
    return 2.0 * kappa(M) * (n * (3 * n + 1) + 2) * EPS32


def lambda_bound(M, J):
    """the entrywise bound of lambda_inv per candidate, from M [..., n, n] and J [..., 6, n] alone -> [...]"""
    n = M.shape[-1]
    return 2.0 * (kappa(M) * n * (3 * n + 1) + n + 2) * EPS32 * np.linalg.norm(J, 2, axis=(-2, -1)) ** 2 * inv_norm(M)


def columns(x):
    """[..., n] -> [..., n, 1]: a vector is one column"""
    return np.asarray(x, dtype=np.float64)[..., None]


def col_norm(x):
    """2-norm per column of [..., n, r] -> [..., r]"""
    return np.sqrt((np.asarray(x, dtype=np.float64) ** 2).sum(axis=-2))


def hold_columns(what, x, x_ref, rel, extra=None):
    """assert ||x - x_ref|| <= rel ||x_ref|| (+ extra) per candidate and column; x, x_ref [..., n, r], rel [...], extra [..., r] or None.  Prints and returns
    the worst error relative to ||x_ref|| and the worst share of the allowance used."""
    err, ref = col_norm(np.asarray(x, dtype=np.float64) - x_ref), col_norm(x_ref)
    allow = rel[..., None] * ref + (0.0 if extra is None else extra)
    live = ref > 0
    worst = float((err[live] / ref[live]).max()) if live.any() else 0.0
    share = float((err[allow > 0] / allow[allow > 0]).max()) if (allow > 0).any() else 0.0
    own = f" (the solve's own bound: {float(rel.min()):.1e} .. {float(rel.max()):.1e})" if np.any(rel) else ""
    print(f"dynamics solve {what}: worst error {worst:.3e} of ||x_ref||, {share:.3e} of its bound{own}")
    assert np.isfinite(np.asarray(x)).all(), what
    assert (err <= allow).all(), (what, float((err - allow).max()))
    return worst, share


def J6(jacp, jacr):
    """[..., 3, n] twice -> J [..., 6, n]"""
    return np.concatenate([np.asarray(jacp, dtype=np.float64), np.asarray(jacr, dtype=np.float64)], axis=-2)


def solve(M, b):
    """numpy's fp64 solve, stacked: M [..., n, n], b [..., n, r] or [..., n]"""
    M, b = np.asarray(M, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.linalg.solve(M, b[..., None])[..., 0] if b.ndim == M.ndim - 1 else np.linalg.solve(M, b)


def tau_draw(B, K, n):
    return D.rates(B, K, n, SEED_TAU, TAU_MAX)


def rhs_draw(B, K, n, r):
    """[B, K, n, r] uniform in +-1, fp32-representable"""
    return D.rates(B, K, n * r, SEED_RHS, 1.0).reshape(B, K, n, r)


def chain16():
    from robosuite_amd import mjcf
    from tests import capacity_models
    from tests import clearance_scenes as S

    flat = mjcf.compile_mjcf(capacity_models.model_xml(16, 1))
    return flat, S.dofs_of(flat, [f"h{i}" for i in range(16)])
