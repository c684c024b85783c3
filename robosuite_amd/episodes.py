"""Host mirror of k_end_episodes (csrc/rsim_episode.hip): which envs end their episode early, and what a restart from the reset ring writes.

The kernel runs behind every control step of a batch with an early-end rule armed (include/rsim.h rsim_set_early_end) and on its own for
rsim_end_episodes; the restart it performs is the one the control step performs at the horizon (rsim_step.hip step_body, RF_EPISODE).  This module
restates both decisions and writes in numpy, as dr.py restates k_randomize: it is the specification the kernel is tested against
(tests/test_early_end_host.py on hand-made arrays, tests/test_early_end.py against the device), and it runs without a GPU.
"""
from __future__ import annotations

import numpy as np

RUNNING, HORIZON, SUCCESS, DIVERGED, REQUESTED = 0, 1, 2, 3, 4     # RSIM_END_REASON
RULE_SUCCESS, RULE_DIVERGED = 1, 2                                  # bits of `rules`
PATCH_TASK_OBJECT = -1                                              # RSIM_PATCH_TASK_OBJECT
MPRC_VALID = 3                                                      # word of a pair's warm-start record that marks it valid


def end_reasons(state, rules: int, mask=None, min_steps: int = 1, standalone: bool = False):
    """int32 [B]: the cause the kernel finds for every env, first match wins.  In a control step: 1 the step itself restarted the env at the horizon
    (never twice), 2 success rule, 3 divergence rule (RSIM_DIVERGED moved since the previous launch), 4 mask.  standalone (rsim_end_episodes): the mask
    alone decides -- done / success are an earlier step's."""
    B = len(state["done"])
    m = np.zeros(B, dtype=bool) if mask is None else np.asarray(mask).reshape(B) != 0
    if standalone:
        return np.where(m, REQUESTED, RUNNING).astype(np.int32)
    r = np.zeros(B, dtype=np.int32)
    r[m] = REQUESTED
    if rules & RULE_DIVERGED:
        r[np.asarray(state["diverged"]) != np.asarray(state["seen_diverged"])] = DIVERGED
    if rules & RULE_SUCCESS:
        r[(np.asarray(state["success"]) != 0) & (np.asarray(state["ep_step"]) >= int(min_steps))] = SUCCESS
    r[np.asarray(state["done"]) == 1] = HORIZON
    return r


def end_episodes_reference(state_dict, bank, rules: int, mask=None, min_steps: int = 1, standalone: bool = False, applied: bool = False):
    """The state k_end_episodes leaves, as a new dict of arrays (the input is not modified).

    state_dict: [B, ...] arrays under the backend's field names -- done, success, ep_step, ep_index, diverged, seen_diverged (the kernel's own record
      of `diverged`), end_reason, bank_stale, needs_reset, obs, terminal_obs, qpos, qvel, qacc_warmstart, ctrl, time; optional: task_object,
      qfrc_applied / xfrc_applied, mprc [B, npair, 12], ft [B, n] (the env's float table, or any array the bank's patch offsets index) and ft_base.
      Arrays that are absent are skipped, as the kernel skips a null pointer.
    bank: dict(rows [B, E, nq + P], tags [B, E], patch_idx [P]) -- the reset ring as the device holds it.
    rules / min_steps: rsim_set_early_end; mask: [B] requested ends or None; standalone: rsim_end_episodes (outside a control step: an env that
      does not end keeps done and end_reason); applied: the applied-force arrays are read by the control step, so a restart zeroes them."""
    s = {k: np.array(v, copy=True) for k, v in state_dict.items()}
    rows, tags, pidx = np.asarray(bank["rows"]), np.asarray(bank["tags"]), np.asarray(bank["patch_idx"], dtype=np.int64).reshape(-1)
    E, nq = rows.shape[1], s["qpos"].shape[1]
    reason = end_reasons(s, rules, mask, min_steps, standalone)
    if not standalone:
        if "seen_diverged" in s:
            s["seen_diverged"][:] = s["diverged"]
        s["end_reason"][:] = reason
    for env in np.nonzero(reason >= SUCCESS)[0]:
        ep = int(s["ep_index"][env]) + 1
        slot = ep % E
        src = rows[env, slot]
        if tags[env, slot] != ep:
            s["bank_stale"][env] += 1
        if "terminal_obs" in s:
            s["terminal_obs"][env] = s["obs"][env]
        s["qpos"][env] = src[:nq]
        for k in ("qvel", "qacc_warmstart", "ctrl", "time"):
            s[k][env] = 0
        for p, pi in enumerate(pidx):
            if pi == PATCH_TASK_OBJECT:
                s["task_object"][env] = int(src[nq + p])
                continue
            s["ft"][env, pi] = src[nq + p]
            if "ft_base" in s:
                s["ft_base"][env, pi] = src[nq + p]
        if "mprc" in s:
            s["mprc"][env, :, MPRC_VALID] = 0
        if applied:
            s["qfrc_applied"][env] = 0
            s["xfrc_applied"][env] = 0
        s["ep_index"][env], s["ep_step"][env], s["done"][env], s["needs_reset"][env] = ep, 0, 1, 1
        if standalone:
            s["end_reason"][env] = REQUESTED
    return s
