// rsim_episode.hip -- ending episodes early on the device (include/rsim.h rsim_set_early_end / rsim_end_episodes).
//
// The fused control step ends an episode at the horizon, inside k_step (rsim_step.hip step_body, RF_EPISODE).  The other ways an episode ends -- the task
// succeeded, the bad-state guard fired, the caller asked -- are decided here, in a kernel of its own that runs on the batch's stream after every pass of a
// control step has committed and before the k_prepare(reset_only) / k_reset_obs launches that finish ANY restart (constant blocks of the patched float
// tables, reset observation).  It is compiled once, not per kernel configuration, and takes everything it needs as its own kernel argument: the control-step
// code objects (and DModel / DBatch, which are their kernel arguments) are untouched by the feature, so an unarmed batch runs what it always ran.
//
// The restart itself restates the horizon branch of step_body on global memory (that one works on the LDS-resident state and lets the state store that
// follows it write qpos .. time): robosuite_amd/episodes.py is the host mirror both are tested against.
#include <hip/hip_runtime.h>
#include "rsim_episode.h"

// One lane tests one env (coalesced loads of done / success / ep_step / diverged / mask); the wavefront then walks the set of its ending envs with the env
// index in a scalar register and does each env's copies 64 lanes wide, like the in-kernel branch.  Nobody ending -- the common case -- costs the loads and
// one ballot per 64 envs.
__global__ __launch_bounds__(64) void k_end_episodes(DEndEpisodes a) {
  const int lane = threadIdx.x;
  const int base = (int)blockIdx.x * 64;
  const int i = base + lane;
  int reason = 0;
  if (i < a.nenv) {
    const int env = a.env0 + i;
    if (a.standalone) {
      if (a.mask[env]) reason = 4;
      a.sel[env] = reason ? 1 : 0;
    } else {
      const int dv = a.diverged[env];
      if (a.done[env] == 1) reason = 1;                                                               // restarted at the horizon by the control step itself: never twice
      else if ((a.rules & 1) && a.success[env] != 0 && a.ep_step[env] >= a.min_steps) reason = 2;
      else if ((a.rules & 2) && dv != a.seen_diverged[env]) reason = 3;
      else if (a.mask && a.mask[env]) reason = 4;
      a.seen_diverged[env] = dv;
      a.end_reason[env] = reason;
    }
  }
  unsigned long long ending = __ballot(reason >= 2);
  while (ending) {
    const int l = __builtin_ctzll(ending);
    ending &= ending - 1;
    const int env = __builtin_amdgcn_readfirstlane(a.env0 + base + l);
    const int ep = __builtin_amdgcn_readfirstlane(a.ep_index[env] + 1), slot = ep % a.bank_E;
    const float* src = a.bank + ((size_t)env * a.bank_E + slot) * (a.nq + a.bank_P);
    if (lane == 0 && a.bank_tag && a.bank_tag[(size_t)env * a.bank_E + slot] != ep) a.bank_stale[env] += 1;
    if (a.term_obs) for (int k = lane; k < a.nobs; k += 64) a.term_obs[(size_t)env * a.nobs + k] = a.obs[(size_t)env * a.nobs + k];
    for (int k = lane; k < a.nq; k += 64) a.qpos[(size_t)env * a.nq + k] = src[k];
    for (int k = lane; k < a.nv; k += 64) { a.qvel[(size_t)env * a.nv + k] = 0.f; a.qacc_ws[(size_t)env * a.nv + k] = 0.f; }
    for (int k = lane; k < a.nu; k += 64) a.ctrl[(size_t)env * a.nu + k] = 0.f;
    for (int p = lane; p < a.bank_P; p += 64) {
      const int pi = a.patch_idx[p];
      if (pi < 0) { a.task_object[env] = (int)src[a.nq + p]; continue; }   // RSIM_PATCH_TASK_OBJECT
      a.ft_rw[(size_t)env * a.fstride + pi] = src[a.nq + p];
      if (a.ft_base) a.ft_base[(size_t)env * a.fstride + pi] = src[a.nq + p];
    }
    if (a.mprc) for (int p = lane; p < a.npair; p += 64) a.mprc[((size_t)env * a.npair + p) * RSIM_MPRC_STRIDE + 3] = 0.f;   // cold narrow phase, as after a host reset
    if (a.applied) {
      for (int k = lane; k < a.nv; k += 64) a.qfrc_applied[(size_t)env * a.nv + k] = 0.f;
      for (int k = lane; k < a.nbody * 6; k += 64) a.xfrc_applied[(size_t)env * a.nbody * 6 + k] = 0.f;
    }
    if (lane == 0) {
      a.time[env] = 0.f;
      a.ep_index[env] = ep; a.ep_step[env] = 0; a.done[env] = 1; a.needs_reset[env] = 1;
      if (a.standalone) a.end_reason[env] = 4;
    }
  }
}

extern "C" int rsim_launch_end_episodes(const DEndEpisodes* a, hipStream_t stream) {
  if (a->nenv <= 0) return 0;
  hipLaunchKernelGGL(k_end_episodes, dim3((a->nenv + 63) / 64), dim3(64), 0, stream, *a);
  return (int)hipGetLastError();
}
