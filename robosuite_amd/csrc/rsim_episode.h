// rsim_episode.h -- kernel argument of k_end_episodes (rsim_episode.hip), filled by the C-ABI host code (rsim_api.cpp).  Not part of the public boundary.
#pragma once
#define RSIM_MPRC_STRIDE 12   /* floats per candidate pair in DBatch.mprc (rsim_step.hip Sim::MPRC); word 3 of a record is its `valid` flag */

struct DEndEpisodes {
  int env0, nenv;          // this launch covers envs [env0, env0 + nenv) (an env block of a stream group, or the whole batch)
  int nq, nv, nu, nbody, nobs, npair, fstride;
  int bank_E, bank_P;
  int rules, min_steps;    // bit 0: success ends the episode from episode step min_steps on; bit 1: a bad-state guard hit ends it
  int standalone;          // 1: rsim_end_episodes outside a control step -- only the mask decides, `done` / `success` are an earlier step's and are not read,
                           //    and an env that does not end keeps done / end_reason as they are
  int applied;             // zero qfrc_applied / xfrc_applied of a restarted env (the control step reads them: RF_APPLIED, or the debug form)
  const int *success, *diverged;
  const unsigned char* mask;   // [B] or null
  int* seen_diverged;      // [B] RSIM_DIVERGED as of the previous launch (null with standalone)
  int* end_reason;         // [B] RSIM_END_REASON
  int* sel;                // standalone: [B] 1 for the envs this launch restarted, 0 for every other -- the passes that finish the restart take it for needs_reset,
                           //    so that an env the previous control step restarted (its flag still waits for that step's successor) is not visited again
  int *done, *ep_step, *ep_index, *needs_reset, *bank_stale, *task_object;
  const float* bank; const int* bank_tag; const int* patch_idx;
  float *obs, *term_obs, *qpos, *qvel, *qacc_ws, *ctrl, *time, *ft_rw, *ft_base, *mprc, *qfrc_applied, *xfrc_applied;
};

extern "C" int rsim_launch_end_episodes(const DEndEpisodes* a, hipStream_t stream);
