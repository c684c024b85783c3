// rsim_dyn.h -- kernel argument of the dynamics query kernels (rsim_dyn.hip), filled by the C-ABI host code (rsim_api.cpp).  Not part of the public boundary.
// Everything the joint walk takes (rsim_grad.h DGrad: the body table, the pose scratch, the joint store, the signature table) plus the model-term offsets, the
// column table, the dynamics scratch and the outputs.
#pragma once
#include "rsim_grad.h"

struct DDyn {
  DGrad g;                       // g.c: the body table, the pose scratch k_clear_fk fills; g.jscr: the joint store k_clear_joints fills; g.sig, g.slide_mask
  const float *qd, *qdd;         // [B][K][n] each, or null: zeros
  float* dscr;                   // [nslot][RSIM_DYN_RNE_WORDS or RSIM_DYN_CRB_WORDS][NC]: the per-body words that outlive a walk's forward half
  const int* cols;               // [n][RSIM_DYN_COL]: dof id and table element of every controlled column
  int fo_mass, fo_inertia, fo_ipos, fo_iquat, fo_armature, fo_damping, fo_opt;   // float-table offsets (rsim_internal.h FO_*)
  float* tau;                    // [B][K][n]
  float* M;                      // [B][K][n][n]
  // the site Jacobian
  int site_body, site_slot, o_site_pos;   // the site's body, its pose-store slot or -1, float-table offset of its site_pos
  unsigned site_sig;             // the body's dof signature
  float *jacp, *jacr;            // [B][K][3][n] each, or null
};

extern "C" int rsim_launch_dyn_rne(const DDyn* a, hipStream_t stream);
extern "C" int rsim_launch_dyn_crb(const DDyn* a, hipStream_t stream);
extern "C" int rsim_launch_dyn_jac(const DDyn* a, hipStream_t stream);
