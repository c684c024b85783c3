// rsim_dyn_att.h -- launchers of the dynamics query kernels with carried payloads (rsim_dyn_att.hip), called by the C-ABI host code (rsim_api.cpp).  Not part
// of the public boundary.  The kernel argument is rsim_dyn.h's DDyn, unchanged: its g.c carries natt, held and rel as every attached query's DClear does.  For
// the Jacobian, site_sig holds the site body's whole signature word (not held | held << 16) and site_att, passed beside it, the attachment the body belongs to
// (-1: none).
#pragma once
#include "rsim_dyn.h"

extern "C" int rsim_launch_dyn_rne_att(const DDyn* a, hipStream_t stream);
extern "C" int rsim_launch_dyn_crb_att(const DDyn* a, hipStream_t stream);
extern "C" int rsim_launch_dyn_jac_att(const DDyn* a, int site_att, hipStream_t stream);
