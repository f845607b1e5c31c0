/* myo_hip_forward.h -- forward pass of the HIP stepper: body, site and geom frames and the contact list at the batch's current state,
 * without a step (mj_forward's position stage and collision; what sim.data.xpos / site_xpos / geom_xpos / ncon / contact are read from).
 * Includes myo_hip.h; myo_hip.h does not include it.  An extension of libmyo_hip.so only: the float64 oracle's twin of the ABI
 * (oracle/myo_oracle_abi.c) has no counterpart, the float64 side of the check is the oracle's own forward pass (tests/forward_ref.py).
 *
 * myo_forward launches one kernel, one wavefront per env, that runs the step kernel's own state check, kinematics, broad phase and narrow
 * phase -- the same code, with no MPR warm-start entry going in -- on MYO_F_QPOS / MYO_F_QVEL as they are, so the contacts it reports are
 * by construction those of the first substep of the next myo_step.  It honours the per-env overrides the batch carries (MYO_F_BODYPOS,
 * MYO_F_BODYQUAT, MYO_F_GEOMSIZE, MYO_F_HFIELD) and myo_model_set_switch's disable_contact (then ncon = 0).  It writes its own buffers,
 * MYO_F_FLAGS and the env's launch-local contact overflow scratch, and nothing else: no state, no warm start, no diagnostics, no
 * observation or sensor row.  No force-level quantity leaves it.
 *
 * An env whose qpos or qvel is non-finite or larger than 1e10 in magnitude gets MYO_FLAG_BAD_STATE, zeros in all its forward rows and
 * ncon = 0; unlike myo_step, myo_forward does not reset it.  Contacts the narrow phase drops for want of room raise
 * MYO_FLAG_CONTACT_OVERFLOW, as in a step. */
#ifndef MYO_HIP_FORWARD_H
#define MYO_HIP_FORWARD_H

#include "myo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the buffers of a forward pass, float32 unless noted; positions are world coordinates, rotations row-major world-from-local */
enum { MYO_FWD_XPOS = 0,       /* [B][nbody][3] body frame origins */
       MYO_FWD_XMAT = 1,       /* [B][nbody][9] body frame rotations */
       MYO_FWD_XIPOS = 2,      /* [B][nbody][3] body centres of mass */
       MYO_FWD_SITE_XPOS = 3,  /* [B][nsite][3] */
       MYO_FWD_SITE_XMAT = 4,  /* [B][nsite][9]; MYO_E_UNSUPPORTED for a model blob without site_quat (compiled without touch sensors) */
       MYO_FWD_GEOM_XPOS = 5,  /* [B][ngeom][3] every geom of the model, in model numbering */
       MYO_FWD_GEOM_XMAT = 6,  /* [B][ngeom][9] */
       MYO_FWD_NCON = 7,       /* [B] int32 contacts of the env */
       MYO_FWD_CONTACT = 8,    /* [B][ncon_max][16]: dist | pos[3] | frame[9] = normal (geom1 -> geom2), tangent 1, tangent 2 as the constraint
                                  rows use them | geom1, geom2 (model geom ids), pair index (int32).  Records at or beyond the env's ncon are
                                  unspecified; the order of an env's contacts is the kernel's and unspecified */
       MYO_FWD_COUNT = 9 };
#define MYO_FWD_CONTACT_WORDS 16

/* sizes of the buffers: bodies (the world included), sites, geoms, and the contact records per env (the capacity of the model's step kernel:
 * its LDS rows plus its overflow rows).  MYO_E_UNSUPPORTED for a model without a forward pass (below) */
int myo_model_forward_dims(const myo_model*, int* nbody, int* nsite, int* ngeom, int* ncon_max);
/* Asynchronous on `stream`, like myo_step.  The first call allocates the batch's forward buffers; before it nothing is allocated.
 * MYO_E_UNSUPPORTED where myo_step would run the generic lanes kernel: a model the wave-per-env kernel cannot take, or lanes != 64
 * (myo_set_lanes / MYO_LANES) for a model the lanes kernel can take.  myo_model_forward_dims refuses the same */
int myo_forward(myo_batch*, void* stream);
/* device pointer / pitch / width (elements per env) of one buffer; MYO_E_ARG for an unknown `which` and before the first myo_forward */
int myo_forward_buffer(myo_batch*, int which, void** dev_ptr, size_t* pitch, size_t* width);
/* synchronous host copy of one buffer, B * width elements of 4 bytes (plumbing without torch, like myo_batch_read); errors as above, and
 * MYO_E_ARG for a size mismatch */
int myo_forward_read(myo_batch*, int which, void* host, size_t nbytes);
/* The export tables myo_model_load builds for the kernel, from the blob alone (no device needed): table 0 bodies, 1 sites, 2 geoms, each
 * [n][16] float64 = link (< 0: welded to the world) | position[3] | rotation[9] inside the link's frame (world-welded: world pose relative to
 * the blob's hip_origin) | bodies: centre of mass inside the link's frame [3]; sites, geoms: body id, 0, 0.  out == NULL or capacity (in
 * doubles) too small: only *n is set.  For tests and tools */
int myo_forward_host_tables(const void* blob, size_t nbytes, int table, double* out, size_t capacity, int* n);

#ifdef __cplusplus
}
#endif

#endif
