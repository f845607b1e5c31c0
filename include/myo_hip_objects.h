/* myo_hip_objects.h -- per-env object parameters of the HIP stepper: size, position and friction of up to 16 collision geoms and the mass
 * of up to 4 bodies, one value per env, with an optional re-draw at every reset (what myoChallengeBaodingP2-v1 does to its two balls and
 * myoChallengeDieReorientP2-v0 to its die: baoding_v1.py:360-385, reorient_v0.py:221-247).  Includes myo_hip.h; myo_hip.h does not include
 * it, and it adds nothing to the myo_field numbering or to myo_task_config.  An extension of libmyo_hip.so only.
 *
 * Models of the TrackEnv class only (the step kernel that steps key-turn, pen, baoding, die and the MyoDM objects), Euler integrator.
 * Everything else is refused with MYO_E_UNSUPPORTED and a message: other kernel classes, the RK4 twin, mesh / hull, plane and height-field
 * geoms, a geom that is no collision geom of the model (it takes part in no pair the lowering kept), a geom of a body welded to the world,
 * a body that shares its kinematic link with another body, more than MYO_OBJ_MAX_GEOMS geoms or MYO_OBJ_MAX_BODIES bodies.
 *
 * Four tables in device memory, float32, env-major, all starting at the compiled model's values:
 *   MYO_OBJ_SIZE      [B][ng][3]  mjModel.geom_size of the selected geoms
 *   MYO_OBJ_POS       [B][ng][3]  mjModel.geom_pos: in the frame of the geom's body, in the user's coordinates
 *   MYO_OBJ_FRICTION  [B][ng][3]  mjModel.geom_friction (sliding, torsional, rolling)
 *   MYO_OBJ_MASS      [B][nb]     mjModel.body_mass of the selected bodies
 * A value written through the device pointer (or myo_objects_write) takes effect at the next myo_step / myo_forward / myo_bench_rollout:
 * every such launch first composes the rows its kernel reads from the tables (bounding radius, position in the link frame), once per launch
 * and not per substep.  Writes through the pointer are not validated; myo_objects_write is.
 *
 * Semantics, as when the same arrays of a compiled MuJoCo model are edited without mj_setConst (what the reference does):
 *   size      the narrow and broad phase use the env's size; the bounding radius is recomputed from it (sphere r; capsule r + half length;
 *             box |size|; ellipsoid max; cylinder hypot(r, half length)), as MYO_F_GEOMSIZE does.  The pair table is shared by all envs:
 *             which pairs exist, their dof lists and their static pruning are those of the compiled sizes.
 *   pos       the geom's centre in its body; its orientation stays.
 *   friction  the friction of every pair the geom takes part in is mixed again per env by mj_contactParam's rule: geom priorities differ ->
 *             the higher priority's friction, else the component-wise maximum with the partner's friction (the partner's compiled value, or
 *             its own per-env row when it is selected too).  The sliding coefficient and, for condim-4 pairs, the torsional one change;
 *             solref, solimp, margin, gap and the condim of the pair stay.  A mixed coefficient below 1e-5 counts as 1e-5 (MuJoCo's mjMINMU):
 *             a friction of 0 is accepted and does not make the pair frictionless.  The rolling component is stored and not used (no condim 6).
 *   mass      the link's mass is the env's scalar; inertia about the COM, COM, body_invweight0 (hence the contact regularisation),
 *             meaninertia and the actuator constants keep their compiled values, as with MYO_F_BODYMASS.  This is why a selected body must be
 *             the only body of its link: the link's mass is then the body's, and there is nothing to recompose.
 * The MPR warm-start table of the step kernel needs no care: it lives inside one launch (every launch starts with no entry) and an entry is
 * only the starting direction of a pair's next MPR call, so a size written between two launches cannot meet a stale entry.
 *
 * A bad env that the step kernel resets itself keeps its rows: they are model data, not state.  The forward pass shows the same edits
 * (geom_xpos of the selected geoms, the contact list).  The die's visual `target_dice` geom collides with nothing, is no collision geom and
 * is not modelled here. */
#ifndef MYO_HIP_OBJECTS_H
#define MYO_HIP_OBJECTS_H

#include "myo_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MYO_OBJ_MAX_GEOMS 16
#define MYO_OBJ_MAX_BODIES 4
#define MYO_OBJ_MAX_DRAWS 8
enum { MYO_OBJ_SIZE = 0, MYO_OBJ_POS = 1, MYO_OBJ_FRICTION = 2, MYO_OBJ_MASS = 3, MYO_OBJ_COUNT = 4 };

/* Selects the geoms (model geom ids) and bodies (model body ids) and allocates the tables; either list may be empty, not both.  A second call
 * with the same lists is a no-op, with other lists MYO_E_ARG (the selection of a batch is fixed).  Refusals: the header comment */
int myo_objects_enable(myo_batch*, const int* geom_ids, int ngeom, const int* body_ids, int nbody);
/* number of selected geoms / bodies; 0 / 0 before myo_objects_enable */
int myo_objects_count(const myo_batch*, int* ngeom, int* nbody);
/* device pointer / pitch / width (elements per env: 3 * ngeom, or nbody) of one table; MYO_E_ARG while the subsystem is not enabled
 * ("absent") and for a table without entries (MYO_OBJ_MASS with no body selected, the geom tables with no geom) */
int myo_objects_table(myo_batch*, int which, void** dev_ptr, size_t* pitch, size_t* width);
/* synchronous host copy of a table, B * width floats; MYO_E_ARG for a size mismatch */
int myo_objects_read(myo_batch*, int which, void* host, size_t nbytes);
/* synchronous write of a whole table.  Sizes, frictions and masses must be finite and >= 0, positions finite: otherwise MYO_E_ARG and
 * nothing is written */
int myo_objects_write(myo_batch*, int which, const void* host, size_t nbytes);
/* The draw table.  Scalar parameter p of an env's rows, in the order size (3 * ngeom) | pos (3 * ngeom) | friction (3 * ngeom) | mass (nbody),
 * n = 9 * ngeom + nbody in all, becomes base[p] + scale[p] * u at every reset of the env by myo_reset / myo_autoreset (and by the fused
 * epilogue of myo_bench_rollout); scale[p] == 0 leaves the parameter alone (its base is ignored).  draw[p] in [0, ndraw) names one of
 * ndraw <= MYO_OBJ_MAX_DRAWS uniform draws u[k] in [0, 1) shared by every parameter that names it (the die's del_size drives 12 half lengths,
 * 9 box sizes and the geom positions with one draw); draw[p] == -1 gives the parameter a draw of its own.  The draws come from the counter
 * RNG of the reset, keyed by (the reset's seed and the env's episode count, the GLOBAL env id = env + myo_set_env_offset, k or
 * MYO_OBJ_MAX_DRAWS + p): a sharded batch draws what the unsharded one draws.  base + scale * [0, 1) must be finite and, for sizes,
 * frictions and masses, >= 0 at both ends: otherwise MYO_E_ARG.  n == 0 (or NULL arrays) switches the draws off.
 * MYO_E_UNSUPPORTED while the MyoDM track task of the MJX flavour is configured (it resets inside the step kernel; explicit values work) */
int myo_objects_set_draws(myo_batch*, int ndraw, int n, const float* base, const float* scale, const int* draw);

#ifdef __cplusplus
}
#endif

#endif
