/* myo_hip.h -- C ABI of libmyo_hip.so: the MI355X-native batched musculoskeletal stepper.
 *
 * Drop-in boundary for the reference's sim-backend / MJX step path.  Each entry point names
 * the reference interface it replaces (paths relative to /root/reference/myosuite/):
 *
 *   myo_model_load   <- mjx.put_model(mj_model)                 mjx/play.py:10
 *                       DMSimScene._load_simulation             physics/mj_sim_scene.py:28-49
 *   myo_batch_create <- mjx.put_data(m, d) (vmapped Data)        mjx/play.py:11
 *   myo_reset        <- Robot.reset / PoseEnvV0.reset            robot/robot.py:913-998, envs/myo/myobase/pose_v0.py:172-255
 *   myo_set_state /
 *   myo_get_state    <- SimScene.set_state/get_state             physics/sim_scene.py:145-166, envs/env_base.py:643-705
 *   myo_step         <- BaseV0.step -> Robot.step -> sim.advance envs/myo/base_v0.py:83-119, robot/robot.py:844-910,
 *                       -> Physics.step(substeps)                physics/mj_sim_scene.py:51-65 ; jit(mjx.step) mjx/play.py:41,47
 *   myo_obs          <- MujocoEnv.get_obs / get_obs_dict / get_reward_dict / obsdict2obsvec
 *                       envs/env_base.py:392-417, envs/myo/myobase/pose_v0.py:98-138, reach_v0.py:88-144,
 *                       envs/obs_vec_dict.py:86-98
 *   myo_status       <- DMSimScene.advance's exception-and-reset path  physics/mj_sim_scene.py:54-61
 *
 * Conventions: every function returns 0 on success or a negative MYO_E_* code and never throws
 * or aborts; myo_last_error() gives a thread-local message.  All device arrays are env-major
 * float32: element (env e, index i) of a field lives at ptr[e * pitch + i].  Functions taking a
 * `stream` are asynchronous on that hipStream_t (NULL = default stream).  One host thread per
 * myo_batch.  No torch types anywhere in this ABI.
 */
#ifndef MYO_HIP_H
#define MYO_HIP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct myo_model myo_model;
typedef struct myo_batch myo_batch;

enum { MYO_OK = 0, MYO_E_ARG = -1, MYO_E_BLOB = -2, MYO_E_HIP = -3, MYO_E_UNSUPPORTED = -4, MYO_E_NOMEM = -5 };

typedef struct myo_dims {
  /* na = MuJoCo's na: actuators with an activation state (muscles).  Stateless actuators (<motor> etc.) still own a slot of the
   * [B][nu]-wide MYO_F_ACT rows (kept at zero) so that actuator indices address every per-actuator field alike */
  int nq, nv, nu, na, nbody, ntendon, nsite, nlink, obs_dim, env_lds_bytes, lanes_per_env, ncon_max;
  float timestep;
} myo_dims;

/* per-env state / output fields (all float32 unless noted) */
typedef enum myo_field {
  MYO_F_QPOS = 0,    /* [B][nq] */
  MYO_F_QVEL,        /* [B][nv] */
  MYO_F_ACT,         /* [B][nu]  activation per actuator (zero for stateless actuators) */
  MYO_F_CTRL,        /* [B][nu]  last applied control (after the action map) */
  MYO_F_WARMSTART,   /* [B][nv]  qacc_warmstart */
  MYO_F_TIME,        /* [B][1] */
  MYO_F_TARGET,      /* [B][ntarget] pose: target joint vector; reach: target tip positions */
  MYO_F_OBS,         /* [B][obs_dim] */
  MYO_F_REWARD,      /* [B][1] dense reward */
  MYO_F_DONE,        /* [B][1] 1.0f if done */
  MYO_F_SOLVED,      /* [B][1] 1.0f if solved */
  MYO_F_FLAGS,       /* [B][1] int32 bit flags, see MYO_FLAG_* */
  MYO_F_DIAG,        /* [B][8] int32 diagnostics: nefc, ncon, solver_iter(max over substeps), ncon_dropped, ... */
  MYO_F_QACC,        /* [B][nv]  qacc of the last substep (diagnostic / parity) */
  MYO_F_TENLEN,      /* [B][nu]  actuator (tendon) lengths of the last substep */
  MYO_F_ACTFORCE,    /* [B][nu]  actuator forces of the last substep */
  MYO_F_SITEXPOS,    /* [B][3*ntip] tip site world positions after the step (reach task) */
  MYO_F_ELAPSED,     /* [B][1] int32 env steps since the last reset (gym TimeLimit counter) */
  MYO_F_ACTION,      /* [B][nu]  library-owned action buffer: write normalised actions here and pass its pointer to myo_step */
  MYO_F_FATIGUE,     /* [B][3*nu] fatigue compartments MA | MR | MF (muscle condition "fatigue") */
  MYO_F_HFIELD,      /* [B][nrow*ncol] height-field elevation per env (terrain models: mjModel.hfield_data, rewritten per episode by
                        TerrainEnvV0.reset, walk_v0.py:563-622); absent (MYO_E_ARG) for models without a colliding height field */
  MYO_F_GEOMSIZE,    /* [B][4] per-env size (3) + bounding radius of the geom named in myo_batch_set_geom_override (absent otherwise) */
  MYO_F_LINKX,       /* [B][12*nlink] world frame (pos 3 + rotation 9, row-major) of every kinematic link as the LAST substep's position stage
                        computed it, i.e. at the state before that substep's integration: what an MJX pipeline_state holds in xpos / xmat
                        after mjx.step (forward, then integrate; mjx/myodm_v0.py:201-232 reads it).  Models of the TrackEnv class only */
  MYO_F_METRICS,     /* [B][4] reward terms of the track task: pose, object, bonus, penalty (mjx/myodm_v0.py:243-262 `rwd_dict`) */
  MYO_F_BODYMASS,    /* [B][nbody] mass of every body in every env (mjModel.body_mass, compiled-model body numbering): the per-env
                        `model.body_mass[bid] = ...` of PoseEnvV0.reset (envs/myo/myobase/pose_v0.py:163-176, weight_bodyname / weight_range).
                        The per-env body-mass override starts the first time this field or MYO_F_BODYMASS_RANGE is written (myo_batch_write)
                        or its device pointer is handed out (myo_batch_field): both buffers are allocated, the masses filled with the model's
                        body_mass, the ranges with zeros.  Before that, myo_batch_read returns the model's masses and starts nothing.
                        The step uses the masses as they are at the launch (a device-side write takes effect at the next myo_step); the
                        link mass / COM / inertia of every link are recomposed from them once per launch.  As with mjModel.body_mass edited
                        at run time without mj_setConst, nothing else changes: body_inertia, acc0, the invweights (constraint impedance)
                        and muscle lengthrange keep their compiled values.  Bodies welded to the world have no dynamic effect: their entries
                        are accepted and ignored.  A host write with a negative mass returns MYO_E_ARG; device-side writes are the caller's
                        responsibility.  Refused (MYO_E_UNSUPPORTED) for RK4 models, TrackEnv-class models, height-field models, the lanes
                        kernel (myo_set_lanes != 64) and batches configured for MYO_TASK_WALK / STAND / TRACK (their observations and
                        rewards use model-wide mass totals).  Hand / leg models that start it step on the run-time-sizes kernel of their class */
  MYO_F_BODYMASS_RANGE, /* [B][2*nbody] per-env mass range: a `lo` block (nbody) then a `hi` block (nbody).  At every reset of an env
                        (myo_reset, myo_autoreset) each body with hi > lo gets mass = lo + (hi - lo) u, u ~ U(0,1) from the counter RNG
                        keyed by (episode seed, global env id, body); bodies with lo == hi keep their mass.  Starts the override like
                        MYO_F_BODYMASS; a host write with lo < 0 or hi < lo returns MYO_E_ARG */
  MYO_F_COUNT
} myo_field;

/* further per-env fields (ids continue after MYO_F_COUNT, the size of the myo_field list above; myo_batch_field / read / write take them
 * like any field) */
enum {
  MYO_F_BODYPOS = MYO_F_COUNT, /* [B][3] per-env translation of ONE body: the body that carries the model's last joint, which must be a child of the
                        world heading a kinematic root link (myohand_keyturn: the key) -- KeyTurnEnvV0.reset's `model.body_pos[-1] = ...`
                        (envs/myo/myobase/key_turn_v0.py:157-169) as an offset from the compiled body_pos.  Starts like MYO_F_BODYMASS: on the
                        first write of this field or MYO_F_BODYPOS_RANGE, or the first request for either device pointer (both buffers
                        zero-filled); before that myo_batch_read returns zeros and starts nothing.  The step and the key-turn observation use
                        the offsets as they are at the launch.  Nothing else changes (the body's inertia, acc0, invweights keep their compiled
                        values, as without mj_setConst).  Refused (MYO_E_UNSUPPORTED) for models outside the TrackEnv class and when that
                        body is not a root body; a host write with a non-finite value returns MYO_E_ARG */
  MYO_F_BODYPOS_RANGE,   /* [B][6] per-env offset range: lo (3) then hi (3).  At every reset of an env (myo_reset, myo_autoreset) each
                        component with hi > lo gets offset = lo + (hi - lo) u, u ~ U(0,1) from the counter RNG keyed by (episode seed, global
                        env id, component); components with lo == hi keep their offset.  Starts the offset like MYO_F_BODYPOS; a host write with
                        hi < lo or a non-finite value returns MYO_E_ARG */
};

enum { MYO_FLAG_BAD_STATE = 1, MYO_FLAG_BAD_QACC = 2, MYO_FLAG_CONTACT_OVERFLOW = 4, MYO_FLAG_CAND_OVERFLOW = 8,
       MYO_FLAG_SCHED_TIMEOUT = 16 /* opt-in substep scheduler gave up waiting (raised on env 0); the step is incomplete */ };
/* A bad env (mj_checkPos / mj_checkVel / mj_checkAcc and DMSimScene.advance's reset, physics/mj_sim_scene.py:54-61).  An env is bad when, at
 * the start of a substep, an entry of its qpos or qvel is non-finite or larger than 1e10 in magnitude (MYO_FLAG_BAD_STATE), or when that
 * substep's qacc is (MYO_FLAG_BAD_QACC).  myo_step resets it like mj_resetData at that substep and runs no further substep of it in that
 * launch; the other envs of the launch are untouched, bit for bit.  After the launch, for a bad env:
 *   MYO_F_QPOS = qpos0; MYO_F_QVEL, ACT, CTRL, WARMSTART, QACC and TIME are exactly zero; the flag bit is set (until myo_status clears it);
 *   MYO_F_TENLEN, ACTFORCE, LINKX, SENSORDATA and CFRC are zeros; MYO_F_ELAPSED counts on (sim.reset() does not end the gym episode).
 * One deliberate exception to "a NaN in is a bad env": under MYO_ACTMAP_SIGMOID_FATIGUE the fatigue model's clip (np.clip in
 * envs/myo/fatigue.py, which would keep the NaN in MA / MR / MF for good) is fminf / fmaxf here, so a NaN action drives the muscle with the
 * clip's lower bound, the compartments stay finite and the env is not flagged: mj_resetData does not touch the compartments, so a NaN
 * there would outlive every reset of the env.
 * Every float field myo_batch_read returns is finite for every env.  None of this depends on the kernel that ran: lanes, size
 * specialisation, integrator, substep scheduler, placement.
 * Tasks.  Where the observation is a pass of its own (myo_obs, or the one-launch epilogue of myo_bench_rollout), MYO_F_OBS / REWARD / DONE /
 * SOLVED / SITEXPOS and the reward-term row of a bad env are those of the reset state.  The walk / stand pass fused into myo_step writes what
 * myo_obs would write right after the launch.  The fused TrackEnv step (MYO_TASK_TRACK with MYO_ACTMAP_CTRLRANGE), whose MJX reference has no
 * error path, ends the episode of a bad env, with or without `autoreset`: MYO_F_DONE = 1, REWARD = 0, METRICS = 0, SOLVED = 0, the state of
 * TrackEnv.reset (init_qpos; zero velocity, activation, control, warm start and time), MYO_F_ELAPSED = 0, MYO_F_OBS = [init_qpos, 0]. */

/* per-env orientation of one world-welded body (ids continue after MYO_F_BODYPOS_RANGE) */
enum {
  MYO_F_BODYQUAT = MYO_F_BODYPOS_RANGE + 1, /* [B][4] absolute body_quat (w x y z) of the body selected by myo_task_config.quat_body (a jointless
                        child of the world, myohand_pen: the target) -- PenTwirlRandomEnvV0.reset's `model.body_quat[target] = euler2quat(...)`
                        (envs/myo/myobase/pen_v0.py:173-184).  Its static collision geoms and sites turn about the body origin: x = p_b +
                        R(q) R(q0)^T (x0 - p_b).  Starts like MYO_F_BODYPOS: on the first write of this field or MYO_F_BODYQUAT_RANGE, or the
                        first request for either device pointer (filled with the compiled quaternion, empty ranges); before that
                        myo_batch_read returns the compiled quaternion and starts nothing.  The body is selected through
                        myo_task_config.quat_body; without a selected body: MYO_E_ARG.  A host write
                        with a non-finite value or a quaternion whose norm is not 1 (to 1e-4) returns MYO_E_ARG */
  MYO_F_BODYQUAT_RANGE,  /* [B][6] per-env Euler range: lo (3) then hi (3).  At every reset of an env with hi > lo in some component, the
                        angles e_k = lo_k + (hi_k - lo_k) u_k, u ~ U(0,1) from the counter RNG keyed by (episode seed, global env id,
                        component), give body_quat = euler2quat(e) (the reference's utils/quat_math.py:77-93); ranges with lo == hi in all
                        components keep the quaternion.  Starts like MYO_F_BODYQUAT; a host write with hi < lo or a non-finite value
                        returns MYO_E_ARG */
};

/* touch sensors and contact forces (ids continue after MYO_F_BODYQUAT_RANGE); both read-only (a host write returns MYO_E_ARG) and absent
 * (MYO_E_ARG) until myo_batch_enable_sensors.  Values are those of d.sensordata after mj_step: the forces of the last substep's solve of the
 * last myo_step, at that substep's pre-integration state; zeros for an env that launch reset (bad state) or that myo_reset / myo_autoreset
 * reset since */
enum {
  MYO_F_SENSORDATA = 30, /* [B][nsensor] touch sensors, in the model's sensor order: summed normal force of the contacts the sensor counts
                            (mj_computeSensor's rule: a geom on the site's body, positive normal force, the ray from the contact point along
                            the normal -- reversed when the site's body is geom 2's -- meets the site's box / sphere) */
  MYO_F_CFRC             /* [B][(nsensor + 1) * 3] world force those contacts put on the model (contacts between two moving geoms are internal
                            and add nothing), then one row with the force of ALL contacts against world-fixed geoms: the ground reaction force */
};


/* action -> control map applied inside myo_step (base_v0.py:87-91) */
enum {
  MYO_ACTMAP_NONE = 0,
  MYO_ACTMAP_MUSCLE_SIGMOID = 1,
  MYO_ACTMAP_SIGMOID_FATIGUE = 2,          /* + muscle condition "fatigue": 3CC-r model, envs/myo/fatigue.py:61-108, base_v0.py:100-104 */
  MYO_ACTMAP_SIGMOID_REAFFERENTATION = 3,  /* + EIP -> EPL tendon transfer, base_v0.py:105-109 (ids set with myo_batch_set_condition) */
  MYO_ACTMAP_CTRLRANGE = 4                 /* TrackEnv.step, mjx/myodm_v0.py:272-275: ctrl = (a + 1) (hi - lo) / 2 + lo over actuator_ctrlrange; with
                                              MYO_TASK_TRACK configured this map also switches the task's fused prologue / epilogue on */
};

/* tasks understood by myo_obs / myo_reset */
typedef enum myo_task { MYO_TASK_NONE = 0, MYO_TASK_POSE = 1, MYO_TASK_REACH = 2, MYO_TASK_WALK = 3,
                        MYO_TASK_STAND = 5, /* walk_v0.py:13-183 ReachEnvV0 (myoLegStandRandom-v0): reach with a site of the free root link; obs = qpos, qvel*dt,
                                               tip (3), target - tip (3), act; reward 10 - d - 10 |qvel dt| + bonus - 100 |act|/na - penalty */
                        MYO_TASK_TRACK = 6, /* MyoDM TrackEnv (mjx/myodm_v0.py:14-304): see myo_track_config */
                        MYO_TASK_KEYTURN = 7, /* KeyTurnEnvV0 (envs/myo/myobase/key_turn_v0.py), models of the TrackEnv class whose last
                                                 joint is the one hinge of a root body (the key).  ntip = 3 sites: key head, index tip, thumb
                                                 tip.  obs = hand qpos, hand qvel*dt, key qpos, key qvel*dt, head - index tip (3), head -
                                                 thumb tip (3), act, with the site positions of the post-step state (also MYO_F_SITEXPOS).
                                                 d_k = | |head - tip_k| - near_th |; reward = w_pose key_q - w_reach (d_IF + d_TH) - w_act_reg
                                                 |act|/na + w_bonus ([key_q > pi/2] + [key_q > pi]) - w_penalty ([d_IF > far_th/2] + [d_TH >
                                                 far_th/2]); solved = key_q > pose_thd (goal_th); done = d_IF > far_th or d_TH > far_th.
                                                 ntarget = 0; the reset draws the key angle through reset_noise / reset_clip */
                        MYO_TASK_PEN = 8, /* PenTwirl{Fixed,Random}EnvV0 (envs/myo/myobase/pen_v0.py), models of the TrackEnv class whose
                                             last six joints are the free-standing pen (3 slides + 3 hinges of one root body).  ntip = 5
                                             sites: object top, object bottom, target top, target bottom, eps_ball; tip_lpos = the object
                                             body's origin in its link frame.  obs = hand qpos (nq - 6), object position (3), object
                                             qvel*dt (6), obj_rot (3), obj_des_rot (3), object position - eps_ball (3), obj_rot - obj_des_rot
                                             (3), act, with the site positions of the post-step state (also MYO_F_SITEXPOS, 15 floats);
                                             rot = (top - bottom) / length.  pos_align = |obj_err_pos|, rot_align = cosine; reward = -w_pose
                                             pos_align + w_reach rot_align - w_act_reg |act|/na - w_penalty [pos_align > far_th] + w_bonus
                                             ([rot_align > 0.9] + 5 [rot_align > 0.95]) [pos_align < far_th]; done = pos_align > far_th;
                                             solved = rot_align > pose_thd and not done.  ntarget = 0 */
                        MYO_TASK_BAODING = 9, /* BaodingEnvV1 (envs/myo/myochallenge/baoding_v1.py), models of the TrackEnv class whose
                                                 last two joints are free joints of root bodies (the balls; nq = nv + 2).  ntip = 4 sites:
                                                 ball1, ball2, target1, target2 (both targets on one body).  ntarget = 5: the per-env goal
                                                 row of MYO_F_TARGET = start angle, direction sign (0 hold, -1 CW, +1 CCW), x radius, y radius,
                                                 period; drawn at every reset as U(target_lo, target_hi) (target_generate = 1), the sign
                                                 rounded down to an integer.  After env step k the targets sit at angle theta = sign 2 pi
                                                 (k - 1) dt / period + start (ball 2: theta - pi) on the ellipse (x_r cos, y_r sin) + (-0.0125,
                                                 -0.07) in their body's frame, the compiled z kept; after a reset, at k = 1.  obs = hand qpos
                                                 (nq - 14), ball1 position, ball1 linear qvel*dt, ball2 position, ball2 linear qvel*dt, target1,
                                                 target2, target1 - ball1, target2 - ball2 (no act); MYO_F_SITEXPOS: the four sites (12
                                                 floats).  reward = -w_pose d1 - w_reach d2; done = a ball site below far_th (drop_th);
                                                 solved = d1 < pose_thd and d2 < pose_thd (proximity_th) and not done */
                        MYO_TASK_DIE = 10, /* ReorientEnvV0 (envs/myo/myochallenge/reorient_v0.py; myoChallengeDieReorient{Demo,P1}-v0), models
                                              of the TrackEnv class whose last six joints are the die (3 slides + 3 hinges of one root body, a
                                              child of the world).  ntip = 8 sites: object_o, object_x, object_y, object_z, target_o, target_x,
                                              target_y, target_z (origin and axis points of the two frames; column k of a frame = (x_k - x_o) /
                                              |lpos_k - lpos_o|); quat_body = the target body, which carries the four target sites and no
                                              colliding geom.  ntarget = 3: the per-env row of MYO_F_TARGET is the goal offset, the target's
                                              position minus its compiled one, drawn at every reset as U(target_lo, target_hi) (target_generate
                                              = 1; goal_pos on all three components); MYO_F_BODYQUAT_RANGE = goal_rot on all three Euler
                                              angles draws the target's orientation.  goal_obj_offset = target_o - object_o at qpos0, a model
                                              constant worked out at configure time.  obs = qpos[:nq - 7] (the reference's off-by-one is kept),
                                              qvel[:nv - 6] * dt, obj_pos (3), goal_pos (3), pos_err = goal_pos - obj_pos - goal_obj_offset (3),
                                              obj_rot = mat2euler(object frame) (3), goal_rot = mat2euler(target frame) (3), rot_err = goal_rot
                                              - obj_rot (3) (no act; mat2euler: utils/quat_math.py:96-115), with the site positions of the
                                              post-step state (also MYO_F_SITEXPOS, 24 floats).  pos_dist = |pos_err|, rot_dist = |rot_err|,
                                              drop = pos_dist > far_th (drop_th); reward = -w_pose pos_dist - w_reach rot_dist + w_bonus
                                              ([pos_dist < 2 near_th] + [pos_dist < near_th]) - w_act_reg |act|/na - w_penalty drop; done =
                                              drop; solved = pos_dist < near_th (pos_th; +inf allowed) and rot_dist < pose_thd (rot_th) and not
                                              drop.  The reset puts envs at init_qpos with zero velocity */
                        MYO_TASK_HOLD = 4 /* ObjHoldFixedEnvV0 (envs/myo/myobase/obj_hold_v0.py:13-118): the model's LAST joint is the free
                                             object; obs = hand qpos, hand qvel*dt, object position, goal - object, act; target = goal (3) */
} myo_task;

typedef struct myo_task_config {
  int task;              /* myo_task */
  int frame_skip;        /* substeps per env step; obs scales qvel by frame_skip*timestep */
  int reset_random;      /* pose: 1 = qpos ~ U(jnt_range) (reset_type "random"), 0 = init_qpos */
  int target_generate;   /* 1 = sample target ~ U(target_lo, target_hi) on reset, 0 = fixed (target_lo) */
  int ntarget;           /* pose: nq; reach: 3*ntip; hold: 3 */
  int ntip;              /* reach: number of tip sites */
  int tip_site[8];       /* reach: site ids (compiled-model numbering) */
  float pose_thd, far_th, near_th;   /* hold: near_th = goal threshold (0.010), far_th = drop distance (0.300) */
  float w_pose, w_bonus, w_act_reg, w_penalty, w_reach;   /* hold: w_reach weighs goal_dist */
  const float* target_lo; /* host pointers, ntarget floats each (copied) */
  const float* target_hi;
  const float* init_qpos; /* host pointer, nq floats (copied); NULL = qpos0 */
  /* optional reset noise (walk_v0.py:152-167 generate_qpos): qpos = clip(init_qpos + U(noise_lo, noise_hi), clip_lo, clip_hi) per qpos
   * entry; host pointers, nq floats each (copied), all four or none (NULL) */
  const float *reset_noise_lo, *reset_noise_hi, *reset_clip_lo, *reset_clip_hi;
  const float* init_qvel; /* host pointer, nv floats (copied) or NULL = zero */
  float tip_lpos[3];      /* stand: the tip site's position in the root link's frame; pen: the object body's origin in its link frame
                             (die: unused, the library works goal_obj_offset out itself) */
  int quat_body;          /* > 0: selects the body of MYO_F_BODYQUAT / MYO_F_BODYQUAT_RANGE (compiled-model body id; 0: no selection, an
                             earlier one stays).  A batch selects one body once.  MYO_E_UNSUPPORTED for models outside the TrackEnv class
                             and for a body with joints or whose parent is not the world */
} myo_task_config;

/* walk task (WalkEnvV0: envs/myo/myobase/walk_v0.py:187-470, registered as myoLegWalk-v0 in envs/myo/myobase/__init__.py:443-459).
 * Observation = qpos[2:], qvel*dt, com_vel(2), torso xquat(4), feet heights(2), COM height, feet - pelvis(6), phase, muscle
 * length / clipped velocity / clipped force/1000 (nu each), act (nu).  With this task configured, myo_step itself produces
 * MYO_F_OBS / REWARD / DONE / SOLVED at the post-step state (one fused pass); myo_obs recomputes them without stepping. */
typedef struct myo_walk_config {
  int frame_skip, hip_period;
  float min_height, max_rot, target_x_vel, target_y_vel;
  float target_rot[4];                                         /* reference root quaternion (walk_v0.py:425-431) */
  int body_talus_l, body_talus_r, body_pelvis, body_torso;     /* compiled-model body ids */
  int qadr_hip_flexion_l, qadr_hip_flexion_r;                  /* qpos addresses (walk_v0.py:413-420) */
  int qadr_joint_angle[4];                                     /* hip_adduction_l, hip_adduction_r, hip_rotation_l, hip_rotation_r */
  float w_vel_reward, w_done, w_cyclic_hip, w_ref_rot, w_joint_angle_rew;
  const float* init_qpos;                                      /* host, nq floats: reset pose (reset_type "init": key_qpos[2]) */
  const float* init_qvel;                                      /* host, nv floats or NULL (zero) */
  /* TerrainEnvV0 (walk_v0.py:490-671, myoLeg{Rough,Hilly,Stair}TerrainWalk-v0), terrain models only; all zero for WalkEnvV0 */
  float knee_height;                                           /* > 0: also done when COM height - mean feet height < this (0.61, :660-671) */
  int terrain;                                                 /* myo_terrain: elevation grid re-drawn at every reset of an env (:563-622) */
  float terrain_scalar_lo, terrain_scalar_hi;                  /* hilly / stairs height scale ~ U(lo, hi); variant "fixed": lo == hi */
  /* reset_type "random" (WalkEnvV0.get_randomized_initial_state, walk_v0.py:316-332): with probability 1/2 the alternative keyframe
   * (init = key 2, alt = key 3), then qpos += N(0, reset_noise_std) on every coordinate except the root height and quaternion */
  const float* init_qpos_alt;                                  /* host, nq floats or NULL (reset_type "init") */
  const float* init_qvel_alt;                                  /* host, nv floats or NULL */
  float reset_noise_std;                                       /* 0.02 in the reference */
} myo_walk_config;
/* MyoDM TrackEnv (mjx/myodm_v0.py:14-304; the env the reference runs on MJX), models of the TrackEnv class (myohand_object_*).  With this
 * task configured, ONE myo_step(action, MYO_ACTMAP_CTRLRANGE, n_frames) is a whole env step:
 *   ctrl = (action + 1) (hi - lo) / 2 + lo (:272-275); reference row looked up at the pre-step time + motion_start_time (:278-279,
 *   mjx/reference_motion.py:7-313 == logger/reference_motion.py, its arithmetic kept: see `interpolation_linear`); n_frames substeps;
 *   MYO_F_OBS = [qpos, qvel] (:297-304); MYO_F_REWARD / DONE / METRICS = compute_reward on the stepped state with the body frames of the last
 *   substep's position stage (:185-267); with `autoreset`, envs that are done go back to init_qpos / zero velocity, activation, time and
 *   their observation row is the first one of the new episode.
 * myo_reset puts envs at init_qpos (TrackEnv.reset :152-173); myo_obs writes [qpos, qvel] without stepping. */
typedef struct myo_track_config {
  int n_frames;                            /* physics substeps per env step (5, :41-46) */
  int ref_type;                            /* 0 FIXED (1 row), 1 RANDOM (2 rows: low / high), 2 TRACK (> 2 rows) (reference_motion.py:64-75) */
  int horizon, robot_horizon, object_horizon, robot_dim, object_dim;
  int motion_extrapolation;                /* hold the last frame beyond the motion's end */
  int interpolation_linear;                /* 0: the reference's between-frame arithmetic, (1 - b) ** x[i] + b x[i+1] with b = t - T[i] / dt; 1: linear */
  double motion_start_time;
  const double *ref_time, *ref_robot, *ref_robot_vel /* or NULL */, *ref_object;   /* host; [horizon], [robot_horizon][robot_dim] x2, [object_horizon][object_dim] */
  const float* init_qpos;                  /* host, nq */
  const float *ctrl_lo, *ctrl_hi;          /* host, nu: actuator_ctrlrange */
  int object_link, wrist_link;             /* kinematic links carrying the object body and the wrist (lunate) body */
  float object_ipos[3], object_imat[9], wrist_ipos[3];   /* the bodies' inertial frames (xipos / ximat) inside those links */
  float lift_z;                            /* object height that earns the lift bonus (:137-139) */
  float obj_err_scale, base_err_scale, lift_bonus_mag, qpos_reward_weight, qpos_err_scale, qvel_reward_weight, qvel_err_scale;   /* :104-128 */
  float obj_fail_thresh, base_fail_thresh, qpos_fail_thresh;
  int terminate_obj_fail, terminate_pose_fail;
  float w_pose, w_object, w_bonus, w_penalty;   /* DEFAULT_RWD_KEYS_AND_WEIGHTS :16-21 */
  int autoreset;
  int max_episode_steps;                   /* gym TimeLimit of the registered MyoDM ids (envs/myo/myodm/__init__.py:571,649; 0: none): MYO_F_SOLVED = 1 when the
                                              episode is truncated by it (and not done); with `autoreset` such envs are reset as well */
  uint64_t seed;                           /* RANDOM references: draws keyed by (seed, global env id, env step) */
  int flavour;                             /* 0: the MJX TrackEnv above (default).  1: the classic gym TrackEnv (envs/myo/myodm/myodm_v0.py), the
                                              entry point of the registered MyoDM ids: an env step is myo_step(action, MYO_ACTMAP_MUSCLE_SIGMOID,
                                              n_frames = 10) then myo_obs (MYO_ACTMAP_CTRLRANGE is refused with MYO_E_ARG).  myo_obs /
                                              myo_obs_reset_only write qpos, qvel, hand_qpos_err, hand_qvel_err (robot_dim entries, or one 0
                                              without ref_robot_vel), obj_com_err (3), act (na) -- nq + nv + 2 robot_dim + 3 + na floats, or
                                              nq + nv + robot_dim + 4 + na -- with the reference looked up at t = elapsed * n_frames * timestep +
                                              motion_start_time (t = 0 after a reset) and the body frames of the post-step qpos (:189-251);
                                              MYO_F_REWARD / DONE / METRICS from get_reward_dict (:253-311: object = exp(-obj_err_scale (com_err
                                              + 0.1 rot_err)) + exp(-base_err_scale base_err)); MYO_F_SOLVED = 0.  myo_reset / myo_autoreset put
                                              envs at init_qpos.  RANDOM references draw a fresh row at every lookup, keyed by (seed of the last
                                              myo_reset / myo_autoreset, the env's episode count, global env id, env step); `seed`, `autoreset`
                                              and `max_episode_steps` above are unused.  Needs robot_dim = nq - 6, object_dim = 7, nq = nv */
} myo_track_config;

typedef enum myo_terrain { MYO_TERRAIN_NONE = 0, MYO_TERRAIN_ROUGH = 1, MYO_TERRAIN_HILLY = 2, MYO_TERRAIN_STAIRS = 3 } myo_terrain;

const char* myo_last_error(void);
int myo_version(void);

int myo_model_load(const void* blob, size_t nbytes, int device, myo_model** out);
void myo_model_free(myo_model*);
int myo_model_dims(const myo_model*, myo_dims* out);
/* test switches mirroring the oracle's (disable contacts / limits / ellipsoid pairs) */
int myo_model_set_switch(myo_model*, int disable_contact, int disable_limit, int disable_ellipsoid);

int myo_batch_create(const myo_model*, int B, myo_batch** out);
void myo_batch_free(myo_batch*);
int myo_batch_size(const myo_batch*);
int myo_batch_configure(myo_batch*, const myo_task_config* cfg);
int myo_batch_configure_walk(myo_batch*, const myo_walk_config* cfg);
int myo_batch_configure_track(myo_batch*, const myo_track_config* cfg);
/* muscle conditions (envs/myo/base_v0.py:61-80): time step of the fatigue model (frame_skip * timestep) and the actuator ids of
 * the EIP -> EPL tendon transfer (-1: none).  Sarcopenia is a model edit (peak force of gainprm halved) made before myo_model_load. */
int myo_batch_set_condition(myo_batch*, int frame_skip, int epl_actuator, int eip_actuator);
/* fatigue state at reset (CumulativeFatigue.reset, envs/myo/fatigue.py:114-134; BaseV0 kwargs fatigue_reset_vec / fatigue_reset_random,
 * base_v0.py:30-31,120-127): mode 0 all rested (MA 0, MR 1, MF 0); 1 random (u1, u2 ~ U(0,1): MA = u1 u2, MR = u1 (1 - u2), MF = 1 - u1);
 * 2 a given fatigue vector (host, nu floats; MF = vec, MR = 1 - vec, MA = 0) */
int myo_batch_set_fatigue_reset(myo_batch*, int mode, const float* fatigue_vec);
/* per-env size of ONE collision geom (compiled-model geom id), as ObjHoldRandomEnvV0.reset edits model.geom_size per episode
 * (envs/myo/myobase/obj_hold_v0.py:122-140): every reset of an env draws size ~ U(lo, hi) per axis; mass and inertia are untouched, as in
 * the reference (the model is not recompiled).  lo == hi == NULL switches the override off.  Generic large-kernel models only. */
int myo_batch_set_geom_override(myo_batch*, int geom_id, const float* size_lo, const float* size_hi);
/* touch sensors: myo_batch_enable_sensors / myo_model_nsensor are declared in myo_hip_sensors.h (included at the end of this file) */
/* device pointer + pitch (elements per env row) of a field */
int myo_batch_field(myo_batch*, int field, void** dev_ptr, size_t* pitch, size_t* width);
/* synchronous host copies (tests / plumbing without torch); host buffers are [B][width] */
int myo_batch_read(myo_batch*, int field, void* host, size_t nbytes);
int myo_batch_write(myo_batch*, int field, const void* host, size_t nbytes);

/* reset envs whose mask byte is nonzero (mask == NULL: all); mask is a DEVICE pointer, B bytes */
int myo_reset(myo_batch*, const uint8_t* mask_dev, uint64_t seed, void* stream);
/* overwrite state from device arrays [B][n] (NULL = leave field unchanged) */
int myo_set_state(myo_batch*, const float* qpos, const float* qvel, const float* act, const float* time, void* stream);
/* one env step: ctrl = actmap(action[B][nu]) (action == NULL: keep MYO_F_CTRL), then nsubsteps physics substeps */
int myo_step(myo_batch*, const float* action_dev, int actmap, int nsubsteps, void* stream);
/* observation / reward / done for the configured task into MYO_F_OBS / REWARD / DONE / SOLVED */
int myo_obs(myo_batch*, void* stream);
/* observation vector only (reward / done / solved untouched): used after an auto-reset */
int myo_obs_only(myo_batch*, void* stream);
/* observation vector only, and only for envs whose elapsed-step counter is 0 (i.e. those myo_autoreset just reset) */
int myo_obs_reset_only(myo_batch*, void* stream);
/* gym TimeLimit + done handling (envs/myo/myobase/__init__.py max_episode_steps): reset every env whose done flag is
 * set or whose elapsed env-step counter reached max_episode_steps, with the configured reset / target sampling */
int myo_autoreset(myo_batch*, int max_episode_steps, uint64_t seed, void* stream);
/* global id of this batch's env 0 (multi-GPU sharding: RNG streams are keyed by global env id) */
int myo_set_env_offset(myo_batch*, int env_offset);
/* copy per-env int32 flags to host and clear them */
int myo_status(myo_batch*, int32_t* host_flags);
/* fill action[B][nu] with U(-1,1) from a counter-based generator (seed, step, global env id) */
int myo_random_action(myo_batch*, float* action_dev, uint64_t seed, uint64_t step, int env_offset, void* stream);
int myo_sync(void* stream);
/* cost-sorted workgroup -> env placement for the wave-per-env kernel (default on; speed only, results unchanged) */
int myo_set_balance(myo_batch*, int on);
/* lanes cooperating on one env (16, 32 or 64; default 16 or $MYO_LANES) -- a tuning knob, results are identical up to float round-off */
int myo_set_lanes(int lanes);
/* diagnostic build (-DMYO_STAMPS=1) only: per-workgroup clock64 totals per kernel stage; returns 1 in the normal build */
int myo_read_stamps(myo_batch*, long long* host, int nwg);

/* timing helper for bench.py: run `steps` env steps on `stream` bracketed by HIP events recorded on that same
 * stream; returns elapsed milliseconds in *ms_out.  mode bits select what runs inside the timed region. */
enum { MYO_BENCH_OBS = 1, MYO_BENCH_FRESH_ACTIONS = 2, MYO_BENCH_AUTORESET = 4 };
int myo_bench_rollout(myo_batch*, int steps, int nsubsteps, uint64_t seed, int mode, int max_episode_steps, void* stream, float* ms_out);
/* ms_out == NULL makes myo_bench_rollout asynchronous: launches are enqueued on `stream` and nothing waits (a multi-GPU caller puts
 * its observation all-gather on the same stream between calls).
 * myo_bench_last_kernel_ms: HIP-event milliseconds spent inside the step-kernel launches of the last synchronous call, or of all
 * asynchronous calls since the previous collection (waits for them); events are recorded on the launches' own stream */
int myo_bench_last_kernel_ms(myo_batch*, float* ms_out);
/* roofline probe (no reference counterpart): measured chip-wide issue rate of wave64 v_fma_f32 instructions per second with
 * `waves_per_simd` (1..4, or 8 = two workgroups per CU) waves resident on every SIMD; bench.py prices the step kernel's VALU instruction
 * count against the figure at 4, the occupancy the hand kernel runs at */
int myo_probe_valu(int device, int waves_per_simd, int iters, double* wave_insts_per_s, int* n_cu_out);
/* name of the step-kernel template instantiation the last launch used, spelled as rocprofv3 prints it */
const char* myo_bench_last_kernel_name(const myo_batch*);

/* ---- policy inference: the network family of the reference's `mjx_brax_policy` artefact (a brax PPO
 * policy: running-statistics observation normalisation, MLP with swish hidden layers, tanh-normal head; brax is third-party and
 * absent from the reference tree, so the formulas are restated from its documentation -- parity unpinned).
 *   x = (obs - mean) / std ; h_{l+1} = swish(h_l W_l + b_l) ; (loc, raw) = split(h_L W_L + b_L) ;
 *   action = tanh(loc)                                   (deterministic)
 *          = tanh(loc + (softplus(raw) + 0.001) * eps)    (sampled; eps ~ N(0,1) from the counter RNG (seed, step, global env id))
 * Kernels are row-major [in][out] float32, copied at load time.  obs / action are DEVICE pointers, env-major, e.g. the
 * MYO_F_OBS buffer and the action argument of myo_step: a rollout never leaves the GPU. */
typedef struct myo_policy myo_policy;
int myo_policy_load(int device, int obs_dim, int act_dim, int nlayers, const int* layer_out /* nlayers entries, last = 2*act_dim */,
                    const float* obs_mean, const float* obs_std, const float* const* kernels, const float* const* biases, myo_policy** out);
void myo_policy_free(myo_policy*);
int myo_policy_act(myo_policy*, const float* obs_dev, int B, float* action_dev, int deterministic, uint64_t seed, uint64_t step,
                   int env_offset, void* stream);

#include "myo_hip_sensors.h"
#include "myo_hip_rewards.h"
#include "myo_hip_obs.h"
#include "myo_hip_ppo.h"

#ifdef __cplusplus
}
#endif
#endif
