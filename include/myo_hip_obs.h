/* myo_hip_obs.h -- observation terms, obs_keys and proprio_keys of the HIP stepper (included by myo_hip.h; not a stand-alone header).  An
 * extension of libmyo_hip.so only: the float64 oracle's twin of the ABI (oracle/myo_oracle_abi.c) has no counterpart.
 *
 * The reference's envs keep their observation as a dictionary (get_obs_dict of the task's env class) and build the policy's input by
 * concatenating the entries named by obs_keys (envs/env_base.py obsdict2obsvec), and the proprioception vector by concatenating those named
 * by proprio_keys (env_base.py:512-531).  Here every configured task has a table of those terms, in the reference's order:
 *   MYO_TASK_POSE     time, qpos, qvel, act, pose_err                                                    envs/myo/myobase/pose_v0.py
 *   MYO_TASK_REACH    time, qpos, qvel, act, tip_pos, target_pos, reach_err                              reach_v0.py
 *   MYO_TASK_STAND    time, qpos, qvel, act, tip_pos, target_pos, reach_err                              walk_v0.py (ReachEnvV0)
 *   MYO_TASK_HOLD     time, hand_qpos, hand_qvel, obj_pos, obj_err, act                                  obj_hold_v0.py
 *   MYO_TASK_KEYTURN  time, hand_qpos, hand_qvel, key_qpos, key_qvel, IFtip_approach, THtip_approach, act    key_turn_v0.py
 *   MYO_TASK_PEN      time, hand_jnt, obj_pos, obj_des_pos, obj_vel, obj_rot, obj_des_rot, obj_err_pos, obj_err_rot, act   pen_v0.py
 *   MYO_TASK_WALK     t, time, qpos_without_xy, qvel, com_vel, torso_angle, feet_heights, height, feet_rel_positions, phase_var,
 *                     muscle_length, muscle_velocity, muscle_force, act                                  walk_v0.py (WalkEnvV0)
 *   MYO_TASK_BAODING  time, hand_pos, object1_pos, object2_pos, object1_velp, object2_velp, target1_pos, target2_pos, target1_err,
 *                     target2_err, act                                                                   envs/myo/myochallenge/baoding_v1.py
 *   MYO_TASK_DIE      time, hand_qpos_noMD5, hand_qpos, hand_qvel, obj_pos, goal_pos, pos_err, obj_rot, goal_rot, rot_err, act   reorient_v0.py
 * A term's width follows from the model (nq, nv, nu, the number of muscles, the number of tips); `act` has width 0 for a model without
 * muscles, except in the pose task, where the reference fills it with nq zeros.  No task, and the MyoDM track task, have no table.
 *
 * MYO_F_OBS stays the canonical row with the canonical obs_dim, written by the same kernels as before.  Once enabled, one more launch
 * (obs_terms_kernel) follows every launch that wrote MYO_F_OBS -- myo_obs, myo_obs_only, myo_obs_reset_only and, for the walk task, myo_step
 * -- and rewrites the three rows below for ALL envs from the current buffers (so it needs no reset mask and may run any number of times).
 * Most terms are slices of MYO_F_OBS and are copied bit for bit; time / t come from MYO_F_TIME, target_pos from MYO_F_TARGET, the die's
 * hand_qpos from MYO_F_QPOS, the baoding and die tasks' act from MYO_F_ACT, and the pen's obj_des_pos (a site of the world body) from a
 * constant of the batch.  Unlike the reward-term row, which describes the transition just made, the rows describe the observation that
 * MYO_F_OBS holds: after an auto-reset and myo_obs_reset_only, an env that was reset shows its first observation (time = 0). */
#ifndef MYO_HIP_OBS_H
#define MYO_HIP_OBS_H

enum { MYO_OBS_TERMS = 0,      /* [B][sum of all term widths] float32: every term of the table, in table order */
       MYO_OBS_SELECTED = 1,   /* [B][selected width] float32: the obs_keys concatenation */
       MYO_OBS_PROPRIO = 2     /* [B][proprio width] float32: the proprio_keys concatenation; absent (MYO_E_ARG) when none were given */ };

/* the table of the configured task: number of terms (0: the task has none), name of term k (NULL out of range) and its width in floats
 * (0: the model lacks the term; -1 out of range) */
int myo_batch_obs_nterm(const myo_batch*);
const char* myo_batch_obs_term_name(const myo_batch*, int k);
int myo_batch_obs_term_width(const myo_batch*, int k);
/* The same table by value, with no batch and no device: the table of `task` (a MYO_TASK_* id) for a model of the given dimensions -- nq, nv,
 * nu, na (its muscles), ntip (reach tips; 1 for the stand task) and pose_act (na, or nq for a model without muscles).  Returns the number of
 * terms (0: the task has no table) and, for term k, its name (NULL out of range), its width (-1 out of range) and its offset in the canonical
 * row MYO_F_OBS (-1: the term comes from outside the row, or k is out of range); *row_dim = the width of the canonical row.  Any out-pointer
 * may be NULL.  The three calls above answer from this table, with the dimensions of the batch's model */
int myo_obs_term_table(int task, int nq, int nv, int nu, int na, int ntip, int pose_act, int k, const char** name, int* width, int* offset, int* row_dim);
/* Allocates the three rows and turns the extra launch on, after the task was configured.  obs_terms[nobs] / proprio_terms[nproprio]: indices
 * into the table, in concatenation order; an index may repeat; nobs >= 1; nproprio == 0 (proprio_terms may be NULL): no MYO_OBS_PROPRIO.
 * Refused: no task or the MyoDM track task (MYO_E_UNSUPPORTED), the walk task with myo_set_lanes != 64 (MYO_E_UNSUPPORTED), an index out
 * of range or of a term the model lacks (MYO_E_ARG), a pen model whose eps_ball site is not on the world body (MYO_E_UNSUPPORTED), and a
 * second call (MYO_E_ARG: the rows are handed out as device pointers, so a batch selects once).  While enabled the batch cannot be
 * configured again.  Without the call nothing is allocated and no launch is added */
int myo_batch_enable_obs_terms(myo_batch*, const int* obs_terms, int nobs, const int* proprio_terms, int nproprio);
/* device pointer / pitch / width of one of the rows; MYO_E_ARG until enabled */
int myo_batch_obs_buffer(myo_batch*, int which, void** dev_ptr, size_t* pitch, size_t* width);
/* synchronous host copy of one of the rows, [B][width] float32 */
int myo_batch_obs_read(myo_batch*, int which, void* host, size_t nbytes);

#endif
