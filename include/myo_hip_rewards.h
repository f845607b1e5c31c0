/* myo_hip_rewards.h -- reward terms, weighted_reward_keys and episode statistics of the HIP stepper (included by myo_hip.h; not a
 * stand-alone header).  An extension of libmyo_hip.so only: the float64 oracle's twin of the ABI (oracle/myo_oracle_abi.c) has no
 * counterpart, the float64 side of the check is tests/reward_terms_ref.py.
 *
 * The reference's envs return the reward as a dictionary (get_reward_dict: the task's named terms, then sparse, solved, done, and dense =
 * the sum of the terms weighted by weighted_reward_keys; envs/env_base.py:559-570 puts it into `info`).  Here every env gets one float32
 * row with those columns, in the reference's order for the configured task, `dense` last:
 *   MYO_TASK_POSE     pose, bonus, penalty, act_reg                                   envs/myo/myobase/pose_v0.py:118-135
 *   MYO_TASK_REACH    reach, bonus, act_reg, penalty                                  reach_v0.py:126-141
 *   MYO_TASK_STAND    reach, bonus, act_reg, penalty                                  walk_v0.py:117-133
 *   MYO_TASK_HOLD     goal_dist, bonus, act_reg, penalty                              obj_hold_v0.py:102-117
 *   MYO_TASK_KEYTURN  key_turn, IFtip_approach, THtip_approach, act_reg, bonus, penalty   key_turn_v0.py:134-152
 *   MYO_TASK_PEN      pos_align, rot_align, act_reg, drop, bonus                      pen_v0.py:150-167
 *   MYO_TASK_WALK     vel_reward, cyclic_hip, ref_rot, joint_angle_rew, act_mag       walk_v0.py:298-311
 *   MYO_TASK_BAODING  pos_dist_1, pos_dist_2, act_reg                                 envs/myo/myochallenge/baoding_v1.py:239-262
 *   MYO_TASK_DIE      pos_dist, rot_dist, bonus, act_reg, penalty                     reorient_v0.py:148-176
 * each followed by sparse, solved, done, dense.  The row is written by the launch that writes MYO_F_REWARD (myo_obs, the walk task's
 * myo_step, myo_bench_rollout's epilogue) and, like the reward, describes the transition just made: the state before an auto-reset.
 * myo_obs_only / myo_obs_reset_only leave it alone.  The MyoDM track task has no row: its terms are MYO_F_METRICS. */
#ifndef MYO_HIP_REWARDS_H
#define MYO_HIP_REWARDS_H

enum { MYO_RWD_DENSE = 0, MYO_RWD_SPARSE = 1 };   /* what MYO_F_REWARD holds: the dense column or the sparse one (env_base's rwd_mode) */

/* columns of the configured task's row, dense included (0: the task has no row), and the name of column `col` (NULL out of range) */
int myo_batch_rwd_ncol(const myo_batch*);
const char* myo_batch_rwd_name(const myo_batch*, int col);
/* Allocates the row and turns it on, after the task was configured: weights = one float per column except dense (nweights = ncol - 1,
 * copied; a column the caller does not weigh gets 0), dense = sum_k weights[k] * row[k].  From then on MYO_F_REWARD is the row's dense (or,
 * with MYO_RWD_SPARSE, sparse) column rather than the kernel's fixed-weight sum -- the same number up to float32 rounding when the weights
 * are the configured ones.  A second call replaces weights and mode.  Without it nothing is allocated and no launch is added */
int myo_batch_enable_rewards(myo_batch*, const float* weights, int nweights, int mode);
/* device pointer / pitch / width (= ncol) of the row; MYO_E_ARG until enabled */
int myo_batch_rwd_row(myo_batch*, void** dev_ptr, size_t* pitch, size_t* width);
/* synchronous host copy of the rows, [B][ncol] float32 (plumbing without torch, like myo_batch_read) */
int myo_batch_rwd_read(myo_batch*, void* host, size_t nbytes);

/* Episode statistics for batches whose finished episodes are reset in place (the device-side gym RecordEpisodeStatistics).  Needs the
 * reward terms.  myo_episode_update, once per env step after the observation pass and before myo_autoreset, adds (dense, sparse, 1, solved) to
 * every env's running row; for an env whose episode ends by myo_autoreset's rule (done, or elapsed >= max_episode_steps) it copies the
 * running row to the env's `last` row, raises the env's `finished` byte, counts the episode and clears the running row; the other envs'
 * bytes are cleared.  myo_episode_clear zeroes the running rows and the bytes (a caller-driven reset of all envs) */
enum { MYO_EP_RUNNING = 0,   /* [B][4] float32: dense return, sparse return, length, solved steps of the episode under way */
       MYO_EP_LAST = 1,      /* [B][4] float32: the same of the env's last finished episode */
       MYO_EP_FINISHED = 2,  /* [B] uint8: 1 if the last update ended the env's episode */
       MYO_EP_COUNT = 3      /* [B] int32: episodes ended so far */ };
int myo_batch_enable_episode_stats(myo_batch*);
int myo_batch_episode_buffer(myo_batch*, int which, void** dev_ptr, size_t* pitch, size_t* width);
/* synchronous host copy of one of the buffers, B * width elements of its type */
int myo_batch_episode_read(myo_batch*, int which, void* host, size_t nbytes);
int myo_episode_update(myo_batch*, int max_episode_steps, void* stream);
int myo_episode_clear(myo_batch*, void* stream);

#endif
