/* myo_hip_ppo.h -- the device side of on-policy training (PPO) with a myo_policy (included by myo_hip.h; not a stand-alone header).
 * An extension of libmyo_hip.so only: the float64 oracle's twin of the ABI (oracle/myo_oracle_abi.c) has no counterpart, the float64 side
 * of the check is tests/ppo_ref.py.  brax is third-party and absent from the reference tree, so its formulas are restated here from its
 * documentation -- parity with brax itself is unpinned, as for myo_policy_act.  The learner on top is myosuite_mjx_amd/ppo.py. */
#ifndef MYO_HIP_PPO_H
#define MYO_HIP_PPO_H

/* Overwrites the device buffers of a loaded policy in place; shapes are those given to myo_policy_load.  Any pointer, and any entry of
 * kernels / biases (nlayers entries each), may be NULL: that buffer is kept.  src_is_device = 0: host pointers, the call returns after
 * the copies are done.  src_is_device = 1: device pointers (e.g. the storage of a learner's parameters), copied device-to-device on
 * `stream` without allocation or host synchronisation: launches queued on that stream before the call see the old weights, later ones
 * the new */
int myo_policy_update(myo_policy*, const float* obs_mean, const float* obs_std, const float* const* kernels, const float* const* biases,
                      int src_is_device, void* stream);

/* myo_policy_act(deterministic = 0) that keeps what a learner needs.  action_dev [B][act_dim] is bit-identical to what myo_policy_act
 * writes for the same (seed, step, env_offset); raw_dev [B][act_dim] = u, the pre-tanh sample (action = tanh(u));
 *   logp_dev [B] = sum_j [ log N(u_j; loc_j, scale_j) - 2 (log 2 - u_j - softplus(-2 u_j)) ],   scale = softplus(raw) + 0.001
 * the log-density of the action under the tanh-normal, in the form that stays finite where tanh saturates */
int myo_policy_sample(myo_policy*, const float* obs_dev, int B, float* action_dev, float* raw_dev, float* logp_dev, uint64_t seed,
                      uint64_t step, int env_offset, void* stream);

/* Generalised advantage estimation over an unroll, brax's compute_gae.  Device arrays [T][B] float32 with B fastest, bootstrap [B]:
 *   mask_t   = 1 - truncation_t
 *   v_next_t = values_{t+1}                                                            (bootstrap for t = T-1)
 *   delta_t  = (rewards_t + discount (1 - termination_t) v_next_t - values_t) mask_t
 *   acc_t    = delta_t + discount (1 - termination_t) mask_t lambda acc_{t+1}          (acc_T = 0)
 *   vs_t     = acc_t + values_t
 *   adv_t    = (rewards_t + discount (1 - termination_t) vs_{t+1} - values_t) mask_t   (vs_T = bootstrap)
 * One launch on `stream`.  MYO_E_ARG for T <= 0, B <= 0 or a NULL pointer */
int myo_ppo_gae(const float* rewards, const float* values, const float* bootstrap, const float* termination, const float* truncation,
                int T, int B, float discount, float lambda, float* vs_out, float* adv_out, void* stream);

#endif
