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

/* ---- The learner: one PPO minibatch SGD step on the device (kernels: csrc/myo_kernels_learner.h; Python: ppo.Learner, ppo.train(update="hip")).
 * It owns both networks' parameters, their gradients and the Adam moments, and the workspace of a step.  Networks: swish MLPs as in
 * myo_policy_load, kernels [in][out]; the policy's last layer is 2 * act_dim wide (loc, raw; scale = softplus(raw) + 0.001), the value
 * network's is 1 wide.  Limits: obs_dim >= 1, 1..8 layers of width 1..512 per network; outside them MYO_E_UNSUPPORTED.
 * The Adam hyperparameters are doubles because torch.optim.Adam takes them as doubles and forms 1 - beta in double before it rounds to
 * float32: 1 - (float)0.999 is off from 0.001 by 1.3e-5 of it.  No weight decay; bias-corrected as torch does it
 * (step = lr / (1 - beta1^t), denom = sqrt(v) / sqrt(1 - beta2^t) + eps). */
typedef struct myo_ppo_learner myo_ppo_learner;
typedef struct myo_ppo_config {
  int obs_dim, act_dim;
  int policy_nlayers, policy_out[8];      /* last = 2 * act_dim */
  int value_nlayers, value_out[8];        /* last = 1 */
  int max_unroll, max_minibatch;          /* the workspace holds (max_unroll + 1) * max_minibatch rows; allocated by create */
  double learning_rate, beta1, beta2, adam_eps;
  float discounting, gae_lambda, clipping_epsilon, entropy_cost, reward_scaling;
  int normalize_advantage;
} myo_ppo_config;

/* Host arrays, one per layer, kernels [in][out].  MYO_E_ARG: a NULL pointer, obs_dim / act_dim / max_unroll / max_minibatch < 1, no layer, a
 * width < 1, a policy head that is not 2 * act_dim wide or a value head that is not 1 wide */
int myo_ppo_learner_create(int device, const myo_ppo_config* config, const float* const* policy_kernels, const float* const* policy_biases,
                           const float* const* value_kernels, const float* const* value_biases, myo_ppo_learner** out);
void myo_ppo_learner_free(myo_ppo_learner*);

/* One SGD step on the unrolls idx[0 .. mb) of a rollout.  Device arrays, float32: obs [T+1][B][obs_dim]; u [T][B][act_dim] (pre-tanh
 * samples); logp, rewards, termination, truncation [T][B]; idx: mb int64 env columns in [0, B), any order, no repeats; obs_mean, obs_std
 * [obs_dim]; entropy_noise [T][mb][act_dim].  Row t * mb + i of the minibatch is env idx[i] at time t.
 *   x      = (obs - obs_mean) / obs_std;  (loc, raw) = policy(x) on the rows t < T;  V = value(x) on all T + 1 rows
 *   vs, A  = the recurrence of myo_ppo_gae on rewards * reward_scaling, V and the bootstrap V_T; constants for the gradient
 *   A      = (A - mean A) / (std A + 1e-8) if normalize_advantage (over the T * mb values, std with 1 / N)
 *   rho    = exp(log pi(u) - logp);  policy = -mean(min(rho A, clip(rho, 1 - eps, 1 + eps) A))
 *   value  = 1/4 mean((vs - V)^2);   entropy = -entropy_cost mean(entropy at loc + scale * entropy_noise)
 * then one Adam step on policy + value + entropy.  loss_sums (device, 3 floats, may be NULL): the three terms of this step are ADDED to it
 * by one thread.  Everything runs on `stream`; nothing is allocated and the host is not synchronised.  The number of launches is
 * 3 (policy_nlayers + value_nlayers) + 2.  Every sum has a fixed order and no atomics: equal inputs give bit-equal parameters.
 * NaNs in the inputs propagate into the parameters, as with torch; nothing guards against them.
 * MYO_E_ARG (nothing is launched): a NULL pointer other than loss_sums, T < 1, mb < 1, T > max_unroll, mb > max_minibatch, mb > B */
int myo_ppo_learner_step(myo_ppo_learner*, const float* obs, const float* u, const float* logp, const float* rewards, const float* termination,
                         const float* truncation, int T, int B, const int64_t* idx, int mb, const float* obs_mean, const float* obs_std,
                         const float* entropy_noise, float* loss_sums, void* stream);

/* Device pointer and element count of one of the learner's tensors: net 0 policy / 1 value; what 0 kernel [in][out] / 1 bias;
 * which 0 parameter / 1 gradient of the last step / 2 Adam's first moment / 3 its second.  The pointers stay valid until free */
int myo_ppo_learner_tensor(myo_ppo_learner*, int net, int layer, int what, int which, float** dev_ptr, size_t* count);

#endif
