// myo_host_policy.h -- the device policy on the host: myo_policy with its load / free / act (include/myo_hip.h) and, for PPO training, its
// in-place update, sampling with log-probabilities and the GAE launch (include/myo_hip_ppo.h).  Kernels: myo_kernels_ppo.h.
#ifndef MYO_HOST_POLICY_H
#define MYO_HOST_POLICY_H

struct myo_policy {
  int device = 0;
  PolicyDev pd{};
  DevPool pool;
};

int myo_policy_load(int device, int obs_dim, int act_dim, int nlayers, const int* layer_out, const float* obs_mean, const float* obs_std,
                    const float* const* kernels, const float* const* biases, myo_policy** out) {
  if (!out || !layer_out || !obs_mean || !obs_std || !kernels || !biases || obs_dim <= 0 || act_dim <= 0 || nlayers <= 0 || nlayers > 8)
    return fail(MYO_E_ARG, "myo_policy_load: bad arguments");
  if (layer_out[nlayers - 1] != 2 * act_dim) return fail(MYO_E_ARG, "myo_policy_load: last layer must have 2*act_dim outputs (loc, scale)");
  for (int l = 0; l < nlayers; l++) if (layer_out[l] <= 0 || layer_out[l] > 512) return fail(MYO_E_UNSUPPORTED, "myo_policy_load: layer width must be in 1..512");
  int rc = use_device(device, "myo_policy_load");
  if (rc) return rc;
  std::unique_ptr<myo_policy> p(new myo_policy());   // a failed load frees what it had uploaded
  p->device = device;
  PolicyDev& P = p->pd;
  P.obs_dim = obs_dim; P.act_dim = act_dim; P.nlayers = nlayers;
  if ((rc = p->pool.upload(&P.mean, obs_mean, obs_dim)) || (rc = p->pool.upload(&P.std, obs_std, obs_dim))) return rc;
  int nin = obs_dim;
  for (int l = 0; l < nlayers; l++) {
    P.width[l] = layer_out[l];
    if ((rc = p->pool.upload(&P.W[l], kernels[l], (size_t)nin * layer_out[l])) || (rc = p->pool.upload(&P.b[l], biases[l], layer_out[l]))) return rc;
    nin = layer_out[l];
  }
  *out = p.release();
  return MYO_OK;
}

void myo_policy_free(myo_policy* p) { delete p; }

// dynamic LDS of the policy kernels: two activation rows per env of a workgroup, as wide as the widest of observation, POL_MAXW and the
// layers (policy_forward, myo_kernels_ppo.h); 0: wider than the 64 KB a workgroup may ask for
static size_t policy_lds_bytes(const PolicyDev& P) {
  int stride = P.obs_dim > POL_MAXW ? P.obs_dim : POL_MAXW;
  for (int l = 0; l < P.nlayers; l++) if (P.width[l] > stride) stride = P.width[l];
  const size_t lds = (size_t)2 * POL_ENVS * stride * 4;
  return lds > 64 * 1024 ? 0 : lds;
}

int myo_policy_act(myo_policy* p, const float* obs_dev, int B, float* action_dev, int deterministic, uint64_t seed, uint64_t step,
                   int env_offset, void* stream) {
  if (!p || !obs_dev || !action_dev || B <= 0) return fail(MYO_E_ARG, "myo_policy_act: bad arguments");
  HIPCHK(hipSetDevice(p->device));
  const size_t lds = policy_lds_bytes(p->pd);
  if (!lds) return fail(MYO_E_UNSUPPORTED, "myo_policy_act: observation too wide for the LDS tile");
  hipLaunchKernelGGL(policy_kernel, dim3((B + POL_ENVS - 1) / POL_ENVS), dim3(POL_ENVS * POL_MAXW), lds, (hipStream_t)stream, p->pd, obs_dev, B,
                     action_dev, deterministic, seed, step, env_offset);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

int myo_policy_update(myo_policy* p, const float* obs_mean, const float* obs_std, const float* const* kernels, const float* const* biases,
                      int src_is_device, void* stream) {
  if (!p) return fail(MYO_E_ARG, "myo_policy_update: null policy");
  HIPCHK(hipSetDevice(p->device));
  const PolicyDev& P = p->pd;
  const hipMemcpyKind kind = src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  auto put = [&](const float* dst, const float* src, size_t n) -> hipError_t {
    return src ? hipMemcpyAsync(const_cast<float*>(dst), src, n * 4, kind, (hipStream_t)stream) : hipSuccess;
  };
  HIPCHK(put(P.mean, obs_mean, P.obs_dim));
  HIPCHK(put(P.std, obs_std, P.obs_dim));
  int nin = P.obs_dim;
  for (int l = 0; l < P.nlayers; l++) {
    if (kernels) HIPCHK(put(P.W[l], kernels[l], (size_t)nin * P.width[l]));
    if (biases) HIPCHK(put(P.b[l], biases[l], P.width[l]));
    nin = P.width[l];
  }
  if (!src_is_device) HIPCHK(hipStreamSynchronize((hipStream_t)stream));      // the caller may free its host arrays on return
  return MYO_OK;
}

int myo_policy_sample(myo_policy* p, const float* obs_dev, int B, float* action_dev, float* raw_dev, float* logp_dev, uint64_t seed,
                      uint64_t step, int env_offset, void* stream) {
  if (!p || !obs_dev || !action_dev || !raw_dev || !logp_dev || B <= 0) return fail(MYO_E_ARG, "myo_policy_sample: bad arguments");
  HIPCHK(hipSetDevice(p->device));
  const size_t lds = policy_lds_bytes(p->pd);
  if (!lds) return fail(MYO_E_UNSUPPORTED, "myo_policy_sample: observation too wide for the LDS tile");
  hipLaunchKernelGGL(policy_sample_kernel, dim3((B + POL_ENVS - 1) / POL_ENVS), dim3(POL_ENVS * POL_MAXW), lds, (hipStream_t)stream, p->pd, obs_dev, B,
                     action_dev, raw_dev, logp_dev, seed, step, env_offset);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

int myo_ppo_gae(const float* rewards, const float* values, const float* bootstrap, const float* termination, const float* truncation,
                int T, int B, float discount, float lambda, float* vs_out, float* adv_out, void* stream) {
  if (!rewards || !values || !bootstrap || !termination || !truncation || !vs_out || !adv_out || T <= 0 || B <= 0)
    return fail(MYO_E_ARG, "myo_ppo_gae: bad arguments");
  hipLaunchKernelGGL(ppo_gae_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, rewards, values, bootstrap, termination, truncation,
                     T, B, discount, lambda, vs_out, adv_out);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

#endif  // MYO_HOST_POLICY_H
