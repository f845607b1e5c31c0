// myo_kernels_ppo.h -- the policy network on the device: inference (policy_kernel) and the device side of PPO training
// (include/myo_hip_ppo.h): sampling with log-probabilities, GAE.
// Part of the single translation unit myo_hip.hip (included there after myo_kernels_aux.h); not a stand-alone header.
#ifndef MYO_KERNELS_PPO_H
#define MYO_KERNELS_PPO_H

// ------------------------------------------------------------------------------------------------
// policy inference (brax PPO network family): 8 envs per 512-thread workgroup, thread = (env, hidden unit); activations ping-pong
// through LDS, weights are read coalesced across units and shared by the 8 envs through the cache.  ~13 kMAC per env for
// the hand observation: negligible next to the physics step, so plain FMAs (no MFMA)
#define POL_ENVS 8
#define POL_MAXW 64
struct PolicyDev {
  int obs_dim, act_dim, nlayers;
  int width[8];               // output width of each layer
  const float* W[8];
  const float* b[8];
  const float *mean, *std;
};
// The forward pass, shared by policy_kernel and policy_sample_kernel: one env = one wavefront (lane j of wave le);
// returns the env's head row in LDS, [loc[act_dim], raw[act_dim]].  Every thread of the workgroup calls it (it holds the barriers)
__device__ __forceinline__ const float* policy_forward(const PolicyDev& P, const float* __restrict__ obs, int B, float* sh, const int j, const int le, const int e) {
  int stride = max(P.obs_dim, POL_MAXW);
  for (int l = 0; l < P.nlayers; l++) stride = max(stride, P.width[l]);
  float* xin = sh + le * stride;
  float* xout = sh + (POL_ENVS + le) * stride;
  if (e < B)
    for (int i = j; i < P.obs_dim; i += POL_MAXW) xin[i] = (obs[(size_t)e * P.obs_dim + i] - P.mean[i]) / P.std[i];
  __syncthreads();
  int nin = P.obs_dim;
  for (int l = 0; l < P.nlayers; l++) {
    const int nout = P.width[l];
    if (e < B) {
      const float* Wl = P.W[l];
      for (int jj = j; jj < nout; jj += POL_MAXW) {
        float acc = P.b[l][jj];
        for (int i = 0; i < nin; i++) acc += xin[i] * Wl[(size_t)i * nout + jj];
        xout[jj] = (l + 1 < P.nlayers) ? acc / (1.0f + expf(-acc)) : acc;     // swish on hidden layers, linear head
      }
    }
    __syncthreads();
    float* t = xin; xin = xout; xout = t;
    nin = nout;
  }
  return xin;
}
// the tanh-normal head's draw for action jj of global env ge: u = loc + scale * eps, scale = softplus(raw) + 0.001, eps by Box-Muller
__device__ __forceinline__ float policy_draw(float loc, float raw, uint64_t seed, uint64_t step, uint64_t ge, int jj, float* scale_out) {
  float scale = (raw > 20.f ? raw : log1pf(expf(raw))) + 0.001f;
  float u1 = fmaxf(rng_u<RS_POLICY_U1>(seed, ge, jj, step), 1e-7f), u2 = rng_u<RS_POLICY_U2>(seed, ge, jj, step);
  *scale_out = scale;
  return loc + scale * sqrtf(-2.0f * logf(u1)) * cosf(6.283185307179586f * u2);   // Box-Muller
}
__global__ void __launch_bounds__(POL_ENVS * POL_MAXW) policy_kernel(PolicyDev P, const float* __restrict__ obs, int B, float* __restrict__ action,
                                                                     int deterministic, uint64_t seed, uint64_t step, int env_offset) {
  extern __shared__ float sh[];                       // [POL_ENVS][max(obs_dim, POL_MAXW)] x 2
  const int j = threadIdx.x % POL_MAXW, le = threadIdx.x / POL_MAXW;
  const int e = blockIdx.x * POL_ENVS + le;
  const float* head = policy_forward(P, obs, B, sh, j, le, e);
  if (e < B) {
    for (int jj = j; jj < P.act_dim; jj += POL_MAXW) {
      float a = head[jj], scale;
      if (!deterministic) a = policy_draw(a, head[P.act_dim + jj], seed, step, (uint64_t)(e + env_offset), jj, &scale);
      action[(size_t)e * P.act_dim + jj] = tanhf(a);
    }
  }
}

// softplus(x) = log(1 + e^x) without overflow: max(x, 0) + log1p(e^-|x|)
__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// policy_kernel's sampled branch that also keeps what an on-policy learner needs: u (the pre-tanh sample) and its log-probability under
// the tanh-normal, sum_j [ log N(u_j; loc_j, scale_j) - 2 (log 2 - u_j - softplus(-2 u_j)) ].  Same forward pass, RNG streams and draw as
// policy_kernel (policy_forward / policy_draw), so `action` is bit-identical to myo_policy_act(deterministic = 0).  One env = one wavefront:
// each lane sums its strided share of the act_dim terms, a __shfl_xor butterfly adds the 64 partial sums, lane 0 stores
__global__ void __launch_bounds__(POL_ENVS * POL_MAXW) policy_sample_kernel(PolicyDev P, const float* __restrict__ obs, int B, float* __restrict__ action,
                                                                            float* __restrict__ raw_out, float* __restrict__ logp_out,
                                                                            uint64_t seed, uint64_t step, int env_offset) {
  extern __shared__ float sh[];                       // as policy_kernel
  const int j = threadIdx.x % POL_MAXW, le = threadIdx.x / POL_MAXW;
  const int e = blockIdx.x * POL_ENVS + le;
  const float* head = policy_forward(P, obs, B, sh, j, le, e);
  if (e >= B) return;                                 // uniform over the wave (e depends on the wave's index only): the butterfly below sees all 64 lanes
  float part = 0.f;
  for (int jj = j; jj < P.act_dim; jj += POL_MAXW) {
    const float loc = head[jj];
    float scale;
    const float u = policy_draw(loc, head[P.act_dim + jj], seed, step, (uint64_t)(e + env_offset), jj, &scale);
    action[(size_t)e * P.act_dim + jj] = tanhf(u);
    raw_out[(size_t)e * P.act_dim + jj] = u;
    const float z = (u - loc) / scale;
    const float log_normal = -0.5f * z * z - logf(scale) - 0.9189385332046727f;                 // 0.5 log(2 pi)
    const float log_det = 2.0f * (0.6931471805599453f - u - softplus_f(-2.0f * u));             // log |d tanh(u) / du|
    part += log_normal - log_det;
  }
  for (int off = POL_MAXW / 2; off > 0; off >>= 1) part += __shfl_xor(part, off);
  if (j == 0) logp_out[e] = part;
}

// brax's compute_gae (restated in include/myo_hip_ppo.h): one thread per env column, one reverse pass over t with v_{t+1}, vs_{t+1} and the
// accumulator in registers; consecutive lanes read and write consecutive floats of row t
__global__ void __launch_bounds__(256) ppo_gae_kernel(const float* __restrict__ rewards, const float* __restrict__ values, const float* __restrict__ bootstrap,
                                                      const float* __restrict__ termination, const float* __restrict__ truncation, int T, int B,
                                                      float discount, float lambda, float* __restrict__ vs_out, float* __restrict__ adv_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float v_next = bootstrap[b], vs_next = v_next, acc = 0.f;
  for (int t = T - 1; t >= 0; t--) {
    const size_t i = (size_t)t * B + b;
    const float r = rewards[i], v = values[i];
    const float cont = discount * (1.0f - termination[i]), mask = 1.0f - truncation[i];
    const float delta = (r + cont * v_next - v) * mask;
    acc = delta + cont * mask * lambda * acc;
    const float vs = acc + v;
    vs_out[i] = vs;
    adv_out[i] = (r + cont * vs_next - v) * mask;
    v_next = v;
    vs_next = vs;
  }
}

#endif
