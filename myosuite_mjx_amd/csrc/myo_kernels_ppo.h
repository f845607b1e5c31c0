// myo_kernels_ppo.h -- the device side of PPO training (include/myo_hip_ppo.h): sampling with log-probabilities, GAE.
// Part of the single translation unit myo_hip.hip (included there after myo_kernels_aux.h); not a stand-alone header.
#ifndef MYO_KERNELS_PPO_H
#define MYO_KERNELS_PPO_H

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
