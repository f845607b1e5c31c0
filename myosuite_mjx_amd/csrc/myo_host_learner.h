// myo_host_learner.h -- the PPO learner on the host (include/myo_hip_ppo.h): its record, creation and destruction, the views of its
// tensors, and the SGD step as a fixed sequence of launches.  Kernels: myo_kernels_learner.h.
#ifndef MYO_HOST_LEARNER_H
#define MYO_HOST_LEARNER_H

struct LearnerNet {
  int nlayers = 0, width[8] = {};
  size_t off[8] = {};                 // of layer l's kernel in the flat parameter array; its bias follows at off + in * out
  float* Z[8] = {};                   // pre-activations [rows][width], and the loss's derivative with respect to them
  float* dZ[8] = {};
  int in(int l, int obs_dim) const { return l ? width[l - 1] : obs_dim; }
};

struct myo_ppo_learner {
  int device = 0;
  myo_ppo_config cfg{};
  LearnerNet net[2];                  // 0 policy, 1 value
  size_t total = 0;                   // floats in the flat parameter array
  float* flat = nullptr;              // [4][total]: parameters, gradients, Adam's m and v
  float* partial = nullptr;           // [LRN_MAXSPLIT or fewer][total]: the dW launches' split sums
  float *vs = nullptr, *adv = nullptr, *rowloss = nullptr, *stats = nullptr;
  long long steps = 0;
  DevPool pool;
};

static int learner_splits(int rows) { return std::min(LRN_MAXSPLIT, (rows + LRN_CHUNK - 1) / LRN_CHUNK); }

int myo_ppo_learner_create(int device, const myo_ppo_config* c, const float* const* policy_kernels, const float* const* policy_biases,
                           const float* const* value_kernels, const float* const* value_biases, myo_ppo_learner** out) {
  if (!out || !c || !policy_kernels || !policy_biases || !value_kernels || !value_biases || c->obs_dim < 1 || c->act_dim < 1 ||
      c->policy_nlayers < 1 || c->value_nlayers < 1 || c->max_unroll < 1 || c->max_minibatch < 1)
    return fail(MYO_E_ARG, "myo_ppo_learner_create: bad arguments");
  if (c->policy_nlayers > 8 || c->value_nlayers > 8) return fail(MYO_E_UNSUPPORTED, "myo_ppo_learner_create: at most 8 layers per network");
  const float* const* ks[2] = {policy_kernels, value_kernels};
  const float* const* bs[2] = {policy_biases, value_biases};
  for (int n = 0; n < 2; n++) {
    const int L = n ? c->value_nlayers : c->policy_nlayers;
    const int* w = n ? c->value_out : c->policy_out;
    for (int l = 0; l < L; l++) {
      if (w[l] < 1 || !ks[n][l] || !bs[n][l]) return fail(MYO_E_ARG, "myo_ppo_learner_create: a layer without width, kernel or bias");
      if (w[l] > 512) return fail(MYO_E_UNSUPPORTED, "myo_ppo_learner_create: layer width must be in 1..512");
    }
    if (w[L - 1] != (n ? 1 : 2 * c->act_dim)) return fail(MYO_E_ARG, "myo_ppo_learner_create: the policy head is 2 * act_dim wide, the value head 1");
  }
  int rc = use_device(device, "myo_ppo_learner_create");
  if (rc) return rc;
  const size_t rows = ((size_t)c->max_unroll + 1) * c->max_minibatch;
  if (rows > (size_t)1 << 30) return fail(MYO_E_UNSUPPORTED, "myo_ppo_learner_create: more than 2^30 rows");
  std::unique_ptr<myo_ppo_learner> p(new myo_ppo_learner());   // a failed create frees what it had allocated
  p->device = device;
  p->cfg = *c;
  DevPool& pool = p->pool;
  for (int n = 0; n < 2; n++) {
    LearnerNet& N = p->net[n];
    N.nlayers = n ? c->value_nlayers : c->policy_nlayers;
    for (int l = 0; l < N.nlayers; l++) {
      N.width[l] = (n ? c->value_out : c->policy_out)[l];
      N.off[l] = p->total;
      p->total += ((size_t)N.in(l, c->obs_dim) + 1) * N.width[l];
      if ((rc = pool.alloc(&N.Z[l], rows * N.width[l] * 4)) || (rc = pool.alloc(&N.dZ[l], rows * N.width[l] * 4))) return rc;
    }
  }
  if ((rc = pool.alloc(&p->flat, 4 * p->total * 4)) || (rc = pool.alloc(&p->partial, (size_t)learner_splits((int)rows) * p->total * 4)) ||
      (rc = pool.alloc(&p->vs, rows * 4)) || (rc = pool.alloc(&p->adv, rows * 4)) || (rc = pool.alloc(&p->rowloss, 3 * rows * 4)) ||
      (rc = pool.alloc(&p->stats, 2 * 4))) return rc;
  for (int n = 0; n < 2; n++)
    for (int l = 0; l < p->net[n].nlayers; l++) {
      const LearnerNet& N = p->net[n];
      const size_t nk = (size_t)N.in(l, c->obs_dim) * N.width[l];
      HIPCHK(hipMemcpy(p->flat + N.off[l], ks[n][l], nk * 4, hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(p->flat + N.off[l] + nk, bs[n][l], (size_t)N.width[l] * 4, hipMemcpyHostToDevice));
    }
  *out = p.release();
  return MYO_OK;
}

void myo_ppo_learner_free(myo_ppo_learner* p) { delete p; }

int myo_ppo_learner_tensor(myo_ppo_learner* p, int net, int layer, int what, int which, float** dev_ptr, size_t* count) {
  if (!p || !dev_ptr || !count || net < 0 || net > 1 || what < 0 || what > 1 || which < 0 || which > 3 || layer < 0 || layer >= p->net[net].nlayers)
    return fail(MYO_E_ARG, "myo_ppo_learner_tensor: bad arguments");
  const LearnerNet& N = p->net[net];
  const size_t nk = (size_t)N.in(layer, p->cfg.obs_dim) * N.width[layer];
  *dev_ptr = p->flat + (size_t)which * p->total + N.off[layer] + (what ? nk : 0);
  *count = what ? (size_t)N.width[layer] : nk;
  return MYO_OK;
}

int myo_ppo_learner_step(myo_ppo_learner* p, const float* obs, const float* u, const float* logp, const float* rewards, const float* termination,
                         const float* truncation, int T, int B, const int64_t* idx, int mb, const float* obs_mean, const float* obs_std,
                         const float* entropy_noise, float* loss_sums, void* stream) {
  if (!p || !obs || !u || !logp || !rewards || !termination || !truncation || !idx || !obs_mean || !obs_std || !entropy_noise)
    return fail(MYO_E_ARG, "myo_ppo_learner_step: null pointer");
  if (T < 1 || mb < 1 || T > p->cfg.max_unroll || mb > p->cfg.max_minibatch || mb > B)
    return fail(MYO_E_ARG, "myo_ppo_learner_step: T in 1..max_unroll and mb in 1..min(max_minibatch, B)");
  HIPCHK(hipSetDevice(p->device));
  const myo_ppo_config& c = p->cfg;
  hipStream_t st = (hipStream_t)stream;
  const int rows_of[2] = {T * mb, (T + 1) * mb};
  const int S = learner_splits(rows_of[1]);
  const dim3 blk(256);
  auto tiles = [](int n) { return (unsigned)((n + LRN_TILE - 1) / LRN_TILE); };
  auto gemm = [&](int n, int l) {
    const LearnerNet& N = p->net[n];
    LearnerGemm g{};
    g.X = l ? N.Z[l - 1] : nullptr;
    g.W = p->flat + N.off[l];
    g.dZ = N.dZ[l];
    g.Zprev = g.X;
    g.obs = obs; g.idx = idx; g.mean = obs_mean; g.std = obs_std;
    g.rows = rows_of[n]; g.kdim = N.in(l, c.obs_dim); g.n = N.width[l]; g.mb = mb; g.B = B;
    g.chunk = ((rows_of[n] + S - 1) / S + LRN_TK - 1) / LRN_TK * LRN_TK;
    g.split_stride = p->total;
    return g;
  };
  // forward: Z_l = in_l W_l + b_l
  for (int n = 0; n < 2; n++)
    for (int l = 0; l < p->net[n].nlayers; l++) {
      LearnerGemm g = gemm(n, l);
      g.out = p->net[n].Z[l];
      const dim3 grid(tiles(g.rows), tiles(g.n));
      if (l) hipLaunchKernelGGL((learner_gemm_kernel<LRN_FWD, LRN_SRC_SWISH>), grid, blk, 0, st, g);
      else hipLaunchKernelGGL((learner_gemm_kernel<LRN_FWD, LRN_SRC_OBS>), grid, blk, 0, st, g);
    }
  // the loss and its derivative at the two heads
  const LearnerNet &P = p->net[0], &V = p->net[1];
  hipLaunchKernelGGL(learner_gae_kernel, dim3(1), blk, 0, st, V.Z[V.nlayers - 1], rewards, termination, truncation, idx, T, mb, B, c.discounting,
                     c.gae_lambda, c.reward_scaling, c.normalize_advantage, p->vs, p->adv, p->stats);
  hipLaunchKernelGGL(learner_loss_kernel, dim3((unsigned)((rows_of[1] + 3) / 4)), blk, 0, st, P.Z[P.nlayers - 1], V.Z[V.nlayers - 1], u, logp, entropy_noise,
                     idx, p->vs, p->adv, p->stats, T, mb, B, c.act_dim, c.clipping_epsilon, c.entropy_cost, P.dZ[P.nlayers - 1], V.dZ[V.nlayers - 1],
                     p->rowloss);
  hipLaunchKernelGGL(learner_loss_sum_kernel, dim3(1), blk, 0, st, p->rowloss, rows_of[0], c.entropy_cost, loss_sums);
  // backward: [dW_l; db_l] = [in_l 1]^T dZ_l in S splits, dZ_{l-1} = (dZ_l W_l^T) swish'(Z_{l-1})
  for (int n = 0; n < 2; n++)
    for (int l = p->net[n].nlayers - 1; l >= 0; l--) {
      LearnerGemm g = gemm(n, l);
      g.out = p->partial + p->net[n].off[l];
      const dim3 grid(tiles(g.kdim + 1), tiles(g.n), (unsigned)S);
      if (l) hipLaunchKernelGGL((learner_gemm_kernel<LRN_DW, LRN_SRC_SWISH>), grid, blk, 0, st, g);
      else hipLaunchKernelGGL((learner_gemm_kernel<LRN_DW, LRN_SRC_OBS>), grid, blk, 0, st, g);
      if (l) {
        g.out = p->net[n].dZ[l - 1];
        hipLaunchKernelGGL((learner_gemm_kernel<LRN_DX, LRN_SRC_SWISH>), dim3(tiles(g.rows), tiles(g.kdim)), blk, 0, st, g);
      }
    }
  p->steps++;
  const double bc1 = 1.0 - std::pow(c.beta1, (double)p->steps), bc2 = 1.0 - std::pow(c.beta2, (double)p->steps);
  hipLaunchKernelGGL(learner_adam_kernel, dim3((unsigned)((p->total + 255) / 256)), blk, 0, st, p->total, S, p->partial, p->flat, p->flat + p->total,
                     p->flat + 2 * p->total, p->flat + 3 * p->total, (float)c.beta1, (float)(1.0 - c.beta1), (float)c.beta2, (float)(1.0 - c.beta2),
                     (float)(c.learning_rate / bc1), (float)std::sqrt(bc2), (float)c.adam_eps);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

#endif  // MYO_HOST_LEARNER_H
