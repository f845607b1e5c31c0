// myo_kernels_learner.h -- one PPO minibatch SGD step on the device (myo_ppo_learner_step, include/myo_hip_ppo.h): the two MLPs' forward
// and backward passes on the FP32 matrix cores, GAE, the loss and its derivative at the heads, Adam.
// Part of the single translation unit myo_hip.hip (included there after myo_kernels_ppo.h); not a stand-alone header.
//
// Rows.  Row r = t * mb + i of a minibatch is env idx[i] at time t; the value network runs on all (T + 1) * mb rows (the last mb are the
// bootstrap), the policy on the first T * mb.  Every layer keeps its pre-activation Z [rows][width]; the input of layer l > 0 is
// swish(Z_{l-1}), formed when a GEMM loads it, and the input of layer 0 is (obs - mean) / std, gathered through idx when a GEMM loads it.
// Parameters.  All tensors of both networks lie in one flat array, layer by layer, each kernel [in][out] followed by its bias: kernel and
// bias together are the [in + 1][out] matrix of a layer whose input carries a constant 1 as its last feature, which is how the dW kernel
// gets db (the row `in` of X^T dZ with that 1 appended).  Gradients, Adam's moments and the split partial sums use the same offsets.
// Order of every sum (so that equal inputs give equal bits): an MFMA tile sums its k index in increasing order, one fmaf per product; dW
// splits the rows into S chunks (S is a function of the row count alone), each chunk is one such chain, and learner_adam_kernel adds the
// S partial sums in increasing chunk order; the block reductions below are a strided partial sum per thread and a halving tree in LDS.
// No floating-point atomics anywhere.
#ifndef MYO_KERNELS_LEARNER_H
#define MYO_KERNELS_LEARNER_H

// 0: the build without matrix-core instructions (the MYO_LDL_MFMA=0 A/B build of myo_ldl_mfma.h) forms the same sums on the VALU
#ifndef MYO_LEARNER_MFMA
#define MYO_LEARNER_MFMA MYO_LDL_MFMA
#endif

#define LRN_TILE 64         // block tile: 64 x 64 outputs, one 32 x 32 MFMA tile per wave (2 x 2 waves)
#define LRN_TK 64            // k extent of one LDS stage
#define LRN_NLD (LRN_TK * LRN_TILE / 256)    // values of A, and of B, that one thread loads per stage
#define LRN_LD (LRN_TILE + 1)                // odd row pitch: the k-fastest stores (lane = k, one column) hit 64 different banks
#define LRN_CHUNK 256        // rows per dW split (more when that would make more than LRN_MAXSPLIT splits)
#define LRN_MAXSPLIT 32

enum { LRN_FWD = 0, LRN_DX = 1, LRN_DW = 2 };             // Z = in W + b;  dZprev = (dZ W^T) swish'(Zprev);  [dW; db] = [in 1]^T dZ
enum { LRN_SRC_SWISH = 0, LRN_SRC_OBS = 1 };              // a layer's input: swish(X) or the gathered, normalised observations

struct LearnerGemm {
  const float* X;            // SRC_SWISH: the previous layer's Z [rows][kdim]
  const float* W;            // this layer's kernel [kdim][n]; its bias follows at W + kdim * n
  const float* dZ;           // DX, DW: [rows][n]
  const float* Zprev;        // DX: the previous layer's Z [rows][kdim]
  float* out;                // FWD: Z [rows][n];  DX: dZprev [rows][kdim];  DW: partial sums, split s at out + s * split_stride, [kdim + 1][n]
  const float* obs;          // SRC_OBS: [T + 1][B][kdim]
  const int64_t* idx;
  const float* mean;
  const float* std;
  int rows, kdim, n, mb, B, chunk;
  size_t split_stride;
};

__device__ __forceinline__ float learner_sigmoid(float z) { return 1.0f / (1.0f + expf(-z)); }

// feature c < kdim of row r < rows of a layer's input
template <int SRC> __device__ __forceinline__ float learner_in(const LearnerGemm& g, int r, int c) {
  if (SRC == LRN_SRC_OBS) {
    const int t = r / g.mb, i = r - t * g.mb;
    return (g.obs[((size_t)t * g.B + (size_t)g.idx[i]) * g.kdim + c] - g.mean[c]) / g.std[c];
  }
  const float z = g.X[(size_t)r * g.kdim + c];
  return z * learner_sigmoid(z);
}

// One thread's share of a stage, from global memory into registers: element q of `ra` is As[kk][i] and of `rb` is Bs[kk][j] with
// (kk, i or j) = (tid & 63, (tid >> 6) + 4 q) where k is fastest in memory and ((tid >> 6) + 4 q, tid & 63) where the tile index is, so
// that a wave reads 256 consecutive bytes either way.  Zero outside the matrices, which is all that ragged shapes need.
//   FWD: M = rows, N = n, K = kdim       A = in (k fastest in memory)     B = W
//   DX:  M = rows, N = kdim, K = n       A = dZ (k fastest)               B[k][j] = W[j][k] (k fastest)
//   DW:  M = kdim + 1, N = n, K = the rows of split blockIdx.z            A[i][k] = in[k][i], 1 for i = kdim (i fastest)   B = dZ
template <int FORM, int SRC> __device__ __forceinline__ void learner_fetch(const LearnerGemm& g, int tid, int m0, int n0, int M, int N, int kb, int k1,
                                                                           float (&ra)[LRN_NLD], float (&rb)[LRN_NLD]) {
  const int lo = tid & 63, hi = tid >> 6;
#pragma unroll
  for (int q = 0; q < LRN_NLD; q++) {
    float v = 0.f;
    if (FORM == LRN_DW) {
      const int c = m0 + lo, r = kb + hi + 4 * q;
      if (r < k1) { if (c < g.kdim) v = learner_in<SRC>(g, r, c); else if (c == g.kdim) v = 1.0f; }
    } else {
      const int k = kb + lo, r = m0 + hi + 4 * q;
      if (r < M && k < k1) v = FORM == LRN_FWD ? learner_in<SRC>(g, r, k) : g.dZ[(size_t)r * g.n + k];
    }
    ra[q] = v;
  }
#pragma unroll
  for (int q = 0; q < LRN_NLD; q++) {
    float v = 0.f;
    if (FORM == LRN_DX) {
      const int k = kb + lo, c = n0 + hi + 4 * q;
      if (c < N && k < k1) v = g.W[(size_t)c * g.n + k];
    } else {
      const int c = n0 + lo, k = kb + hi + 4 * q;
      if (c < N && k < k1) v = (FORM == LRN_FWD ? g.W : g.dZ)[(size_t)k * g.n + c];
    }
    rb[q] = v;
  }
}

// C[M][N] = A[M][K] B[K][N] for the three products of a layer, 256 threads per 64 x 64 tile of C.  Per stage of LRN_TK k values the block
// writes As[k][i] and Bs[k][j] from the registers learner_fetch filled, fetches the next stage's share into those registers (the loads
// are in flight while the matrix core works), and each wave runs LRN_TK / 2 MFMAs 32x32x2 on its quarter: operand lane l holds
// A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], accumulator register q of lane l is C[8 (q / 4) + 4 (l >> 5) + q % 4][l & 31].
// A wave whose quarter lies outside C skips the MFMAs (but not the barriers).
template <int FORM, int SRC> __global__ void __launch_bounds__(256) learner_gemm_kernel(LearnerGemm g) {
  __shared__ float As[LRN_TK][LRN_LD], Bs[LRN_TK][LRN_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#if MYO_POISON
  for (int i = tid; i < LRN_TK * LRN_LD; i += 256) { (&As[0][0])[i] = __int_as_float(MYO_POISON_BITS); (&Bs[0][0])[i] = __int_as_float(MYO_POISON_BITS); }
  __syncthreads();
#endif
  const int M = FORM == LRN_DW ? g.kdim + 1 : g.rows, N = FORM == LRN_DX ? g.kdim : g.n;
  const int k0 = FORM == LRN_DW ? min(g.rows, (int)blockIdx.z * g.chunk) : 0;
  const int k1 = FORM == LRN_DW ? min(g.rows, k0 + g.chunk) : FORM == LRN_DX ? g.n : g.kdim;
  const int m0 = blockIdx.x * LRN_TILE, n0 = blockIdx.y * LRN_TILE;
  const int wm = 32 * (wave >> 1), wn = 32 * (wave & 1);
  const bool live = m0 + wm < M && n0 + wn < N;
  const bool a_k_fastest = FORM != LRN_DW, b_k_fastest = FORM == LRN_DX;
  myo_v16f acc;
#pragma unroll
  for (int q = 0; q < 16; q++) acc[q] = 0.f;
  float ra[LRN_NLD], rb[LRN_NLD];
  if (k0 < k1) learner_fetch<FORM, SRC>(g, tid, m0, n0, M, N, k0, k1, ra, rb);
  for (int kb = k0; kb < k1; kb += LRN_TK) {
#pragma unroll
    for (int q = 0; q < LRN_NLD; q++) {
      const int lo = tid & 63, hi = (tid >> 6) + 4 * q;
      if (a_k_fastest) As[lo][hi] = ra[q]; else As[hi][lo] = ra[q];
      if (b_k_fastest) Bs[lo][hi] = rb[q]; else Bs[hi][lo] = rb[q];
    }
    __syncthreads();
    if (kb + LRN_TK < k1) learner_fetch<FORM, SRC>(g, tid, m0, n0, M, N, kb + LRN_TK, k1, ra, rb);
    if (live) {
#if MYO_LEARNER_MFMA
#pragma unroll
      for (int kk = 0; kk < LRN_TK; kk += 2)
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(As[kk + (lane >> 5)][wm + (lane & 31)], Bs[kk + (lane >> 5)][wn + (lane & 31)], acc, 0, 0, 0);
#else
      for (int kk = 0; kk < LRN_TK; kk++) {                 // the same k-ordered fmaf chains, one per accumulator entry, on the VALU
        const float b = Bs[kk][wn + (lane & 31)];
#pragma unroll
        for (int q = 0; q < 16; q++) acc[q] = fmaf(As[kk][wm + 8 * (q / 4) + 4 * (lane >> 5) + q % 4], b, acc[q]);
      }
#endif
    }
    __syncthreads();
  }
  if (!live) return;
  const int col = n0 + wn + (lane & 31);
  if (col >= N) return;
  const float bias = FORM == LRN_FWD ? g.W[(size_t)g.kdim * g.n + col] : 0.f;
  float* out = FORM == LRN_DW ? g.out + (size_t)blockIdx.z * g.split_stride : g.out;
#pragma unroll
  for (int q = 0; q < 16; q++) {
    const int row = m0 + wm + 8 * (q / 4) + 4 * (lane >> 5) + q % 4;
    if (row >= M) continue;
    const size_t o = (size_t)row * N + col;
    if (FORM == LRN_FWD) out[o] = acc[q] + bias;
    else if (FORM == LRN_DW) out[o] = acc[q];               // row kdim is the bias, which follows the kernel
    else {
      const float z = g.Zprev[o], s = learner_sigmoid(z);
      out[o] = acc[q] * (s * (1.0f + z * (1.0f - s)));      // d swish(z) / dz
    }
  }
}

// sum of the 256 threads' values in thread order pairs (a halving tree): the same value in every thread
__device__ __forceinline__ float learner_block_sum(float x, float* red, int tid) {
  __syncthreads();                                          // the previous use of red is over
  red[tid] = x;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  return red[0];
}

// GAE (the recurrence of ppo_gae_kernel) on the minibatch's columns, then mean and std + 1e-8 of the T * mb advantages.  One block: thread
// i walks column i backwards, eight time steps' loads at a time so that the loop waits for memory T / 8 times, not T times.
// V [(T + 1) * mb] is the value head's output; rewards / termination / truncation are [T][B], read through idx.
// stats[0] = mean, stats[1] = std + 1e-8 (0 and 1 without normalisation): the loss kernel forms (adv - stats[0]) / stats[1].
__global__ void __launch_bounds__(256) learner_gae_kernel(const float* __restrict__ V, const float* __restrict__ rewards, const float* __restrict__ termination,
                                                          const float* __restrict__ truncation, const int64_t* __restrict__ idx, int T, int mb, int B,
                                                          float discount, float lambda, float reward_scaling, int normalize,
                                                          float* __restrict__ vs_out, float* __restrict__ adv_out, float* __restrict__ stats) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
#if MYO_POISON
  red[tid] = __int_as_float(MYO_POISON_BITS);
  __syncthreads();
#endif
  for (int i = tid; i < mb; i += 256) {
    const size_t e = (size_t)idx[i];
    float v_next = V[(size_t)T * mb + i], vs_next = v_next, acc = 0.f;
    for (int t1 = T; t1 > 0; t1 -= 8) {
      float r[8], v[8], te[8], tr[8];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int t = t1 - 1 - k;
        if (t >= 0) {
          const size_t s = (size_t)t * B + e;
          r[k] = rewards[s] * reward_scaling; te[k] = termination[s]; tr[k] = truncation[s]; v[k] = V[(size_t)t * mb + i];
        }
      }
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const int t = t1 - 1 - k;
        if (t >= 0) {
          const float cont = discount * (1.0f - te[k]), mask = 1.0f - tr[k];
          const float delta = (r[k] + cont * v_next - v[k]) * mask;
          acc = delta + cont * mask * lambda * acc;
          const float vs = acc + v[k];
          vs_out[(size_t)t * mb + i] = vs;
          adv_out[(size_t)t * mb + i] = (r[k] + cont * vs_next - v[k]) * mask;
          v_next = v[k];
          vs_next = vs;
        }
      }
    }
  }
  if (!normalize) {
    if (tid == 0) { stats[0] = 0.f; stats[1] = 1.0f; }
    return;
  }
  __threadfence_block();
  __syncthreads();                                          // the block's own stores to adv_out are visible to all of its threads
  const int n = T * mb;
  float s = 0.f;
  for (int k = tid; k < n; k += 256) s += adv_out[k];
  const float mean = learner_block_sum(s, red, tid) / (float)n;
  float q = 0.f;
  for (int k = tid; k < n; k += 256) { const float d = adv_out[k] - mean; q += d * d; }
  const float var = learner_block_sum(q, red, tid) / (float)n;
  if (tid == 0) { stats[0] = mean; stats[1] = sqrtf(var) + 1e-8f; }
}

__device__ __forceinline__ float learner_log_det_tanh(float u) { return 2.0f * (0.6931471805599453f - u - softplus_f(-2.0f * u)); }

// The loss at the heads and its derivative with respect to the heads' outputs.  One wavefront per row r of the (T + 1) * mb; lanes stride
// over the act_dim actions and a __shfl_xor butterfly sums the row's log-probability and entropy (every lane ends with the same bits).
//   head [T mb][2 A] = (loc, raw);  dhead = d(policy + entropy loss) / d head;  dV [(T + 1) mb] = d(value loss) / dV, 0 on the bootstrap rows
//   rowloss [T mb][3] = min(rho A, clip(rho) A), (V - vs)^2, the entropy estimate: learner_loss_sum_kernel adds them up
// d log pi / d loc = z / scale, d log pi / d scale = (z^2 - 1) / scale with z = (u - loc) / scale; the surrogate passes A rho to log pi where
// rho is inside the clip range or rho A is the smaller branch, else nothing; the entropy estimate at u_e = loc + scale noise has
// d / d loc = -2 tanh(u_e) and d / d scale = 1 / scale - 2 tanh(u_e) noise; d scale / d raw = sigmoid(raw).
__global__ void __launch_bounds__(256) learner_loss_kernel(const float* __restrict__ head, const float* __restrict__ V, const float* __restrict__ u,
                                                           const float* __restrict__ logp_b, const float* __restrict__ noise, const int64_t* __restrict__ idx,
                                                           const float* __restrict__ vs, const float* __restrict__ adv, const float* __restrict__ stats,
                                                           int T, int mb, int B, int A, float clip_eps, float entropy_cost,
                                                           float* __restrict__ dhead, float* __restrict__ dV, float* __restrict__ rowloss) {
  const int lane = threadIdx.x & 63, r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n = T * mb;
  if (r >= n + mb) return;                                  // uniform over the wave
  if (r >= n) { if (lane == 0) dV[r] = 0.f; return; }
  const int t = r / mb, i = r - t * mb;
  const size_t e = (size_t)t * B + (size_t)idx[i];
  const float* h = head + (size_t)r * 2 * A;
  const float* ur = u + e * A;
  const float* nr = noise + (size_t)r * A;
  float lp = 0.f, ent = 0.f;
  for (int j = lane; j < A; j += 64) {
    const float loc = h[j], scale = softplus_f(h[A + j]) + 0.001f, uu = ur[j];
    const float z = (uu - loc) / scale, ls = logf(scale);
    lp += -0.5f * z * z - ls - 0.9189385332046727f - learner_log_det_tanh(uu);
    ent += 0.5f + 0.9189385332046727f + ls + learner_log_det_tanh(loc + scale * nr[j]);
  }
  for (int off = 32; off > 0; off >>= 1) { lp += __shfl_xor(lp, off); ent += __shfl_xor(ent, off); }
  const float inv_n = 1.0f / (float)n;
  const float a = (adv[r] - stats[0]) / stats[1];
  const float rho = expf(lp - logp_b[e]);
  const float lo = 1.0f - clip_eps, hi = 1.0f + clip_eps;
  const float s1 = rho * a, s2 = fminf(fmaxf(rho, lo), hi) * a;
  const float g_rho = (rho >= lo && rho <= hi) || s1 < s2 ? a : 0.f;
  const float d_lp = -g_rho * rho * inv_n, ce = -entropy_cost * inv_n;
  float* dh = dhead + (size_t)r * 2 * A;
  for (int j = lane; j < A; j += 64) {
    const float loc = h[j], raw = h[A + j], scale = softplus_f(raw) + 0.001f, uu = ur[j], eps = nr[j];
    const float z = (uu - loc) / scale, th = tanhf(loc + scale * eps);
    dh[j] = d_lp * (z / scale) + ce * (-2.0f * th);
    dh[A + j] = (d_lp * ((z * z - 1.0f) / scale) + ce * (1.0f / scale - 2.0f * th * eps)) * learner_sigmoid(raw);
  }
  if (lane == 0) {
    const float verr = V[r] - vs[r];
    dV[r] = 0.5f * verr * inv_n;
    rowloss[(size_t)r * 3] = fminf(s1, s2);
    rowloss[(size_t)r * 3 + 1] = verr * verr;
    rowloss[(size_t)r * 3 + 2] = ent;
  }
}

// the three loss terms of the step from rowloss [n][3]; thread 0 adds them to loss_sums (nothing is written when it is NULL)
__global__ void __launch_bounds__(256) learner_loss_sum_kernel(const float* __restrict__ rowloss, int n, float entropy_cost, float* loss_sums) {
  __shared__ float red[256];
  const int tid = threadIdx.x;
#if MYO_POISON
  red[tid] = __int_as_float(MYO_POISON_BITS);
  __syncthreads();
#endif
  float s[3] = {0.f, 0.f, 0.f};
  for (int k = tid; k < n; k += 256)
    for (int c = 0; c < 3; c++) s[c] += rowloss[(size_t)k * 3 + c];
  for (int c = 0; c < 3; c++) s[c] = learner_block_sum(s[c], red, tid);
  if (tid == 0 && loss_sums) {
    loss_sums[0] += -s[0] / (float)n;
    loss_sums[1] += 0.25f * s[1] / (float)n;
    loss_sums[2] += -entropy_cost * s[2] / (float)n;
  }
}

// gradient = the S partial sums of the dW launches in chunk order (kept for myo_ppo_learner_tensor), then torch.optim.Adam's update:
//   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2;  p -= step (m / (sqrt(v) / bc2_sqrt + eps)),  step = lr / (1 - b1^t), bc2_sqrt = sqrt(1 - b2^t)
__global__ void __launch_bounds__(256) learner_adam_kernel(size_t total, int S, const float* __restrict__ partial, float* __restrict__ param,
                                                           float* __restrict__ grad, float* __restrict__ m, float* __restrict__ v, float b1, float omb1,
                                                           float b2, float omb2, float step, float bc2_sqrt, float eps) {
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (k >= total) return;
  float g = partial[k];
  for (int s = 1; s < S; s++) g += partial[(size_t)s * total + k];
  grad[k] = g;
  const float mk = b1 * m[k] + omb1 * g, vk = b2 * v[k] + omb2 * (g * g);
  m[k] = mk;
  v[k] = vk;
  param[k] -= step * (mk / (sqrtf(vk) / bc2_sqrt + eps));
}

#endif
