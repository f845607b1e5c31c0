// myo_kernels_aux.h -- small kernels: placement hint, random actions, link recomposition, and the two kernels every task body runs in.
// Part of the single translation unit myo_hip.hip (included there, in this order); not a stand-alone header.
#ifndef MYO_KERNELS_AUX_H
#define MYO_KERNELS_AUX_H

// Placement hint for the wave-per-env kernel.  All B envs are co-resident (4 waves per SIMD), so a launch ends when the
// slowest SIMD ends; envs differ ~2x in work (contacts, Newton iterations) and that work is strongly correlated from one
// env step to the next.  Sort envs by last step's cost (counting sort, one workgroup) and deal them out so that the waves
// that land on one SIMD come from different cost quartiles (snake order over `nslot` = B/4 slots).  Dispatch order is not
// a contract: this only ever changes speed.
__global__ void __launch_bounds__(1024) balance_kernel(const int* __restrict__ diag, int B, int* __restrict__ order, int nslot, int prio_mode) {
  __shared__ int hist[256], start[256];
  __shared__ int cmax_s;
  const int t = threadIdx.x;
  if (t < 256) hist[t] = 0;
  if (t == 0) cmax_s = 1;
  __syncthreads();
  // costs of this thread's envs: read once (the first four stay in registers, a launch of 4096 envs has exactly four per thread)
  int c4[4] = {0, 0, 0, 0};
  int cm = 1;
#pragma unroll
  for (int k = 0; k < 4; k++) { const int e = t + 1024 * k; if (e < B) { c4[k] = diag[(size_t)e * 8 + 3]; cm = max(cm, c4[k]); } }
  for (int e = t + 4096; e < B; e += 1024) cm = max(cm, diag[(size_t)e * 8 + 3]);
  for (int off = 32; off > 0; off >>= 1) cm = max(cm, __shfl_xor(cm, off));
  if ((t & 63) == 0) atomicMax(&cmax_s, cm);
  __syncthreads();
  const float sc = 255.0f / (float)cmax_s;
#define BUCKET(c) (255 - min(255, (int)(sc * (float)(c))))     /* bucket 0 = heaviest */
#pragma unroll
  for (int k = 0; k < 4; k++) if (t + 1024 * k < B) atomicAdd(&hist[BUCKET(c4[k])], 1);
  for (int e = t + 4096; e < B; e += 1024) atomicAdd(&hist[BUCKET(diag[(size_t)e * 8 + 3])], 1);
  __syncthreads();
  if (t < 64) {   // exclusive prefix sum of the 256 bins by one wave: 4 bins per lane, then a wave scan of the lane totals
    const int h0 = hist[4 * t], h1 = hist[4 * t + 1], h2 = hist[4 * t + 2], h3 = hist[4 * t + 3];
    int tot = h0 + h1 + h2 + h3, inc = tot;
    for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(inc, off); if (t >= off) inc += v; }
    const int base = inc - tot;
    start[4 * t] = base; start[4 * t + 1] = base + h0; start[4 * t + 2] = base + h0 + h1; start[4 * t + 3] = base + h0 + h1 + h2;
  }
  __syncthreads();
  auto place = [&](int e, int c) {
    const int r = atomicAdd(&start[BUCKET(c)], 1);          // rank by descending cost (ties in arbitrary order)
    const int q = r / nslot, i = r - q * nslot;
    const int wg = q * nslot + ((q & 1) ? nslot - 1 - i : i);   // snake: slot i gets ranks i, 2*nslot-1-i, 2*nslot+i, ...
    const int pr = prio_mode == 2 ? (q < 3 ? 3 - q : 0) : (prio_mode == 1 ? (q == 0 ? 1 : 0) : (prio_mode == 3 ? (q < 2 ? 1 : 0) : 0));
    order[wg < B ? wg : r] = e | (pr << 28);                 // env id + issue priority of its cost quartile
  };
#pragma unroll
  for (int k = 0; k < 4; k++) if (t + 1024 * k < B) place(t + 1024 * k, c4[k]);
  for (int e = t + 4096; e < B; e += 1024) place(e, diag[(size_t)e * 8 + 3]);
#undef BUCKET
}

__global__ void random_action_kernel(float* action, int B, int nu, uint64_t seed, uint64_t step, int env_offset) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)B * nu) return;
  size_t e = i / nu, k = i % nu;
  action[i] = 2.0f * rng_u<RS_RANDOM_ACTION>(seed, (uint64_t)(e + env_offset), k, step) - 1.0f;
}

// per-env body masses (MYO_F_BODYMASS): link mass, COM and inertia about the COM of every link of every env from its bodies' masses, the
// recomposition lowering.py does at compile time (parallel-axis theorem over the bodies welded into the link).  Member m of link l (CSR
// adr[l] .. adr[l+1]) is body body[m] with its COM (3), its inertia (6, xx yy zz xy xz yz, about its COM) in the link frame and its compiled
// float64 mass, tab[10 m ..].  A body whose float32 entry still equals its compiled mass rounded to float32 counts with the float64 mass, so
// that unchanged bodies contribute exactly what lowering summed (an unchanged link gets the model's link tables to the last bit).
// One thread per (env, link), float64 arithmetic; run once per step launch, before the step kernel
__global__ void __launch_bounds__(256) link_compose_kernel(DevBatch Bt, int nl, const int* __restrict__ adr, const int* __restrict__ body,
                                                          const double* __restrict__ tab) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Bt.B * nl) return;
  const int e = t / nl, l = t - e * nl;
  const float* bm = Bt.bmass + (size_t)e * Bt.nbody;
  double mass = 0, mc[3] = {0, 0, 0};
  auto mass_of = [&](int k) { const float f = bm[body[k]]; const double m0 = tab[10 * k + 9]; return f == (float)m0 ? m0 : (double)f; };
  for (int k = adr[l]; k < adr[l + 1]; k++) {
    const double mb = mass_of(k);
    mass += mb;
    for (int j = 0; j < 3; j++) mc[j] += mb * tab[10 * k + j];
  }
  const double inv = mass > 0 ? 1.0 / mass : 0.0;
  const double com[3] = {mc[0] * inv, mc[1] * inv, mc[2] * inv};
  double I[6] = {0, 0, 0, 0, 0, 0};
  for (int k = adr[l]; k < adr[l + 1]; k++) {
    const double mb = mass_of(k);
    const double* c = tab + 10 * k;
    const double d[3] = {c[0] - com[0], c[1] - com[1], c[2] - com[2]}, dd = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    I[0] += c[3] + mb * (dd - d[0] * d[0]);
    I[1] += c[4] + mb * (dd - d[1] * d[1]);
    I[2] += c[5] + mb * (dd - d[2] * d[2]);
    I[3] += c[6] - mb * d[0] * d[1];
    I[4] += c[7] - mb * d[0] * d[2];
    I[5] += c[8] - mb * d[1] * d[2];
  }
  float* o = Bt.linkc + (size_t)t * 10;
  o[0] = (float)mass;
  for (int j = 0; j < 3; j++) o[1 + j] = (float)com[j];
  for (int j = 0; j < 6; j++) o[4 + j] = (float)I[j];
}

// A task hands its observation to the two kernels below as a struct with one static function, Task::obs(M, Bt, T, K, seed, obs_only, e, lane),
// that wraps its *_obs_body (StateObs / TrackObs take the body as a template argument, so a kernel's symbol carries its task's name).  K (the
// track record) and seed (the seed of the last reset) are read by the classic MyoDM flavour only
template <void (*Body)(const DevModel&, const DevBatch&, const TaskDev&, int, int, int)>
struct StateObs {   // a body that reads the batch state alone
  static __device__ __forceinline__ void obs(const DevModel& M, const DevBatch& Bt, const TaskDev& T, const DevTrack*, uint64_t, int obs_only, int e, int lane) {
    Body(M, Bt, T, obs_only, e, lane);
  }
};
template <void (*Body)(const DevModel&, const DevBatch&, const TaskDev&, const DevTrack&, uint64_t, int, int, int)>
struct TrackObs {   // a body that also reads the track record and the seed of the last reset (classic MyoDM)
  static __device__ __forceinline__ void obs(const DevModel& M, const DevBatch& Bt, const TaskDev& T, const DevTrack* K, uint64_t seed, int obs_only, int e, int lane) {
    Body(M, Bt, T, *K, seed, obs_only, e, lane);
  }
};
template <class Task>
__global__ void __launch_bounds__(64) task_obs_kernel(DevModel M, DevBatch Bt, TaskDev T, const DevTrack* K, uint64_t seed, int obs_only, int reset_only) {
  const int e = blockIdx.x;
  if (e >= Bt.B) return;
  if (reset_only && Bt.elapsed[e] != 0) return;    // refresh only the rows of envs an auto-reset just touched
  Task::obs(M, Bt, T, K, seed, obs_only, e, threadIdx.x);
}
// observation / reward / done of the stepped state, gym TimeLimit + done auto-reset, and the first observation of the new episode for the
// envs that were reset: the three launches of the per-step epilogue (task_obs_kernel, reset_kernel, task_obs_kernel(reset_only)) in one --
// on the critical path between two step kernels every launch costs a few microseconds of dispatch gap.  The reset reads its copy of the batch and
// task records through R, after the test: as kernel arguments their loads were issued on every env's path and spilled scalar registers there
template <class Task>
__global__ void __launch_bounds__(64) task_post_kernel(DevModel M, DevBatch Bt, TaskDev T, const DevTrack* K, const ResetArgs* __restrict__ R, int nq,
                                                       const float* qpos0, uint64_t seed, int env_offset, int auto_max) {
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= Bt.B) return;
  Task::obs(M, Bt, T, K, seed, 0, e, lane);
  __syncthreads();                       // reward / done of this env written (lane 0) before every lane tests them
  if (!(Bt.done[e] > 0.f || Bt.elapsed[e] >= auto_max)) return;   // (auto_max > 0: the epilogue is launched for an auto-reset only)
  reset_body<false>(R->Bt, R->T, nq, M.nv, M.nu, qpos0, nullptr, seed, env_offset, auto_max, e, lane);
  __syncthreads();                       // the new state rows (and what the reset drew for the task) are complete before they are read back
  Task::obs(M, Bt, T, K, seed, 1, e, lane);
}

#endif  // MYO_KERNELS_AUX_H
