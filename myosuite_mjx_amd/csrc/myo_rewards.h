// myo_rewards.h -- reward-term rows and episode statistics (include/myo_hip_rewards.h): the lookup of a task's columns, the walk task's
// term kernel, the episode-statistics kernel and the host entry points.  The other tasks write their rows in their own observation kernels
// (rwd_row, myo_common.h).  Included by myo_hip.hip after myo_host.h, before the task files (walk_configure reads rwd_cols).
#ifndef MYO_REWARDS_H
#define MYO_REWARDS_H

// ---- columns: the keys of the reference's rwd_dict per env class, in its order; a task's names live in its hook record (myo_task_<name>.h).
// No task, and the MyoDM track task (its terms are MYO_F_METRICS), have none
static RwdCols rwd_cols(int task) {
  const TaskHooks* hooks = task_hooks(task);
  return hooks ? hooks->rwd : RwdCols{nullptr, 0};
}

// ---- walk task: the step kernel's fused pass keeps its fixed-weight sum; with the term row on, this kernel follows every launch of it
// that wrote MYO_F_REWARD and restates the terms from what that pass stored -- the observation row (qpos[2:], COM velocity, feet heights, COM
// height, phase: the float32 values the fused pass computed its own terms from) -- plus the activations for act_mag.  One wave per env
__global__ void __launch_bounds__(64) walk_terms_kernel(DevBatch Bt, const DevWalk* __restrict__ wk, int nq, int nv, int nu, int na) {
  const int e = blockIdx.x, lane = threadIdx.x;
  if (e >= Bt.B) return;
  const float* a = Bt.act + (size_t)e * nu;
  float act2 = 0.f;
  for (int i = lane; i < nu; i += 64) { const float ai = a[i]; act2 += ai * ai; }
  const float act_mag = sqrtf(wave_sum(act2)) / (float)(na > 0 ? na : 1);   // walk_v0.py:291-295 (0 without muscles: act stays zero)
  if (lane != 0) return;
  const WalkRow R{nq, nv, nu};
  const float* o = Bt.obs + (size_t)e * wk->obs_dim;
  auto qp = [&](int i) { return o[R.qpos_without_xy.at + i - 2]; };    // qpos[i], i >= 2
  const float cvx = o[R.com_vel.at], cvy = o[R.com_vel.at + 1], fl = o[R.feet_heights.at], fr = o[R.feet_heights.at + 1], height = o[R.height.at],
              phase = o[R.phase_var.at];
  const float q[4] = {qp(3), qp(4), qp(5), qp(6)};
  const float dvy = wk->target_y_vel - cvy, dvx = wk->target_x_vel - cvx;
  const float vel_reward = expf(-dvy * dvy) + expf(-dvx * dvx);
  const float d0 = 0.8f * cosf(phase * 6.283185307179586f + 3.141592653589793f) - qp(wk->qadr_hfl);
  const float d1 = 0.8f * cosf(phase * 6.283185307179586f) - qp(wk->qadr_hfr);
  const float cyclic = sqrtf(d0 * d0 + d1 * d1);
  const float dq[4] = {q[0] - wk->target_rot[0], q[1] - wk->target_rot[1], q[2] - wk->target_rot[2], q[3] - wk->target_rot[3]};
  const float ref_rot = expf(-5.0f * sqrtf(dq[0] * dq[0] + dq[1] * dq[1] + dq[2] * dq[2] + dq[3] * dq[3]));
  const float mag = 0.25f * (fabsf(qp(wk->qadr_ja[0])) + fabsf(qp(wk->qadr_ja[1])) + fabsf(qp(wk->qadr_ja[2])) + fabsf(qp(wk->qadr_ja[3])));
  const float ja = expf(-5.0f * mag);
  const float r00 = 1.0f - 2.0f * (q[2] * q[2] + q[3] * q[3]) / (q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  float done = (height < wk->min_height || fabsf(r00) > wk->max_rot) ? 1.f : 0.f;
  if (wk->knee_height > 0.f && height - 0.5f * (fl + fr) < wk->knee_height) done = 1.f;
  rwd_row(Bt, e, {vel_reward, cyclic, ref_rot, ja, act_mag, vel_reward, vel_reward >= 1.0f ? 1.f : 0.f, done});
}

// ---- episode statistics: one thread per env, once per env step after the observation pass and before the auto-reset.  The running row
// gains (dense, sparse, 1, solved); an env whose episode ends by reset_kernel's rule hands its row to `last`, raises its byte and starts anew
__global__ void __launch_bounds__(256) episode_stats_kernel(DevBatch Bt, float4* __restrict__ run, float4* __restrict__ last, uint8_t* __restrict__ finished,
                                                           int* __restrict__ count, int max_steps) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= Bt.B) return;
  const float* r = Bt.rwd + (size_t)e * Bt.rwd_n;
  float4 s = run[e];
  s.x += r[Bt.rwd_n - 1]; s.y += r[Bt.rwd_n - 4]; s.z += 1.f; s.w += Bt.solved[e];
  const bool end = Bt.done[e] > 0.f || Bt.elapsed[e] >= max_steps;
  if (end) { last[e] = s; count[e] += 1; s = make_float4(0.f, 0.f, 0.f, 0.f); }
  finished[e] = end ? 1 : 0;
  run[e] = s;
}

// ---- host
static int rewards_enable(myo_batch* b, const float* w, int nw, int mode) {
  const RwdCols c = rwd_cols(b->task.task);
  if (!c.n) return fail(MYO_E_UNSUPPORTED, "reward terms: no task with a term row is configured (the MyoDM track task reports MYO_F_METRICS)");
  if (!w || nw != c.n - 1) return fail(MYO_E_ARG, "reward terms: one weight per column except dense");
  if (mode != MYO_RWD_DENSE && mode != MYO_RWD_SPARSE) return fail(MYO_E_ARG, "reward terms: mode must be MYO_RWD_DENSE or MYO_RWD_SPARSE");
  for (int k = 0; k < nw; k++) if (!std::isfinite(w[k])) return fail(MYO_E_ARG, "reward terms: weights must be finite");
  if (b->task.task == MYO_TASK_WALK && g_lanes != 64) return fail(MYO_E_UNSUPPORTED, "reward terms: the walk task runs on the wave-per-env kernel only (lanes = 64)");
  DevBatch& d = b->db;
  if (d.rwd && d.rwd_n != c.n) return fail(MYO_E_ARG, "reward terms: enabled for another task");
  HIPCHK(hipSetDevice(b->model->device));
  int rc;
  if (!d.rwd) {
    float *row = nullptr, *wd = nullptr;
    if ((rc = b->pool.alloc(&row, (size_t)d.B * c.n * 4)) || (rc = b->pool.alloc(&wd, (size_t)nw * 4))) return rc;
    d.rwd = row; d.rwd_w = wd; d.rwd_n = c.n;
  }
  if ((rc = copy_to_device(b->model->device, (void*)d.rwd_w, w, (size_t)nw * 4))) return rc;
  d.rwd_sparse = mode == MYO_RWD_SPARSE;
  return MYO_OK;
}

static int walk_terms_launch(myo_batch* b, hipStream_t s) {
  const myo_model* m = b->model;
  hipLaunchKernelGGL(walk_terms_kernel, dim3(b->db.B), dim3(64), 0, s, b->db, (const DevWalk*)b->d_walk, m->nq, m->dm.nv, m->dm.nu, m->dm.na_obs);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

static int episode_enable(myo_batch* b) {
  if (!b->db.rwd) return fail(MYO_E_ARG, "episode statistics: enable the reward terms first (myo_batch_enable_rewards)");
  if (b->episode.run) return MYO_OK;
  myo_episode ep;
  const size_t B = b->db.B;
  int rc;
  HIPCHK(hipSetDevice(b->model->device));
  if ((rc = b->pool.alloc(&ep.run, B * 16)) || (rc = b->pool.alloc(&ep.last, B * 16)) ||
      (rc = b->pool.alloc(&ep.finished, (B + 3) / 4 * 4)) || (rc = b->pool.alloc(&ep.count, B * 4))) return rc;
  b->episode = ep;
  return MYO_OK;
}

int myo_batch_rwd_ncol(const myo_batch* b) { return b ? rwd_cols(b->task.task).n : 0; }
const char* myo_batch_rwd_name(const myo_batch* b, int col) {
  const RwdCols c = rwd_cols(b ? b->task.task : MYO_TASK_NONE);
  return col >= 0 && col < c.n ? c.name[col] : nullptr;
}
int myo_batch_enable_rewards(myo_batch* b, const float* weights, int nweights, int mode) {
  return b ? rewards_enable(b, weights, nweights, mode) : fail(MYO_E_ARG, "myo_batch_enable_rewards: null");
}
// the two families' refusals ("host copy" is the size error of both reads)
static int rwd_buf(const myo_batch* b, int, DevBuf* d) {
  if (!b->db.rwd) return fail(MYO_E_ARG, "reward terms are not enabled (myo_batch_enable_rewards)");
  *d = {b->db.rwd, (size_t)b->db.rwd_n, 4};
  return MYO_OK;
}
static int episode_buf(const myo_batch* b, int which, DevBuf* d) {
  const myo_episode* ep = &b->episode;
  if (!ep->run) return fail(MYO_E_ARG, "episode statistics are not enabled (myo_batch_enable_episode_stats)");
  switch (which) {
    case MYO_EP_RUNNING: *d = {ep->run, 4, 4}; break;
    case MYO_EP_LAST: *d = {ep->last, 4, 4}; break;
    case MYO_EP_FINISHED: *d = {ep->finished, 1, 1}; break;
    case MYO_EP_COUNT: *d = {ep->count, 1, 4}; break;
    default: return fail(MYO_E_ARG, "myo_batch_episode_buffer: unknown buffer");
  }
  return MYO_OK;
}
int myo_batch_rwd_row(myo_batch* b, void** dev_ptr, size_t* pitch, size_t* width) {
  return buf_lookup(rwd_buf, b, 0, dev_ptr, pitch, width, "myo_batch_rwd_row: null");
}
int myo_batch_rwd_read(myo_batch* b, void* host, size_t nbytes) {
  return b ? buf_read(rwd_buf, b, 0, host, nbytes, "host copy: size mismatch") : fail(MYO_E_ARG, "myo_batch_rwd_row: null");
}
int myo_batch_enable_episode_stats(myo_batch* b) { return b ? episode_enable(b) : fail(MYO_E_ARG, "myo_batch_enable_episode_stats: null"); }
int myo_batch_episode_buffer(myo_batch* b, int which, void** dev_ptr, size_t* pitch, size_t* width) {
  return buf_lookup(episode_buf, b, which, dev_ptr, pitch, width, "myo_batch_episode_buffer: null");
}
int myo_batch_episode_read(myo_batch* b, int which, void* host, size_t nbytes) {
  return b ? buf_read(episode_buf, b, which, host, nbytes, "host copy: size mismatch") : fail(MYO_E_ARG, "myo_batch_episode_buffer: null");
}
int myo_episode_update(myo_batch* b, int max_episode_steps, void* stream) {
  if (!b || max_episode_steps <= 0) return fail(MYO_E_ARG, "myo_episode_update: bad arguments");
  const myo_episode* ep = &b->episode;
  if (!ep->run) return fail(MYO_E_ARG, "episode statistics are not enabled (myo_batch_enable_episode_stats)");
  HIPCHK(hipSetDevice(b->model->device));
  hipLaunchKernelGGL(episode_stats_kernel, dim3((b->db.B + 255) / 256), dim3(256), 0, (hipStream_t)stream, b->db, (float4*)ep->run, (float4*)ep->last,
                     ep->finished, ep->count, max_episode_steps);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}
int myo_episode_clear(myo_batch* b, void* stream) {
  if (!b) return fail(MYO_E_ARG, "myo_episode_clear: null");
  const myo_episode* ep = &b->episode;
  if (!ep->run) return fail(MYO_E_ARG, "episode statistics are not enabled (myo_batch_enable_episode_stats)");
  HIPCHK(hipSetDevice(b->model->device));
  HIPCHK(hipMemsetAsync(ep->run, 0, (size_t)b->db.B * 16, (hipStream_t)stream));
  HIPCHK(hipMemsetAsync(ep->finished, 0, (size_t)b->db.B, (hipStream_t)stream));
  return MYO_OK;
}

#endif  // MYO_REWARDS_H
