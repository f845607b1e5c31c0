// myo_task_myodm.h -- the classic gym flavour of the MyoDM TrackEnv (envs/myo/myodm/myodm_v0.py, the entry point of the registered MyoDM
// ids): observation / reward / done / metrics of MYO_TASK_TRACK batches configured with myo_track_config.flavour = 1.  The MJX flavour
// (flavour = 0) is fused into the TRK step kernel (myo_task_track.h); only its state row, mjx_track_obs_body, is here.
//
// The env step itself is BaseV0.step on the TRK step kernel, unchanged: the muscle sigmoid on the muscles, the raw action on the position
// actuators (clamped to ctrlrange where the actuator force reads it, as MuJoCo clamps ctrl), frame_skip = 10 substeps.  get_obs_dict then
// reads the reference at the POST-step time and the object / wrist body frames of the post-step state (update_reference_insim's
// sim.forward()), so this kernel runs its own forward kinematics of the two links it reads, from the post-step qpos, one lane each.
// One 64-lane workgroup per env.
#ifndef MYO_TASK_MYODM_H
#define MYO_TASK_MYODM_H

// get_obs_dict (:189-251, + act, base_v0.py:34-38) and get_reward_dict / check_termination (:253-311, :336-362) of env e.  Row: qpos (nq),
// qvel (nv), hand_qpos_err (nr), hand_qvel_err (nr, or the single 0 of a reference without robot_vel), obj_com_err (3), act (na).
// The reference row is looked up at t = elapsed * frame_skip * timestep + motion_start_time in double (the post-step sim.data.time, which
// the reference rounds to 4 decimals before comparing it with the frame times); RANDOM draws are keyed by (seed, the env's episode count,
// global env id, env step).  `seed` is the seed of the last reset.
__device__ __forceinline__ void myodm_obs_body(const DevModel& M, const DevBatch& Bt, const TaskDev& T, const DevTrack& K, uint64_t seed, int obs_only,
                                               const int e, const int lane) {
  const int nv = M.nv, nr = K.robot_dim;
  const int vdim = K.has_vel ? nr : 1, oe = 2 * nv + nr + vdim;   // offset of obj_com_err
  const auto [o, q, v, a, dt] = task_row(M, Bt, T, e, nv);
  const int elapsed = Bt.elapsed[e];
  track_lookup<true>(K, e, e + Bt.env_offset, 0.f, elapsed, lane, (double)elapsed * (double)T.frame_skip * (double)M.timestep,
                     rng_episode_seed(seed, Bt.episode[e]));
  __syncthreads();                       // the reference row (written by lanes < nr + 7) is complete before every lane reads it
  const float* R = K.ref + (size_t)e * K.ref_pitch;
  const float* tc = R + 2 * nr;          // target object pose: com (3) | quaternion (4)
  // xipos / ximat of the object body (lane 0) and xipos of the wrist (lunate) body (lane 1) of the post-step state
  float p[3] = {0.f, 0.f, 0.f}, Rb[9], x[2][3];
  if (lane < 2) link_chain<true>(M, Bt, q, e, lane == 0 ? K.obj_link : K.wrist_link, lane == 0 ? K.obj_p : K.wrist_p, K.obj_R, p, Rb);
  site_gather<2>(M, Bt, e, lane, 0, p, x);
  const float *com = x[0], *wr = x[1];
  for (int i = lane; i < nv; i += 64) { o[i] = q[i]; o[nv + i] = v[i]; }
  float qe = 0.f, ve = 0.f;
  if (lane < nr) {
    qe = q[lane] - R[lane];
    o[2 * nv + lane] = qe;
    if (K.has_vel) { ve = v[lane] - R[nr + lane]; o[2 * nv + nr + lane] = ve; }
  }
  if (!K.has_vel && lane == 0) o[2 * nv + nr] = 0.f;
  if (lane < 3) o[oe + lane] = com[lane] - tc[lane];
  for (int i = lane; i < M.nu; i += 64) { const int sl = M.act_obs[i]; if (sl >= 0) o[oe + 3 + sl] = a[i]; }   // (the reward has no activation term)
  if (obs_only) return;
  const float q2 = wave_sum(qe * qe), v2 = wave_sum(ve * ve);
  if (lane == 0) {
    float cq[4];
    track_mat2quat(Rb, cq);
    const float e0 = tc[0] - com[0], e1 = tc[1] - com[1], e2 = tc[2] - com[2];
    const float obj_com_err = sqrtf(e0 * e0 + e1 * e1 + e2 * e2);
    const float obj_rot_err = track_rot_err(cq, tc + 3);
    const float obj_reward = expf(-K.obj_err_scale * (obj_com_err + 0.1f * obj_rot_err));            // :262-265
    const float lift_bonus = (tc[2] >= K.lift_z && com[2] >= K.lift_z) ? 1.f : 0.f;                 // :268
    const float qpos_reward = expf(-K.qpos_err_scale * q2);
    const float qvel_reward = expf(-K.qvel_err_scale * v2);             // hand_qvel_err = [0] without robot_vel: exp(0) = 1 (:276-280)
    const float b0 = com[0] - wr[0], b1 = com[1] - wr[1], b2 = com[2] - wr[2];
    const float base_error = sqrtf(b0 * b0 + b1 * b1 + b2 * b2);
    const float base_reward = expf(-K.base_err_scale * base_error);
    bool term = false;
    if (K.term_obj) term = term || (obj_com_err * obj_com_err >= K.obj_fail2) || (base_error * base_error >= K.base_fail2);
    if (K.term_pose) term = term || (q2 >= K.qpos_fail);
    const float done = term ? 1.f : 0.f;
    const float m_pose = K.qpos_w * qpos_reward + K.qvel_w * qvel_reward, m_obj = obj_reward + base_reward, m_bonus = K.lift_bonus_mag * lift_bonus;
    Bt.reward[e] = K.w_pose * m_pose + K.w_object * m_obj + K.w_bonus * m_bonus + K.w_penalty * done;
    Bt.done[e] = done;
    Bt.solved[e] = 0.f;
    float* mt = K.metrics + 4 * (size_t)e;
    mt[0] = m_pose; mt[1] = m_obj; mt[2] = m_bonus; mt[3] = done;
  }
}

using MyodmTask = TrackObs<myodm_obs_body>;

// the MJX flavour's row, TrackEnv.get_obs (mjx/myodm_v0.py:297-304): [qpos, qvel]; reward / done belong to the step kernel's epilogue (they
// need the reference row of the step and the body frames of its last substep) and are not recomputed here
__device__ __forceinline__ void mjx_track_obs_body(const DevModel& M, const DevBatch& Bt, const TaskDev& T, int, const int e, const int lane) {
  const int nv = M.nv, nq = T.nq;
  const auto [o, q, v, a, dt] = task_row(M, Bt, T, e, nq);
  for (int i = lane; i < nq; i += 64) o[i] = q[i];
  for (int i = lane; i < nv; i += 64) o[nq + i] = v[i];
}
using MjxTrackTask = StateObs<mjx_track_obs_body>;

// MYO_TASK_TRACK of either flavour: the configure of myo_batch_configure_track (a config record of its own: no configure hook).  The
// reference tables and the per-env reference rows go into the batch's pool; every call uploads its tables anew
static int track_configure(myo_batch* b, const myo_track_config* c) {
  const myo_model* m = b->model;
  if (!(m->wave_ok && m->trk)) return fail(MYO_E_UNSUPPORTED, "track task: models of the TrackEnv class only (condim-4 / friction-loss / hull geoms)");
  const int nq = m->nq, nv = m->dm.nv, nu = m->dm.nu;
  if (c->n_frames <= 0 || c->ref_type < 0 || c->ref_type > 2 || c->horizon < 1 || c->robot_dim < 0 || c->object_dim < 0 || c->robot_dim > 64 ||
      c->robot_dim + c->object_dim > 64 || c->robot_dim > nq || !c->ref_time || !c->init_qpos || !c->ctrl_lo || !c->ctrl_hi)
    return fail(MYO_E_ARG, "myo_batch_configure_track: bad reference / pose arguments");
  if ((c->robot_dim > 0 && (!c->ref_robot || c->robot_horizon < 1)) || (c->object_dim > 0 && (!c->ref_object || c->object_horizon < 1)))
    return fail(MYO_E_ARG, "myo_batch_configure_track: reference rows missing");
  if (c->ref_type == 1 && ((c->robot_dim > 0 && c->robot_horizon < 2) || (c->object_dim > 0 && c->object_horizon < 2))) return fail(MYO_E_ARG, "RANDOM reference needs two rows");
  if (c->object_link < 0 || c->object_link >= m->dm.nl || c->wrist_link < 0 || c->wrist_link >= m->dm.nl) return fail(MYO_E_ARG, "myo_batch_configure_track: link out of range");
  if (c->flavour != 0 && c->flavour != 1) return fail(MYO_E_ARG, "myo_batch_configure_track: flavour must be 0 (MJX) or 1 (classic)");
  // classic flavour (envs/myo/myodm/myodm_v0.py): hand_qpos_err = qpos[:-6] - robot, the object pose is 7 wide, and its own kinematics walk
  // takes hinge / slide joints only
  if (c->flavour == 1 && (nq != nv || c->robot_dim != nq - 6 || c->object_dim != 7))
    return fail(MYO_E_ARG, "myo_batch_configure_track: the classic flavour needs nq == nv, robot_dim == nq - 6 and object_dim == 7");
  const int obs_dim = c->flavour == 1 ? nq + nv + c->robot_dim + (c->ref_robot_vel ? c->robot_dim : 1) + 3 + m->dm.na_obs : nq + nv;
  if (obs_dim > b->obs_alloc) return fail(MYO_E_ARG, "obs_dim too large");
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipDeviceSynchronize());
  const int B = b->db.B;
  DevPool& pool = b->pool;
  DevTrack K{};
  K.ref_type = c->ref_type; K.horizon = c->horizon; K.robot_horizon = c->robot_horizon; K.object_horizon = c->object_horizon;
  K.robot_dim = c->robot_dim; K.object_dim = c->object_dim; K.has_vel = c->ref_robot_vel != nullptr;
  K.extrapolate = c->motion_extrapolation; K.linear = c->interpolation_linear; K.autoreset = c->autoreset;
  K.term_obj = c->terminate_obj_fail; K.term_pose = c->terminate_pose_fail; K.start_time = c->motion_start_time; K.max_steps = c->max_episode_steps;
  const size_t nrobot = (size_t)c->robot_horizon * c->robot_dim;
  int rc;
  if ((rc = pool.upload(&K.T, c->ref_time, (size_t)c->horizon)) || (rc = pool.upload(&K.robot, c->ref_robot, nrobot)) ||
      (K.has_vel && (rc = pool.upload(&K.robot_vel, c->ref_robot_vel, nrobot))) ||
      (rc = pool.upload(&K.object, c->ref_object, (size_t)c->object_horizon * c->object_dim)) || (rc = pool.upload(&K.init_qpos, c->init_qpos, (size_t)nq)) ||
      (rc = pool.upload(&K.lo, c->ctrl_lo, (size_t)nu)) || (rc = pool.upload(&K.hi, c->ctrl_hi, (size_t)nu))) return rc;
  K.obj_link = c->object_link; K.wrist_link = c->wrist_link;
  for (int k = 0; k < 3; k++) { K.obj_p[k] = c->object_ipos[k]; K.wrist_p[k] = c->wrist_ipos[k]; }
  for (int k = 0; k < 9; k++) K.obj_R[k] = c->object_imat[k];
  K.lift_z = c->lift_z; K.obj_err_scale = c->obj_err_scale; K.base_err_scale = c->base_err_scale; K.lift_bonus_mag = c->lift_bonus_mag;
  K.qpos_w = c->qpos_reward_weight; K.qpos_err_scale = c->qpos_err_scale; K.qvel_w = c->qvel_reward_weight; K.qvel_err_scale = c->qvel_err_scale;
  K.obj_fail2 = c->obj_fail_thresh * c->obj_fail_thresh; K.base_fail2 = c->base_fail_thresh * c->base_fail_thresh; K.qpos_fail = c->qpos_fail_thresh;
  K.w_pose = c->w_pose; K.w_object = c->w_object; K.w_bonus = c->w_bonus; K.w_penalty = c->w_penalty;
  K.ref_pitch = 2 * c->robot_dim + c->object_dim;
  K.seed = c->seed;
  if ((rc = pool.alloc(&K.ref, (size_t)B * K.ref_pitch * 4)) || (!b->d_metrics && (rc = pool.alloc(&b->d_metrics, (size_t)B * 4 * 4))) ||
      (!b->d_track && (rc = pool.alloc(&b->d_track, sizeof(DevTrack))))) return rc;
  K.metrics = b->d_metrics;
  HIPCHK(hipMemcpy(b->d_track, &K, sizeof(DevTrack), hipMemcpyHostToDevice));
  b->db.track = b->d_track;
  b->track_frames = c->n_frames;
  b->track_flavour = c->flavour;
  // the generic reset / observation plumbing: TrackEnv.reset puts every env at init_qpos with zero velocity, activation, control and time
  TaskDev& T = b->task;
  T = TaskDev{};
  T.task = MYO_TASK_TRACK; T.frame_skip = c->n_frames; T.nq = nq; T.obs_dim = obs_dim;
  HIPCHK(hipMemcpy(b->d_init, c->init_qpos, (size_t)nq * 4, hipMemcpyHostToDevice));
  T.init_qpos = b->d_init; T.jnt_lo = b->d_jlo; T.jnt_hi = b->d_jhi; T.target_lo = b->d_tlo; T.target_hi = b->d_thi;
  return MYO_OK;
}

// The classic flavour observes with MyodmTask, keyed by the seed of the last reset, and has a fused epilogue; the MJX flavour observes the
// state-only row and myo_bench_rollout skips its epilogue (the step kernel's own)
static int track_obs(myo_batch* b, hipStream_t s, int obs_only, int reset_only) {
  return b->track_flavour == 1 ? launch_task_obs<MyodmTask>(b, s, obs_only, reset_only) : launch_task_obs<MjxTrackTask>(b, s, obs_only, reset_only);
}
static int track_post(myo_batch* b, hipStream_t s, uint64_t seed, int max_episode_steps) {
  b->reset_seed = seed;
  return launch_task_post<MyodmTask>(b, s, seed, max_episode_steps);
}
static const TaskHooks track_hooks = {nullptr, track_obs, track_post};

#endif  // MYO_TASK_MYODM_H
