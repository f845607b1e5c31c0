// myo_task_pose.h -- PoseEnvV0 (envs/myo/myobase/pose_v0.py) observation / reward / done / solved, MYO_TASK_POSE.  The task reads the
// joint state alone.  One 64-lane workgroup per env, rows written coalesced.
#ifndef MYO_TASK_POSE_H
#define MYO_TASK_POSE_H

// pose_v0.py:98-138, obs_vec_dict.py:86-98.  Row: qpos, qvel * dt, pose_err = target - qpos, act
struct PoseRow {
  int nq, nv, na;
  Blk qpos = {0, nq}, qvel = qpos.then(nv), pose_err = qvel.then(nq), act = pose_err.then(na);
  int dim = act.end();
};
__device__ __forceinline__ void pose_obs_body(const DevModel& M, const DevBatch& Bt, const TaskDev& T, int obs_only, const int e, const int lane) {
  const int nv = M.nv;
  const PoseRow R{nv, nv, M.na_obs};   // nq == nv: hinge / slide joints only
  const auto [o, q, v, a, dt] = task_row(M, Bt, T, e, nv);
  float err2 = 0;
  for (int i = lane; i < nv; i += 64) {
    float qi = q[i], pe = Bt.target[(size_t)e * T.ntarget + i] - qi;
    o[R.qpos.at + i] = qi; o[R.qvel.at + i] = v[i] * dt; o[R.pose_err.at + i] = pe;
    err2 += pe * pe;
  }
  const float act2 = act_sq(M, a, lane, o + R.act.at);
  if (obs_only) return;
  float dist = sqrtf(wave_sum(err2));
  float actn = act_norm(M, act2);
  if (lane == 0) {
    float bonus = (dist < T.pose_thd ? 1.f : 0.f) + (dist < 1.5f * T.pose_thd ? 1.f : 0.f);
    float pen = dist > T.far_th ? -1.f : 0.f;
    const float solved = dist < T.pose_thd ? 1.f : 0.f, done = dist > T.far_th ? 1.f : 0.f;
    if (Bt.rwd) rwd_row(Bt, e, {-dist, bonus, pen, -actn, -dist, solved, done});        // pose_v0.py:118-135
    else Bt.reward[e] = T.w_pose * (-dist) + T.w_bonus * bonus + T.w_act_reg * (-actn) + T.w_penalty * pen;
    Bt.solved[e] = solved;
    Bt.done[e] = done;
  }
}

using PoseTask = StateObs<pose_obs_body>;
static int pose_configure(myo_batch* b, const myo_task_config* c) {
  const int nv = b->model->dm.nv;
  if (c->ntarget != nv) return fail(MYO_E_ARG, "pose task: ntarget must equal nq");
  b->task.obs_dim = PoseRow{nv, nv, b->model->dm.na_obs}.dim;
  return MYO_OK;
}
static const char* const rwd_pose[] = {"pose", "bonus", "penalty", "act_reg", RWD_TAIL};   // pose_v0.py:118-135
static void obs_terms_pose(const ObsDims& D, ObsTable& t) {      // pose_v0.py get_obs_dict
  const PoseRow R{D.nq, D.nv, D.na};
  TERM("time", 1, OBS_SRC_TIME, 0)
  ROW(R, qpos)
  ROW(R, qvel)
  if (D.na > 0) ROW(R, act)
  else TERM("act", D.pose_act, OBS_SRC_CONST, 3)   // no muscles: zeros_like(qpos), the constant table's zeros
  ROW(R, pose_err)
  t.dim = R.dim;
}
static const TaskHooks pose_hooks = {pose_configure, launch_task_obs<PoseTask>, launch_task_post<PoseTask>, RWD_COLS(rwd_pose), obs_terms_pose};

#endif  // MYO_TASK_POSE_H
