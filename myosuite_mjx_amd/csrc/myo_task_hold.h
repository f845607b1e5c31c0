// myo_task_hold.h -- ObjHold{Fixed,Random}EnvV0 (envs/myo/myobase/obj_hold_v0.py) observation / reward / done / solved, MYO_TASK_HOLD.
// The object's site sits at the origin of its free body, whose world position is the free joint's qpos (free-floating models are not
// origin-shifted); the goal site is world-fixed = the target row.  One 64-lane workgroup per env.
#ifndef MYO_TASK_HOLD_H
#define MYO_TASK_HOLD_H

// obj_hold_v0.py:66-118.  Row: hand qpos, hand qvel * dt (the object's free joint comes last), object position, obj_err = goal - object, act
struct HoldRow {
  int nq, nv, na;
  Blk hand_qpos = {0, nq - 7}, hand_qvel = hand_qpos.then(nv - 6), obj_pos = hand_qvel.then(3), obj_err = obj_pos.then(3), act = obj_err.then(na);
  int dim = act.end();
};
__device__ __forceinline__ void hold_obs_body(const DevModel& M, const DevBatch& Bt, const TaskDev& T, int obs_only, const int e, const int lane) {
  const int nv = M.nv, nq = T.nq;
  const HoldRow R{nq, nv, M.na_obs};
  const auto [o, qq, v, a, dt] = task_row(M, Bt, T, e, nq);
  for (int i = lane; i < R.hand_qpos.n; i += 64) o[R.hand_qpos.at + i] = qq[i];
  for (int i = lane; i < R.hand_qvel.n; i += 64) o[R.hand_qvel.at + i] = v[i] * dt;
  float err2 = 0.f;
  if (lane < 3) {
    float p = qq[nq - 7 + lane] + M.origin[lane], er = Bt.target[(size_t)e * T.ntarget + lane] - p;
    o[R.obj_pos.at + lane] = p; o[R.obj_err.at + lane] = er;
    err2 = er * er;
  }
  const float act2 = act_sq(M, a, lane, o + R.act.at);
  if (obs_only) return;
  float dist = sqrtf(wave_sum(err2));
  float actn = act_norm(M, act2);
  if (lane == 0) {
    float bonus = (dist < 2.f * T.near_th ? 1.f : 0.f) + (dist < T.near_th ? 1.f : 0.f);
    float drop = dist > T.far_th ? 1.f : 0.f;
    const float solved = dist < T.near_th ? 1.f : 0.f;
    if (Bt.rwd) rwd_row(Bt, e, {-dist, bonus, -actn, -drop, -dist, solved, drop});      // obj_hold_v0.py:102-117
    else Bt.reward[e] = T.w_reach * (-dist) + T.w_bonus * bonus + T.w_act_reg * (-actn) + T.w_penalty * (-drop);
    Bt.solved[e] = solved;
    Bt.done[e] = drop;
  }
}

using HoldTask = StateObs<hold_obs_body>;
static int hold_configure(myo_batch* b, const myo_task_config* c) {
  const myo_model* m = b->model;
  const int nv = m->dm.nv, nq = m->nq;
  if (c->ntarget != 3) return fail(MYO_E_ARG, "hold task: ntarget must be 3 (goal position)");
  if (!(m->wave_ok && m->dw.has_free && nq == nv + 1 && nv > 6)) return fail(MYO_E_UNSUPPORTED, "hold task needs a model whose last joint is one free object");
  b->task.obs_dim = HoldRow{nq, nv, m->dm.na_obs}.dim;
  return MYO_OK;
}
static const char* const rwd_hold[] = {"goal_dist", "bonus", "act_reg", "penalty", RWD_TAIL};   // obj_hold_v0.py:102-117
static void obs_terms_hold(const ObsDims& D, ObsTable& t) {      // obj_hold_v0.py get_obs_dict
  const HoldRow R{D.nq, D.nv, D.na};
  TERM("time", 1, OBS_SRC_TIME, 0)
  ROW(R, hand_qpos)
  ROW(R, hand_qvel)
  ROW(R, obj_pos)
  ROW(R, obj_err)
  ROW(R, act)
  t.dim = R.dim;
}
static const TaskHooks hold_hooks = {hold_configure, launch_task_obs<HoldTask>, launch_task_post<HoldTask>, RWD_COLS(rwd_hold), obs_terms_hold};

#endif  // MYO_TASK_HOLD_H
