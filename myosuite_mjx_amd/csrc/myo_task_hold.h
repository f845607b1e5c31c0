// myo_task_hold.h -- ObjHold{Fixed,Random}EnvV0 (envs/myo/myobase/obj_hold_v0.py) observation / reward / done / solved, MYO_TASK_HOLD.
// The object's site sits at the origin of its free body, whose world position is the free joint's qpos (free-floating models are not
// origin-shifted); the goal site is world-fixed = the target row.  One 64-lane workgroup per env.
#ifndef MYO_TASK_HOLD_H
#define MYO_TASK_HOLD_H

// obj_hold_v0.py:66-118.  Row: hand qpos (nq - 7), hand qvel * dt (nv - 6), object position (3), obj_err = goal - object (3), act (na)
__device__ __forceinline__ void hold_obs_body(const DevModel& M, const DevBatch& Bt, const TaskDev& T, int obs_only, const int e, const int lane) {
  const int nv = M.nv, nq = T.nq, nqh = nq - 7, nvh = nv - 6;
  const auto [o, qq, v, a, dt] = task_row(M, Bt, T, e, nq);
  for (int i = lane; i < nqh; i += 64) o[i] = qq[i];
  for (int i = lane; i < nvh; i += 64) o[nqh + i] = v[i] * dt;
  float err2 = 0.f;
  if (lane < 3) {
    float p = qq[nqh + lane] + M.origin[lane], er = Bt.target[(size_t)e * T.ntarget + lane] - p;
    o[nqh + nvh + lane] = p; o[nqh + nvh + 3 + lane] = er;
    err2 = er * er;
  }
  const float act2 = act_sq(M, a, lane, o + nqh + nvh + 6);
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
  b->task.obs_dim = (nq - 7) + (nv - 6) + 6 + m->dm.na_obs;
  return MYO_OK;
}
static const TaskHooks hold_hooks = {hold_configure, launch_task_obs<HoldTask>, launch_task_post<HoldTask>};

#endif  // MYO_TASK_HOLD_H
