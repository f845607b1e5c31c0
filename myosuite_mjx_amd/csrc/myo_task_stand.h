// myo_task_stand.h -- ReachEnvV0 on the legs (envs/myo/myobase/walk_v0.py:68-127; myoLegStand*) observation / reward / done / solved,
// MYO_TASK_STAND.  The tip site rides on the free root link, so its world position comes straight from qpos.  One 64-lane workgroup per env.
#ifndef MYO_TASK_STAND_H
#define MYO_TASK_STAND_H

// Row: ReachRow (myo_task_reach.h) with one tip.  T.tip_lpos = the tip site in the root link's frame: world position = root position +
// Rm(root quat) tip_lpos
__device__ __forceinline__ void stand_obs_body(const DevModel& M, const DevBatch& Bt, const TaskDev& T, int obs_only, const int e, const int lane) {
  const int nv = M.nv, nq = T.nq;
  const ReachRow R{nq, nv, 1, M.na_obs};
  const auto [o, qq, v, a, dt] = task_row(M, Bt, T, e, nq);
  float vel2 = 0.f, err2 = 0.f;
  for (int i = lane; i < nq; i += 64) o[R.qpos.at + i] = qq[i];
  for (int i = lane; i < nv; i += 64) { const float vd = v[i] * dt; o[R.qvel.at + i] = vd; vel2 += vd * vd; }
  if (lane < 3) {
    float Rm[9];
    const float qn = 1.0f / sqrtf(qq[3] * qq[3] + qq[4] * qq[4] + qq[5] * qq[5] + qq[6] * qq[6]);
    const float uq[4] = {qq[3] * qn, qq[4] * qn, qq[5] * qn, qq[6] * qn};
    quat2mat(Rm, uq);
    const float p = qq[lane] + Rm[3 * lane] * T.tip_lpos[0] + Rm[3 * lane + 1] * T.tip_lpos[1] + Rm[3 * lane + 2] * T.tip_lpos[2] + M.origin[lane];
    const float er = Bt.target[(size_t)e * T.ntarget + lane] - p;
    o[R.tip_pos.at + lane] = p; o[R.reach_err.at + lane] = er;
    err2 = er * er;
  }
  const float act2 = act_sq(M, a, lane, o + R.act.at);
  if (obs_only) return;
  const float dist = sqrtf(wave_sum(err2)), veld = sqrtf(wave_sum(vel2));
  const float actn = act_norm(M, act2);
  if (lane == 0) {
    const float far_th = Bt.time[e] > 2.f * dt ? T.far_th : 1e30f;
    const float bonus = (dist < 2.f * T.near_th ? 1.f : 0.f) + (dist < T.near_th ? 1.f : 0.f);
    const float pen = dist > far_th ? 1.f : 0.f;
    const float solved = dist < T.near_th ? 1.f : 0.f;
    if (Bt.rwd) rwd_row(Bt, e, {10.0f - dist - 10.0f * veld, bonus, -100.0f * actn, -pen, -dist, solved, pen});   // walk_v0.py:117-133
    else Bt.reward[e] = T.w_reach * (10.0f - dist - 10.0f * veld) + T.w_bonus * bonus + T.w_act_reg * (-100.0f * actn) + T.w_penalty * (-pen);
    Bt.solved[e] = solved;
    Bt.done[e] = pen;
  }
}

using StandTask = StateObs<stand_obs_body>;
static int stand_configure(myo_batch* b, const myo_task_config* c) {
  const myo_model* m = b->model;
  const int nv = m->dm.nv, nq = m->nq;
  if (c->ntarget != 3) return fail(MYO_E_ARG, "stand task: ntarget must be 3 (target position)");
  if (!(m->wave_ok && m->dw.has_free && nq == nv + 1)) return fail(MYO_E_UNSUPPORTED, "stand task needs a model with a free root joint");
  b->task.obs_dim = ReachRow{nq, nv, 1, m->dm.na_obs}.dim;
  return MYO_OK;
}
static const TaskHooks stand_hooks = {stand_configure, launch_task_obs<StandTask>, launch_task_post<StandTask>, RWD_COLS(rwd_reach), obs_terms_reach};

#endif  // MYO_TASK_STAND_H
