// myo_task_keyturn.h -- KeyTurnEnvV0 (envs/myo/myobase/key_turn_v0.py) observation / reward / done / solved, MYO_TASK_KEYTURN.
//
// The model is of the TrackEnv class (the key's box bit and the friction loss of its hinge), whose step kernel keeps no kinematics a
// separate pass could reuse, and the lanes kernel's reach_obs_kernel is not available to it.  So this kernel runs its own forward
// kinematics, and only of what the task reads: the ancestor chains of its three sites (key head, index tip, thumb tip), one lane per site,
// from the post-step qpos -- the site positions of the reference's post-step forward pass.  One 64-lane workgroup per env.
#ifndef MYO_TASK_KEYTURN_H
#define MYO_TASK_KEYTURN_H

// key_turn_v0.py:82-156 (+ act, base_v0.py:34-38).  Row: hand qpos, hand qvel * dt (the key's hinge comes last), key qpos, key qvel * dt,
// head - index tip, head - thumb tip, act.  get_reward_dict reads the approach vectors and act from self.obs_dict but key_q from its argument;
// at step time both are the obs_dict of the stepped state, so one set of values serves both here.
struct KeyturnRow {
  int nq, nv, na;
  Blk hand_qpos = {0, nq - 1}, hand_qvel = hand_qpos.then(nv - 1), key_qpos = hand_qvel.then(1), key_qvel = key_qpos.then(1),
      IFtip_approach = key_qvel.then(3), THtip_approach = IFtip_approach.then(3), act = THtip_approach.then(na);
  int dim = act.end();
};
__device__ __forceinline__ void keyturn_obs_body(const DevModel& M, const DevBatch& Bt, const TaskDev& T, int obs_only, const int e, const int lane) {
  const int nv = M.nv, nh = nv - 1;
  const KeyturnRow R{nv, nv, M.na_obs};   // nq == nv (keyturn_configure)
  const auto [o, q, v, a, dt] = task_row(M, Bt, T, e, nv);
  float p[3] = {0.f, 0.f, 0.f}, x[3][3], dk = 0.f;
  if (lane < 3) site_pos(M, Bt, q, e, T.tip_site[lane], p);   // lane 0: key head, 1: index tip, 2: thumb tip
  site_gather<3>(M, Bt, e, lane, 3, p, x);
  if (lane == 1 || lane == 2) {
    const float* h = x[0];
    const float r[3] = {h[0] - p[0], h[1] - p[1], h[2] - p[2]};
#pragma unroll
    for (int k = 0; k < 3; k++) o[(lane == 1 ? R.IFtip_approach.at : R.THtip_approach.at) + k] = r[k];
    dk = fabsf(norm3(r) - T.near_th);
  }
  for (int i = lane; i < nv; i += 64) {
    if (i < nh) { o[R.hand_qpos.at + i] = q[i]; o[R.hand_qvel.at + i] = v[i] * dt; }
    else { o[R.key_qpos.at] = q[i]; o[R.key_qvel.at] = v[i] * dt; }
  }
  const float act2 = act_sq(M, a, lane, o + R.act.at);
  const float d_if = __shfl(dk, 1), d_th = __shfl(dk, 2);
  if (obs_only) return;
  const float actn = act_norm(M, act2);
  if (lane == 0) {
    const float key_q = q[nh];
    const float bonus = (key_q > 1.57079632679489662f ? 1.f : 0.f) + (key_q > 3.14159265358979324f ? 1.f : 0.f);
    const float pen = -(d_if > 0.5f * T.far_th ? 1.f : 0.f) - (d_th > 0.5f * T.far_th ? 1.f : 0.f);
    const float solved = key_q > T.pose_thd ? 1.f : 0.f, done = (d_if > T.far_th || d_th > T.far_th) ? 1.f : 0.f;
    if (Bt.rwd) rwd_row(Bt, e, {key_q, -d_if, -d_th, -actn, bonus, pen, key_q, solved, done});   // key_turn_v0.py:134-152
    else Bt.reward[e] = T.w_pose * key_q + T.w_reach * (-d_if) + T.w_reach * (-d_th) + T.w_act_reg * (-actn) + T.w_bonus * bonus + T.w_penalty * pen;
    Bt.solved[e] = solved;
    Bt.done[e] = done;
  }
}

using KeyturnTask = StateObs<keyturn_obs_body>;
// key_turn_v0.py: the key is the model's last joint, one hinge of a root body; sites = key head, index tip, thumb tip
static int keyturn_configure(myo_batch* b, const myo_task_config* c) {
  const myo_model* m = b->model;
  const int nv = m->dm.nv;
  if (!trk_model(m) || m->bp_link < 0) return fail(MYO_E_UNSUPPORTED, "key-turn task: a TrackEnv-class model without free / ball joints whose last joint is the hinge of a root body");
  if (m->dof_type[nv - 1] != 3 || m->link_dofnum[m->bp_link] != 1 || m->dof_link[nv - 1] != m->bp_link) return fail(MYO_E_UNSUPPORTED, "key-turn task: the last joint must be the one hinge of its root body");
  if (c->ntip != 3 || c->ntarget != 0) return fail(MYO_E_ARG, "key-turn task: ntip = 3 (key head, index tip, thumb tip) and ntarget = 0");
  if (!sites_in_range(m, c, 3)) return fail(MYO_E_ARG, "key-turn task: site id out of range");
  if (!(c->near_th >= 0.f) || !(c->far_th > 0.f) || !is_number(c->pose_thd)) return fail(MYO_E_ARG, "key-turn task: near_th >= 0, far_th > 0, goal_th (pose_thd) a number");
  b->task.obs_dim = KeyturnRow{m->nq, nv, m->dm.na_obs}.dim;
  return MYO_OK;
}
static const char* const rwd_keyturn[] = {"key_turn", "IFtip_approach", "THtip_approach", "act_reg", "bonus", "penalty", RWD_TAIL};   // key_turn_v0.py:134-152
static void obs_terms_keyturn(const ObsDims& D, ObsTable& t) {   // key_turn_v0.py get_obs_dict
  const KeyturnRow R{D.nq, D.nv, D.na};
  TERM("time", 1, OBS_SRC_TIME, 0)
  ROW(R, hand_qpos)
  ROW(R, hand_qvel)
  ROW(R, key_qpos)
  ROW(R, key_qvel)
  ROW(R, IFtip_approach)
  ROW(R, THtip_approach)
  ROW(R, act)
  t.dim = R.dim;
}
static const TaskHooks keyturn_hooks = {keyturn_configure, launch_task_obs<KeyturnTask>, launch_task_post<KeyturnTask>, RWD_COLS(rwd_keyturn), obs_terms_keyturn};

#endif  // MYO_TASK_KEYTURN_H
