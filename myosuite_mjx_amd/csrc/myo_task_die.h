// myo_task_die.h -- ReorientEnvV0 (envs/myo/myochallenge/reorient_v0.py; myoChallengeDieReorient{Demo,P1}-v0) observation / reward / done /
// solved, MYO_TASK_DIE.
//
// The model (myohand_die) is of the TrackEnv class (the die's boxes), so, as for the key turn, the pen and the balls, this kernel runs its
// own forward kinematics of what the task reads, from the post-step qpos: the die's and the target's origin and axis sites (object_o / x /
// y / z, target_o / x / y / z), one lane each.  Column k of a site frame is (x_k - x_o) / |lpos_k - lpos_o|, the way the pen's axis is
// built.  The target is world-welded: its sites are static, turn with the per-env orientation of MYO_F_BODYQUAT and shift by the env's
// MYO_F_TARGET row (the goal offset; the target carries no colliding geom, so the step kernel never reads it).  One 64-lane workgroup per env.
#ifndef MYO_TASK_DIE_H
#define MYO_TASK_DIE_H

// utils/quat_math.py:96-115 mat2euler, both branches; cx, cy, cz = the columns of the rotation matrix
__device__ __forceinline__ void die_mat2euler(float* eu, const float* cx, const float* cy, const float* cz) {
  const float c = sqrtf(cz[2] * cz[2] + cz[1] * cz[1]);
  eu[1] = -atan2f(-cz[0], c);
  if (c > 8.8817841970012523e-16f) {   // _EPS4 = 4 eps(float64)
    eu[2] = -atan2f(cy[0], cx[0]);
    eu[0] = -atan2f(cz[1], cz[2]);
  } else {
    eu[2] = -atan2f(-cx[1], cy[1]);
    eu[0] = 0.f;
  }
}

// reorient_v0.py:111-176.  Row: qpos[:-7] (the reference's off-by-one is kept: the hand's last joint is missing), qvel[:-6] * dt, obj_pos,
// goal_pos, pos_err = goal_pos - obj_pos - goal_obj_offset, obj_rot, goal_rot, rot_err = goal_rot - obj_rot; act is not observed.
// T.tip_site = object_o, object_x, object_y, object_z, target_o, target_x, target_y, target_z; T.tip_lpos = goal_obj_offset; Bt.target row =
// the goal offset from the compiled target position.
struct DieRow {
  int nq, nv;
  Blk hand_qpos_noMD5 = {0, nq - 7}, hand_qvel = hand_qpos_noMD5.then(nv - 6), obj_pos = hand_qvel.then(3), goal_pos = obj_pos.then(3),
      pos_err = goal_pos.then(3), obj_rot = pos_err.then(3), goal_rot = obj_rot.then(3), rot_err = goal_rot.then(3);
  int dim = rot_err.end();
};
__device__ __forceinline__ void die_obs_body(const DevModel& M, const DevBatch& Bt, const TaskDev& T, int obs_only, const int e, const int lane) {
  const int nv = M.nv;
  const DieRow R{nv, nv};   // nq == nv (die_configure)
  const auto [o, q, v, a, dt] = task_row(M, Bt, T, e, nv);
  float p[3] = {0.f, 0.f, 0.f}, x[8][3];
  if (lane < 8) {   // lanes 0-3: the die's sites, 4-7: the target's
    site_pos(M, Bt, q, e, T.tip_site[lane], p);
    if (lane >= 4) {   // a static site of the per-env oriented body (checked at configure), moved by the env's goal offset
      if (Bt.bquat) body_rot_point({Bt.bquat + 4 * (size_t)e, Bt.bq_c, nullptr}, p);
      const float* g = Bt.target + 3 * (size_t)e;
      p[0] += g[0]; p[1] += g[1]; p[2] += g[2];
    }
  }
  site_gather<8>(M, Bt, e, lane, 8, p, x);
  float col[6][3];   // the columns of the die's frame (0-2) and of the target's (3-5)
#pragma unroll
  for (int f = 0; f < 2; f++)
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float* l0 = M.site_lpos + 3 * T.tip_site[4 * f];
      const float* lk = M.site_lpos + 3 * T.tip_site[4 * f + 1 + k];
      const float d[3] = {lk[0] - l0[0], lk[1] - l0[1], lk[2] - l0[2]};
      const float inv = 1.0f / norm3(d);   // (rotation invariant: from the model's site positions)
#pragma unroll
      for (int c = 0; c < 3; c++) col[3 * f + k][c] = (x[4 * f + 1 + k][c] - x[4 * f][c]) * inv;
    }
  float orot[3], grot[3], perr[3], rerr[3];
  die_mat2euler(orot, col[0], col[1], col[2]);
  die_mat2euler(grot, col[3], col[4], col[5]);
#pragma unroll
  for (int k = 0; k < 3; k++) { perr[k] = x[4][k] - x[0][k] - T.tip_lpos[k]; rerr[k] = grot[k] - orot[k]; }
  if (lane < 3) {
    o[R.obj_pos.at + lane] = x[0][lane];
    o[R.goal_pos.at + lane] = x[4][lane];
    o[R.pos_err.at + lane] = perr[lane];
    o[R.obj_rot.at + lane] = orot[lane];
    o[R.goal_rot.at + lane] = grot[lane];
    o[R.rot_err.at + lane] = rerr[lane];
  }
  for (int i = lane; i < R.hand_qvel.n; i += 64) {
    if (i < R.hand_qpos_noMD5.n) o[R.hand_qpos_noMD5.at + i] = q[i];
    o[R.hand_qvel.at + i] = v[i] * dt;
  }
  if (obs_only) return;
  const float actn = act_norm(M, act_sq(M, a, lane));
  if (lane == 0) {
    const float pos_dist = norm3(perr), rot_dist = norm3(rerr);
    const bool drop = pos_dist > T.far_th;
    const float bonus = (pos_dist < 2.f * T.near_th ? 1.f : 0.f) + (pos_dist < T.near_th ? 1.f : 0.f);
    const float solved = (pos_dist < T.near_th && rot_dist < T.pose_thd && !drop) ? 1.f : 0.f, done = drop ? 1.f : 0.f;
    if (Bt.rwd) rwd_row(Bt, e, {-pos_dist, -rot_dist, bonus, -actn, -done, -rot_dist - 10.0f * pos_dist, solved, done});   // reorient_v0.py:148-176
    else Bt.reward[e] = T.w_pose * (-pos_dist) + T.w_reach * (-rot_dist) + T.w_bonus * bonus + T.w_act_reg * (-actn) + T.w_penalty * (drop ? -1.f : 0.f);
    Bt.solved[e] = solved;
    Bt.done[e] = done;
  }
}

using DieTask = StateObs<die_obs_body>;
// reorient_v0.py: the die is the model's last six joints, 3 slides + 3 hinges of one root body; the target is the body of MYO_F_BODYQUAT.
// goal_obj_offset (:68-71) = target_o - object_o at qpos0, from the compiled body and site positions (both bodies are children of the world)
static int die_configure(myo_batch* b, const myo_task_config* c) {
  const myo_model* m = b->model;
  TaskDev& T = b->task;
  const int nv = m->dm.nv;
  if (!trk_model(m) || nv < 8) return fail(MYO_E_UNSUPPORTED, "die task: a TrackEnv-class model without free / ball joints whose last six joints are the die's");
  const int ol = object_link_6dof(m);
  if (ol < 0) return fail(MYO_E_UNSUPPORTED, "die task: the last six joints must be 3 slides + 3 hinges of one root body");
  if (c->ntip != 8 || c->ntarget != 3) return fail(MYO_E_ARG, "die task: ntip = 8 (object_o / x / y / z, target_o / x / y / z) and ntarget = 3 (goal offset)");
  if (!sites_in_range(m, c, 8)) return fail(MYO_E_ARG, "die task: site id out of range");
  if (b->bq_body < 0) return fail(MYO_E_ARG, "die task: quat_body (the target body) must be selected");
  if (m->site_body.empty() || m->site_pos0.empty() || m->body_pos0.empty()) return fail(MYO_E_UNSUPPORTED, "die task: the model blob lacks the body tables");
  const int ob = m->site_body[c->tip_site[0]], tb = b->bq_body;
  for (int k = 0; k < 4; k++)
    if (m->site_link[c->tip_site[k]] != ol || m->site_body[c->tip_site[k]] != ob || m->site_body[c->tip_site[4 + k]] != tb)
      return fail(MYO_E_UNSUPPORTED, "die task: the object sites must be on the die's body, the target sites on the quat_body");
  if (m->body_parent[ob] != 0) return fail(MYO_E_UNSUPPORTED, "die task: the die's body must be a child of the world");
  auto site_world0 = [&](int body, int s, double* w) {
    double R[9];
    quat2mat_d(R, &m->body_quat0[4 * (size_t)body]);
    const double* sp = &m->site_pos0[3 * (size_t)s];
    for (int k = 0; k < 3; k++) w[k] = m->body_pos0[3 * (size_t)body + k] + R[3 * k] * sp[0] + R[3 * k + 1] * sp[1] + R[3 * k + 2] * sp[2];
  };
  for (int f = 0; f < 2; f++)
    for (int k = 1; k < 4; k++) {
      const double *s0 = &m->site_pos0[3 * (size_t)c->tip_site[4 * f]], *sk = &m->site_pos0[3 * (size_t)c->tip_site[4 * f + k]];
      if (!(std::hypot(sk[0] - s0[0], sk[1] - s0[1], sk[2] - s0[2]) > 1e-6)) return fail(MYO_E_ARG, "die task: an axis site coincides with its origin site");
    }
  if (!is_number(c->near_th) || !is_number(c->pose_thd) || !is_number(c->far_th)) return fail(MYO_E_ARG, "die task: near_th (pos_th), pose_thd (rot_th) and far_th (drop_th) numbers");
  double wo[3], wt[3];
  site_world0(ob, c->tip_site[0], wo);
  site_world0(tb, c->tip_site[4], wt);
  for (int k = 0; k < 3; k++) T.tip_lpos[k] = (float)(wt[k] - wo[k]);
  T.obs_dim = DieRow{m->nq, nv}.dim;
  return MYO_OK;
}
static const char* const rwd_die[] = {"pos_dist", "rot_dist", "bonus", "act_reg", "penalty", RWD_TAIL};   // reorient_v0.py:148-176
static void obs_terms_die(const ObsDims& D, ObsTable& t) {       // reorient_v0.py get_obs_dict
  const DieRow R{D.nq, D.nv};
  TERM("time", 1, OBS_SRC_TIME, 0)
  ROW(R, hand_qpos_noMD5)
  TERM("hand_qpos", D.nq - 6, OBS_SRC_QPOS, 0)
  ROW(R, hand_qvel)
  ROW(R, obj_pos)
  ROW(R, goal_pos)
  ROW(R, pos_err)
  ROW(R, obj_rot)
  ROW(R, goal_rot)
  ROW(R, rot_err)
  TERM("act", D.na, OBS_SRC_ACT, 0)
  t.dim = R.dim;
}
static const TaskHooks die_hooks = {die_configure, launch_task_obs<DieTask>, launch_task_post<DieTask>, RWD_COLS(rwd_die), obs_terms_die};

#endif  // MYO_TASK_DIE_H
