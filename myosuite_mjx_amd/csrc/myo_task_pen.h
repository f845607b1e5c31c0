// myo_task_pen.h -- PenTwirl{Fixed,Random}EnvV0 (envs/myo/myobase/pen_v0.py) observation / reward / done / solved, MYO_TASK_PEN.
//
// The model (myohand_pen) is of the TrackEnv class (the pen's condim-4 pairs), so, as for the key turn, this kernel runs its own forward
// kinematics of what the task reads, from the post-step qpos: five sites (object top / bottom, target top / bottom, eps_ball) and the
// object body's origin, one lane each.  The target is world-welded: its sites are static and turn with the per-env orientation of
// MYO_F_BODYQUAT.  One 64-lane workgroup per env.
#ifndef MYO_TASK_PEN_H
#define MYO_TASK_PEN_H

// pen_v0.py:98-170 (+ act, base_v0.py:34-38).  Row: hand qpos, object position, object qvel * dt, obj_rot, obj_des_rot, obj_err_pos = object
// position - eps_ball, obj_err_rot = obj_rot - obj_des_rot, act.  T.tip_site = object top, object bottom, target top, target bottom,
// eps_ball; T.tip_lpos = the object body's origin in the frame of the link of the last dof.
struct PenRow {
  int nq, na;
  Blk hand_jnt = {0, nq - 6}, obj_pos = hand_jnt.then(3), obj_vel = obj_pos.then(6), obj_rot = obj_vel.then(3), obj_des_rot = obj_rot.then(3),
      obj_err_pos = obj_des_rot.then(3), obj_err_rot = obj_err_pos.then(3), act = obj_err_rot.then(na);
  int dim = act.end();
};
__device__ __forceinline__ void pen_obs_body(const DevModel& M, const DevBatch& Bt, const TaskDev& T, int obs_only, const int e, const int lane) {
  const int nv = M.nv, nh = nv - 6;
  const PenRow R{nv, M.na_obs};   // nq == nv (pen_configure)
  const auto [o, q, v, a, dt] = task_row(M, Bt, T, e, nv);
  float p[3] = {0.f, 0.f, 0.f}, x[6][3];
  if (lane < 6) {   // lanes 0-4: the sites, 5: the object body's origin
    const int s = lane < 5 ? T.tip_site[lane] : 0;
    const int link = lane < 5 ? M.site_link[s] : M.dof_link[nv - 1];
    link_point_pos(M, Bt, q, e, link, lane < 5 ? M.site_lpos + 3 * s : T.tip_lpos, p);
    // a static site of the per-env oriented body
    if (Bt.bquat && lane < 5 && link < 0 && Bt.bq_flag[M.ncg + s]) body_rot_point({Bt.bquat + 4 * (size_t)e, Bt.bq_c, nullptr}, p);
  }
  site_gather<6>(M, Bt, e, lane, 5, p, x);
  const int so_t = T.tip_site[0], so_b = T.tip_site[1], st_t = T.tip_site[2], st_b = T.tip_site[3];
  float lo[3], lt[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { lo[k] = M.site_lpos[3 * so_t + k] - M.site_lpos[3 * so_b + k]; lt[k] = M.site_lpos[3 * st_t + k] - M.site_lpos[3 * st_b + k]; }
  const float plen = norm3(lo), tlen = norm3(lt);   // pen_v0.py:73-80: from the model's site_pos (rotation invariant)
  float rot[3], drot[3], epos[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { rot[k] = (x[0][k] - x[1][k]) / plen; drot[k] = (x[2][k] - x[3][k]) / tlen; epos[k] = x[5][k] - x[4][k]; }
  if (lane < 3) {
    o[R.obj_pos.at + lane] = x[5][lane];
    o[R.obj_rot.at + lane] = rot[lane];
    o[R.obj_des_rot.at + lane] = drot[lane];
    o[R.obj_err_pos.at + lane] = epos[lane];
    o[R.obj_err_rot.at + lane] = rot[lane] - drot[lane];
  }
  for (int i = lane; i < nv; i += 64) {
    if (i < nh) o[R.hand_jnt.at + i] = q[i];
    else o[R.obj_vel.at + (i - nh)] = v[i] * dt;
  }
  const float act2 = act_sq(M, a, lane, o + R.act.at);
  if (obs_only) return;
  const float actn = act_norm(M, act2);
  if (lane == 0) {
    const float pos_align = norm3(epos);
    float np = norm3(rot) * norm3(drot);
    if (np == 0.f) np = 1.f;                       // vector_math.calculate_cosine
    const float rot_align = dot3(rot, drot) / np;
    const bool dropped = pos_align > T.far_th;
    const float near = pos_align < T.far_th ? 1.f : 0.f;
    const float bonus = (rot_align > 0.9f ? 1.f : 0.f) * near + 5.f * (rot_align > 0.95f ? 1.f : 0.f) * near;
    const float solved = (rot_align > T.pose_thd && !dropped) ? 1.f : 0.f, done = dropped ? 1.f : 0.f;
    if (Bt.rwd) rwd_row(Bt, e, {-pos_align, rot_align, -actn, -done, bonus, -pos_align + rot_align, solved, done});   // pen_v0.py:150-167
    else Bt.reward[e] = T.w_pose * (-pos_align) + T.w_reach * rot_align + T.w_act_reg * (-actn) + T.w_penalty * (dropped ? -1.f : 0.f) + T.w_bonus * bonus;
    Bt.solved[e] = solved;
    Bt.done[e] = done;
  }
}

using PenTask = StateObs<pen_obs_body>;
// pen_v0.py: the pen is the model's last six joints, 3 slides + 3 hinges of one root body; sites = object top / bottom, target top / bottom,
// eps_ball
static int pen_configure(myo_batch* b, const myo_task_config* c) {
  const myo_model* m = b->model;
  const int nv = m->dm.nv;
  if (!trk_model(m) || nv < 7) return fail(MYO_E_UNSUPPORTED, "pen task: a TrackEnv-class model without free / ball joints whose last six joints are the pen's");
  if (object_link_6dof(m) < 0) return fail(MYO_E_UNSUPPORTED, "pen task: the last six joints must be 3 slides + 3 hinges of one root body");
  if (c->ntip != 5 || c->ntarget != 0) return fail(MYO_E_ARG, "pen task: ntip = 5 (object top, object bottom, target top, target bottom, eps_ball) and ntarget = 0");
  if (!sites_in_range(m, c, 5)) return fail(MYO_E_ARG, "pen task: site id out of range");
  for (int k = 0; k < 3; k++) if (!std::isfinite(c->tip_lpos[k])) return fail(MYO_E_ARG, "pen task: tip_lpos must be finite");
  if (!(c->far_th > 0.f) || !is_number(c->pose_thd)) return fail(MYO_E_ARG, "pen task: far_th > 0, pose_thd a number");
  b->task.obs_dim = PenRow{m->nq, m->dm.na_obs}.dim;
  return MYO_OK;
}
static const char* const rwd_pen[] = {"pos_align", "rot_align", "act_reg", "drop", "bonus", RWD_TAIL};   // pen_v0.py:150-167
static void obs_terms_pen(const ObsDims& D, ObsTable& t) {       // pen_v0.py get_obs_dict
  const PenRow R{D.nq, D.na};
  TERM("time", 1, OBS_SRC_TIME, 0)
  ROW(R, hand_jnt)
  ROW(R, obj_pos)
  TERM("obj_des_pos", 3, OBS_SRC_CONST, 0)
  ROW(R, obj_vel)
  ROW(R, obj_rot)
  ROW(R, obj_des_rot)
  ROW(R, obj_err_pos)
  ROW(R, obj_err_rot)
  ROW(R, act)
  t.dim = R.dim;
}
static const TaskHooks pen_hooks = {pen_configure, launch_task_obs<PenTask>, launch_task_post<PenTask>, RWD_COLS(rwd_pen), obs_terms_pen};

#endif  // MYO_TASK_PEN_H
