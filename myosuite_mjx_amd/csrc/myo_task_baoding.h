// myo_task_baoding.h -- BaodingEnvV1 (envs/myo/myochallenge/baoding_v1.py) observation / reward / done / solved, MYO_TASK_BAODING.
//
// The model (myohand_baoding) is of the TrackEnv class (the balls' condim-4 pairs), so, as for the key turn and the pen, this kernel runs
// its own forward kinematics of what the task reads, from the post-step qpos: the two ball sites (free joints: pose straight from qpos)
// and the two moving targets, one lane each.  The targets follow the reference's goal trajectory analytically: env step k (MYO_F_ELAPSED)
// uses goal[k - 1], so no per-step host work is needed.  One 64-lane workgroup per env.
#ifndef MYO_TASK_BAODING_H
#define MYO_TASK_BAODING_H

// baoding_v1.py:147-246.  Row, in the order of its DEFAULT_OBS_KEYS: hand qpos (the balls' two free joints come last), ball1 position, ball1
// linear qvel * dt, ball2 position, ball2 linear qvel * dt, target1, target2, target1 - ball1, target2 - ball2 (47 floats for
// myohand_baoding; act is not observed).  T.tip_site = ball1, ball2, target1, target2; Bt.target row = start angle, sign, x radius, y
// radius, period.
struct BaodingRow {
  int nq;
  Blk hand_pos = {0, nq - 14}, object1_pos = hand_pos.then(3), object1_velp = object1_pos.then(3), object2_pos = object1_velp.then(3),
      object2_velp = object2_pos.then(3), target1_pos = object2_velp.then(3), target2_pos = target1_pos.then(3), target1_err = target2_pos.then(3),
      target2_err = target1_err.then(3);
  int dim = target2_err.end();
};
__device__ __forceinline__ void baoding_obs_body(const DevModel& M, const DevBatch& Bt, const TaskDev& T, int obs_only, const int e, const int lane) {
  const int nv = M.nv, nq = nv + 2, nh = nv - 12;
  const BaodingRow R{nq};
  const auto [o, q, v, a, dt] = task_row(M, Bt, T, e, nq);
  float p[3] = {0.f, 0.f, 0.f}, x[4][3];
  if (lane < 4) {
    const int s = T.tip_site[lane];
    if (lane < 2) {   // ball site: its free joint's position + R(quat) site_lpos
      const float* qb = q + nh + 7 * lane;
      float qq[4] = {qb[3], qb[4], qb[5], qb[6]}, Rb[9], w[3];
      const float qn = 1.0f / sqrtf(qq[0] * qq[0] + qq[1] * qq[1] + qq[2] * qq[2] + qq[3] * qq[3]);
      qq[0] *= qn; qq[1] *= qn; qq[2] *= qn; qq[3] *= qn;
      quat2mat(Rb, qq);
      matvec(w, Rb, M.site_lpos + 3 * s);
      p[0] = qb[0] + w[0]; p[1] = qb[1] + w[1]; p[2] = qb[2] + w[2];
    } else {          // target: the goal point goal[k - 1] on its ellipse, in the targets' body frame, carried to the world
      const float* g = Bt.target + (size_t)e * 5;
      const int k = max(Bt.elapsed[e] - 1, 0);
      const float ang = g[1] * 6.283185307179586f * ((float)k * dt / g[4]) + g[0] - (lane == 3 ? 3.141592653589793f : 0.f);
      float sn, cs;
      sincosf(ang, &sn, &cs);
      const float X = g[2] * cs - 0.0125f, Yc = g[3] * sn - 0.07f;
      const float* F = T.bd_frame;
      float lp[3];
#pragma unroll
      for (int c = 0; c < 3; c++) lp[c] = F[6 + 3 * (lane - 2) + c] + F[c] * X + F[3 + c] * Yc;
      link_point_pos(M, Bt, q, e, M.site_link[s], lp, p);
    }
  }
  site_gather<4>(M, Bt, e, lane, 4, p, x);
  if (lane < 3) {
    o[R.object1_pos.at + lane] = x[0][lane];
    o[R.object1_velp.at + lane] = v[nh + lane] * dt;
    o[R.object2_pos.at + lane] = x[1][lane];
    o[R.object2_velp.at + lane] = v[nh + 6 + lane] * dt;
    o[R.target1_pos.at + lane] = x[2][lane];
    o[R.target2_pos.at + lane] = x[3][lane];
    o[R.target1_err.at + lane] = x[2][lane] - x[0][lane];
    o[R.target2_err.at + lane] = x[3][lane] - x[1][lane];
  }
  for (int i = lane; i < nh; i += 64) o[R.hand_pos.at + i] = q[i];
  if (obs_only) return;
  // act_reg (baoding_v1.py:220-222) is a column of the term row only: the registered reward does not weigh it
  const float actn = Bt.rwd ? act_norm(M, act_sq(M, a, lane)) : 0.f;
  if (lane == 0) {
    float d1[3], d2[3];
#pragma unroll
    for (int c = 0; c < 3; c++) { d1[c] = x[2][c] - x[0][c]; d2[c] = x[3][c] - x[1][c]; }
    const float n1 = norm3(d1), n2 = norm3(d2);
    const bool fall = x[0][2] < T.far_th || x[1][2] < T.far_th;
    const float solved = (n1 < T.pose_thd && n2 < T.pose_thd && !fall) ? 1.f : 0.f, done = fall ? 1.f : 0.f;
    if (Bt.rwd) rwd_row(Bt, e, {-n1, -n2, -actn, -(n1 + n2), solved, done});               // baoding_v1.py:239-262
    else Bt.reward[e] = T.w_pose * (-n1) + T.w_reach * (-n2);
    Bt.solved[e] = solved;
    Bt.done[e] = done;
  }
}

using BaodingTask = StateObs<baoding_obs_body>;
// baoding_v1.py: the balls are the model's last two joints, free joints of root bodies (qpos[-14:-7], qpos[-7:]); sites = ball1, ball2,
// target1, target2.  The targets move in the frame of their body (baoding_v1.py:147-181: site_pos), which lowering folds into its link:
// T.bd_frame carries that body's x and y axes and, per target, the body origin lifted by the site's compiled z, in the link frame
static int baoding_configure(myo_batch* b, const myo_task_config* c) {
  const myo_model* m = b->model;
  TaskDev& T = b->task;
  const int nv = m->dm.nv;
  if (!trk_model(m, 2) || nv < 13) return fail(MYO_E_UNSUPPORTED, "baoding task: a TrackEnv-class model whose last two joints are free joints (the balls)");
  const int ball[2] = {root_link_of_dofs(m, nv - 12, 6), root_link_of_dofs(m, nv - 6, 6)};
  if (ball[0] < 0 || ball[1] < 0 || ball[0] == ball[1]) return fail(MYO_E_UNSUPPORTED, "baoding task: the last twelve dofs must be two free joints of root bodies");
  if (c->ntip != 4 || c->ntarget != 5) return fail(MYO_E_ARG, "baoding task: ntip = 4 (ball1, ball2, target1, target2) and ntarget = 5 (goal parameters)");
  if (!sites_in_range(m, c, 4)) return fail(MYO_E_ARG, "baoding task: site id out of range");
  const int tb = m->site_body[c->tip_site[2]], tl = m->site_link[c->tip_site[2]];
  if (m->site_link[c->tip_site[0]] != ball[0] || m->site_link[c->tip_site[1]] != ball[1] || tb != m->site_body[c->tip_site[3]] || tl < 0 || m->body_link[tb] != tl)
    return fail(MYO_E_UNSUPPORTED, "baoding task: the ball sites must be on the balls, both target sites on one moving body");
  if (!is_number(c->far_th) || !is_number(c->pose_thd)) return fail(MYO_E_ARG, "baoding task: far_th (drop_th) and pose_thd (proximity_th) numbers");
  const float* bq = &m->body_lquat[4 * (size_t)tb];
  const double qd[4] = {bq[0], bq[1], bq[2], bq[3]};
  double R[9];
  quat2mat_d(R, qd);
  for (int k = 0; k < 3; k++) { T.bd_frame[k] = (float)R[3 * k]; T.bd_frame[3 + k] = (float)R[3 * k + 1]; }
  for (int t = 0; t < 2; t++) {
    const double z = m->site_pos0[3 * (size_t)c->tip_site[2 + t] + 2];
    for (int k = 0; k < 3; k++) T.bd_frame[6 + 3 * t + k] = (float)(m->body_lpos[3 * (size_t)tb + k] + R[3 * k + 2] * z);
  }
  T.obs_dim = BaodingRow{m->nq}.dim;
  T.target_floor = 1;   // the direction sign: U(-1, 2) rounded down, one of -1, 0, +1
  return MYO_OK;
}
static const char* const rwd_baoding[] = {"pos_dist_1", "pos_dist_2", "act_reg", RWD_TAIL};   // baoding_v1.py:239-262
static void obs_terms_baoding(const ObsDims& D, ObsTable& t) {   // baoding_v1.py get_obs_dict (the positions before the velocities)
  const BaodingRow R{D.nq};
  TERM("time", 1, OBS_SRC_TIME, 0)
  ROW(R, hand_pos)
  ROW(R, object1_pos)
  ROW(R, object2_pos)
  ROW(R, object1_velp)
  ROW(R, object2_velp)
  ROW(R, target1_pos)
  ROW(R, target2_pos)
  ROW(R, target1_err)
  ROW(R, target2_err)
  TERM("act", D.na, OBS_SRC_ACT, 0)
  t.dim = R.dim;
}
static const TaskHooks baoding_hooks = {baoding_configure, launch_task_obs<BaodingTask>, launch_task_post<BaodingTask>, RWD_COLS(rwd_baoding), obs_terms_baoding};

#endif  // MYO_TASK_BAODING_H
