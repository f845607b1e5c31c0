// myo_task_walk.h -- WalkEnvV0 / TerrainEnvV0 (envs/myo/myobase/walk_v0.py; myoLegWalk, the terrain walk ids), MYO_TASK_WALK, on the host.
// The task's observation, reward and done are a fused pass of the large step kernel (myo_wave_motion.h), so there is no observation body
// here: only the configure of myo_batch_configure_walk, which has a config record of its own, and the hook that runs that pass.
#ifndef MYO_TASK_WALK_H
#define MYO_TASK_WALK_H

static int walk_configure(myo_batch* b, const myo_walk_config* c) {
  if (b->bm_on) return fail(MYO_E_UNSUPPORTED, "per-env body masses: the walk task uses model-wide mass totals");
  if (b->db.rwd && rwd_cols(MYO_TASK_WALK).n != b->db.rwd_n) return fail(MYO_E_ARG, "reward terms are enabled for a task with other columns");
  const myo_model* m = b->model;
  const DevModel& dm = m->dm;
  const int nq = m->nq, nv = dm.nv, nu = dm.nu, nb = (int)m->body_link.size();
  if (!(m->wave_ok && m->wave_cfg == 1 && m->dw.has_free)) return fail(MYO_E_UNSUPPORTED, "walk task needs a free-floating model on the large wave kernel");
  const int bodies[4] = {c->body_talus_l, c->body_talus_r, c->body_pelvis, c->body_torso};
  for (int k = 0; k < 4; k++) if (bodies[k] < 1 || bodies[k] >= nb || m->body_link[bodies[k]] < 0) return fail(MYO_E_ARG, "walk task: bad body id");
  if (m->body_link[c->body_torso] != 0) return fail(MYO_E_UNSUPPORTED, "walk task: torso must be welded to the free root body");
  const int qa[6] = {c->qadr_hip_flexion_l, c->qadr_hip_flexion_r, c->qadr_joint_angle[0], c->qadr_joint_angle[1], c->qadr_joint_angle[2], c->qadr_joint_angle[3]};
  for (int k = 0; k < 6; k++) if (qa[k] < 0 || qa[k] >= nq) return fail(MYO_E_ARG, "walk task: bad qpos address");
  if (c->frame_skip <= 0 || c->hip_period <= 0 || !c->init_qpos) return fail(MYO_E_ARG, "walk task: frame_skip, hip_period, init_qpos required");
  DevWalk w{};
  w.obs_dim = WalkRow{nq, nv, nu}.dim;
  if (w.obs_dim > b->obs_alloc) return fail(MYO_E_ARG, "obs_dim too large");
  w.hip_period = c->hip_period; w.dt = (float)c->frame_skip * dm.timestep;
  w.min_height = c->min_height; w.max_rot = c->max_rot; w.target_x_vel = c->target_x_vel; w.target_y_vel = c->target_y_vel;
  for (int k = 0; k < 4; k++) { w.target_rot[k] = c->target_rot[k]; w.lquat_tor[k] = m->body_lquat[4 * c->body_torso + k]; w.qadr_ja[k] = c->qadr_joint_angle[k]; }
  w.link_tl = m->body_link[c->body_talus_l]; w.link_tr = m->body_link[c->body_talus_r];
  w.link_pel = m->body_link[c->body_pelvis]; w.link_tor = m->body_link[c->body_torso];
  for (int k = 0; k < 3; k++) {
    w.lpos_tl[k] = m->body_lpos[3 * c->body_talus_l + k]; w.lpos_tr[k] = m->body_lpos[3 * c->body_talus_r + k];
    w.lpos_pel[k] = m->body_lpos[3 * c->body_pelvis + k]; w.static_mcom[k] = m->mass[1 + k];
  }
  w.qadr_hfl = c->qadr_hip_flexion_l; w.qadr_hfr = c->qadr_hip_flexion_r;
  w.w_vel = c->w_vel_reward; w.w_done = c->w_done; w.w_cyc = c->w_cyclic_hip; w.w_rot = c->w_ref_rot; w.w_ja = c->w_joint_angle_rew;
  w.mass_total = m->mass[0];
  w.knee_height = c->knee_height;
  if (c->terrain != MYO_TERRAIN_NONE && !(m->dw.hf.on && m->dw.hf.nrow == 100 && m->dw.hf.ncol == 100))
    return fail(MYO_E_UNSUPPORTED, "terrain walk needs a model with a colliding 100 x 100 height field");
  if (c->terrain < 0 || c->terrain > MYO_TERRAIN_STAIRS) return fail(MYO_E_ARG, "walk task: bad terrain kind");
  if (const int rc = copy_to_device(m->device, b->d_walk, &w, sizeof w)) return rc;
  HIPCHK(hipMemcpy(b->d_init, c->init_qpos, (size_t)nq * 4, hipMemcpyHostToDevice));
  if (c->init_qvel) HIPCHK(hipMemcpy(b->d_initv, c->init_qvel, (size_t)nv * 4, hipMemcpyHostToDevice));
  TaskDev& T = b->task;
  T.task = MYO_TASK_WALK; T.frame_skip = c->frame_skip; T.reset_random = 0; T.target_generate = 0; T.ntarget = 0; T.ntip = 0; T.target_floor = -1;
  T.obs_dim = w.obs_dim;
  T.init_qvel = c->init_qvel ? b->d_initv : nullptr;
  T.init_qpos_alt = nullptr; T.init_qvel_alt = nullptr; T.reset_noise_std = 0.f;
  if (c->init_qpos_alt) {
    HIPCHK(hipMemcpy(b->d_init2, c->init_qpos_alt, (size_t)nq * 4, hipMemcpyHostToDevice));
    T.init_qpos_alt = b->d_init2; T.reset_noise_std = c->reset_noise_std;
    if (c->init_qvel_alt) { HIPCHK(hipMemcpy(b->d_initv2, c->init_qvel_alt, (size_t)nv * 4, hipMemcpyHostToDevice)); T.init_qvel_alt = b->d_initv2; }
  }
  T.terrain = c->terrain; T.hf_n = c->terrain ? m->dw.hf.nrow * m->dw.hf.ncol : 0; T.terrain_lo = c->terrain_scalar_lo; T.terrain_hi = c->terrain_scalar_hi;
  return MYO_OK;
}

// the walk observation lives in the step kernel: run it with zero substeps as an observation-only pass (in myo_bench_rollout the step
// launch itself observes)
static int walk_obs(myo_batch* b, hipStream_t s, int obs_only, int reset_only) {
  return launch_step(b, nullptr, MYO_ACTMAP_NONE, 0, s, KF_AUX | (obs_only ? KF_OBS_ONLY : 0) | (reset_only ? KF_RESET_ONLY : 0));
}
static const char* const rwd_walk[] = {"vel_reward", "cyclic_hip", "ref_rot", "joint_angle_rew", "act_mag", RWD_TAIL};   // walk_v0.py:298-311
static void obs_terms_walk(const ObsDims& D, ObsTable& t) {      // walk_v0.py WalkEnvV0 get_obs_dict (TerrainEnvV0 inherits it); WalkRow: myo_common.h
  const WalkRow R{D.nq, D.nv, D.nu};
  TERM("t", 1, OBS_SRC_TIME, 0)
  TERM("time", 1, OBS_SRC_TIME, 0)
  ROW(R, qpos_without_xy)
  ROW(R, qvel)
  ROW(R, com_vel)
  ROW(R, torso_angle)
  ROW(R, feet_heights)
  ROW(R, height)
  ROW(R, feet_rel_positions)
  ROW(R, phase_var)
  ROW(R, muscle_length)
  ROW(R, muscle_velocity)
  ROW(R, muscle_force)
  ROW(R, act)
  t.dim = R.dim;
}
static const TaskHooks walk_hooks = {nullptr, walk_obs, nullptr, RWD_COLS(rwd_walk), obs_terms_walk};

#endif  // MYO_TASK_WALK_H
