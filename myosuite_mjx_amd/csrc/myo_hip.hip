// myo_hip.hip -- MI355X (gfx950) batched musculoskeletal stepper: kernels + C ABI (include/myo_hip.h).
//
// One translation unit, split over csrc/ for readability:
//   myo_common.h        limits, device-side structs (model tables, per-env batch arrays, task records), vector math
//   myo_physics.h       tendon wrapping, muscle model, action map (+ muscle conditions), impedance, contact frames, MPR
//   myo_task_track.h    MyoDM TrackEnv as a fused task of the TRK step kernel: reference lookup, reward / done, masked reset
//   myo_kernel_lanes.h  step_kernel<G>: the first kernel, G = 16 / 32 / 64 lanes per env, all state in LDS (cross-check / fallback)
//   myo_kernel_wave.h   step_kernel_w: one env per 64-lane wavefront (default): LDS layout, substep scheduler, size specialisations, the kernel body
//   myo_wave_util.h     its cross-lane / register helpers, WaveCfg (what the template parameters imply), con_row, the stage context
//   myo_wave_motion.h   its stages: state check, kinematics, tendons and muscles, CRB + RNE, integration
//   myo_wave_collision.h   broad phase, narrow phase
//   myo_wave_solver.h   constraint rows, packed mass matrix, sensor readout, task epilogues (the solver itself is inline in the kernel)
//   myo_ldl_mfma.h      dense LDL^T of the Newton Hessian on the FP32 matrix cores (included by myo_wave_util.h)
//   myo_kernels_aux.h   RNG, placement hint, random actions, policy inference, reset, task_obs_kernel / task_post_kernel
//   myo_kernels_ppo.h   PPO training: policy sampling with log-probabilities, GAE (include/myo_hip_ppo.h)
//   myo_kernels_learner.h  the PPO SGD step: both MLPs forward and backward on the FP32 MFMA, loss, Adam (include/myo_hip_ppo.h)
//   myo_host.h          host records: myo_model, myo_batch, the per-task hook record (TaskHooks) and its generic launchers
//   myo_task_util.h     what the task files share: link-chain walk, row prologue, site gather, activation term, the common configure checks
//   myo_task_<name>.h   pose, reach, stand, hold, keyturn, pen, baoding, die, myodm: a task's observation body, its configure checks and its hook record
//   myo_host_model.h    myo_model_load in pieces: blob view, table upload, packing of the per-lane records, kernel class
//   myo_host_batch.h    batch creation, the per-env override records, the table of fields behind myo_batch_field / read / write
//   myo_rewards.h       reward-term rows and episode statistics: column table per task, walk term kernel, statistics kernel, entry points
//   myo_kernel_forward.h   forward_kernel_w: frames and contact list without a step (include/myo_hip_forward.h), its export tables and buffers
//   myo_hip.hip         host side: task configuration, the table of step-kernel instantiations, launches, the task table, the extern "C" entry points
//
// Execution model: one environment = one wavefront = one workgroup; the whole working set of an env (link
// frames, sparse tendon Jacobian rows, spatial inertias, mass matrix, contact rows, Newton vectors) lives in that wave's LDS slice
// and registers for all substeps of an env step; HBM is read once (state + action) and written once (state, observation).
// Model constants are read through the scalar / L1 caches from the DevModel tables produced by myosuite_mjx_amd/lowering.py.
//
// Physics restated per substep (reference: third-party MuJoCo reached at myosuite/physics/mj_sim_scene.py:55; algorithms per
// MuJoCo documentation [3P]): kinematics -> spatial tendons w/ wrapping -> muscle FLV forces -> CRB mass matrix + RNE bias ->
// collision -> limit / equality / contact rows -> Newton solver -> semi-implicit Euler with implicit joint damping.
#include "myo_common.h"
#include "myo_physics.h"
#include "myo_task_track.h"
#include "myo_kernel_lanes.h"
#include "myo_kernel_wave.h"
#include "myo_kernels_aux.h"
#include "myo_kernels_ppo.h"
#include "myo_kernels_learner.h"
#include "myo_host.h"
#include "myo_task_util.h"
#include "myo_task_pose.h"
#include "myo_task_reach.h"
#include "myo_task_stand.h"
#include "myo_task_hold.h"
#include "myo_task_keyturn.h"
#include "myo_task_pen.h"
#include "myo_task_baoding.h"
#include "myo_task_die.h"
#include "myo_task_myodm.h"
#include "myo_host_model.h"
#include "myo_host_batch.h"
#include "myo_rewards.h"
#include "../../include/myo_hip_forward.h"
#include "myo_kernel_forward.h"

extern "C" {

const char* myo_last_error(void) { return g_err.c_str(); }
int myo_version(void) { return 1; }

int myo_model_load(const void* blobv, size_t nbytes, int device, myo_model** out) {
  if (!blobv || !out || nbytes < 16) return fail(MYO_E_ARG, "myo_model_load: bad arguments");
  const Blob B{(const uint8_t*)blobv};
  uint32_t ver;
  memcpy(&ver, B.p + 4, 4);
  if (memcmp(B.p, "MYOB", 4) || ver != 3) return fail(MYO_E_BLOB, "myo_model_load: not a MYOB v3 blob");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MYO_E_HIP, "myo_model_load: no such HIP device (a GPU is required; there is no CPU fallback)");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<myo_model, void (*)(myo_model*)> m(new myo_model(), myo_model_free);   // a failed load frees what it had uploaded
  m->device = device;
  { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess) m->n_cu = prop.multiProcessorCount; }
  int rc = load_model(m.get(), B);
  if (rc || (rc = fwd_model_tables(m.get(), B))) return rc;
  *out = m.release();
  return MYO_OK;
}

void myo_model_free(myo_model* m) {
  if (!m) return;
  for (void* p : m->dev_allocs) (void)hipFree(p);
  delete m;
}

int myo_model_dims(const myo_model* m, myo_dims* out) {
  if (!m || !out) return fail(MYO_E_ARG, "myo_model_dims: null");
  *out = m->dims;
  return MYO_OK;
}

int myo_model_nsensor(const myo_model* m) { return m ? m->dw.ntouch : 0; }

int myo_model_set_switch(myo_model* m, int dc, int dl, int de) {
  if (!m) return fail(MYO_E_ARG, "null model");
  m->dm.disable_contact = dc; m->dm.disable_limit = dl; m->dm.disable_ellipsoid = de;
  if (m->d_dm) { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipMemcpy(m->d_dm, &m->dm, sizeof(DevModel), hipMemcpyHostToDevice)); }
  return MYO_OK;
}

// batches, per-env fields and overrides: myo_host_batch.h
int myo_batch_create(const myo_model* m, int B, myo_batch** out) { return m && out && B > 0 ? batch_create(m, B, out) : fail(MYO_E_ARG, "myo_batch_create: bad arguments"); }
void myo_batch_free(myo_batch* b) { batch_free(b); }
int myo_batch_enable_sensors(myo_batch* b) { return b ? enable_sensors(b) : fail(MYO_E_ARG, "myo_batch_enable_sensors: null"); }
int myo_batch_field(myo_batch* b, int field, void** p, size_t* pitch, size_t* width) { return b && p && pitch && width ? batch_field(b, field, p, pitch, width) : fail(MYO_E_ARG, "myo_batch_field: null"); }
int myo_batch_read(myo_batch* b, int field, void* host, size_t nbytes) { return b && host ? batch_read(b, field, host, nbytes) : fail(MYO_E_ARG, "myo_batch_read: null"); }
int myo_batch_write(myo_batch* b, int field, const void* host, size_t nbytes) { return b && host ? batch_write(b, field, host, nbytes) : fail(MYO_E_ARG, "myo_batch_write: null"); }

int myo_batch_size(const myo_batch* b) { return b ? b->db.B : 0; }

static const TaskHooks* task_hooks(int task);       // (below, after the launches the hooks make)

int myo_batch_configure(myo_batch* b, const myo_task_config* c) {
  if (!b || !c) return fail(MYO_E_ARG, "myo_batch_configure: null");
  if (b->bm_on && c->task == MYO_TASK_STAND) return fail(MYO_E_UNSUPPORTED, "per-env body masses: the stand task uses model-wide mass totals");
  const DevModel& dm = b->model->dm;
  TaskDev& T = b->task;
  int nv = dm.nv, nu = dm.nu;
  if (c->ntarget > b->ntarget_alloc || c->ntip > 8) return fail(MYO_E_ARG, "myo_batch_configure: ntarget/ntip too large");
  if (c->quat_body > 0) { int rc = set_quat_body(b, c->quat_body); if (rc) return rc; }
  if (c->task == MYO_TASK_WALK) return fail(MYO_E_ARG, "use myo_batch_configure_walk for the walk task");
  if (b->db.rwd && rwd_cols(c->task).n != b->db.rwd_n) return fail(MYO_E_ARG, "reward terms are enabled for a task with other columns");
  T.init_qvel = nullptr; T.rnd = nullptr;
  T.terrain = 0; T.hf_n = 0;
  for (int k = 0; k < 3; k++) T.tip_lpos[k] = c->tip_lpos[k];
  if (c->reset_noise_lo || c->reset_noise_hi || c->reset_clip_lo || c->reset_clip_hi) {
    if (!(c->reset_noise_lo && c->reset_noise_hi && c->reset_clip_lo && c->reset_clip_hi)) return fail(MYO_E_ARG, "reset noise: all four arrays or none");
    const float* src[4] = {c->reset_noise_lo, c->reset_noise_hi, c->reset_clip_lo, c->reset_clip_hi};
    for (int k = 0; k < 4; k++) HIPCHK(hipMemcpy(b->d_rnd + (size_t)k * b->model->nq, src[k], (size_t)b->model->nq * 4, hipMemcpyHostToDevice));
    T.rnd = b->d_rnd;
  }
  if (c->init_qvel) { HIPCHK(hipMemcpy(b->d_initv, c->init_qvel, (size_t)nv * 4, hipMemcpyHostToDevice)); T.init_qvel = b->d_initv; }
  T.task = c->task; T.frame_skip = c->frame_skip; T.reset_random = c->reset_random; T.target_generate = c->target_generate;
  T.ntarget = c->ntarget; T.ntip = c->ntip;
  for (int i = 0; i < 8; i++) T.tip_site[i] = c->tip_site[i];
  T.pose_thd = c->pose_thd; T.far_th = c->far_th; T.near_th = c->near_th;
  T.w_pose = c->w_pose; T.w_bonus = c->w_bonus; T.w_act_reg = c->w_act_reg; T.w_penalty = c->w_penalty; T.w_reach = c->w_reach;
  T.nq = b->model->nq;
  const TaskHooks* hooks = task_hooks(c->task);
  if (hooks && hooks->configure) { int rc = hooks->configure(b, c); if (rc) return rc; }
  else T.obs_dim = 0;
  if (T.obs_dim > b->obs_alloc) return fail(MYO_E_ARG, "obs_dim too large");
  if (c->ntarget > 0) {
    if (!c->target_lo) return fail(MYO_E_ARG, "target_lo required");
    HIPCHK(hipMemcpy(b->d_tlo, c->target_lo, c->ntarget * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->d_thi, c->target_hi ? c->target_hi : c->target_lo, c->ntarget * 4, hipMemcpyHostToDevice));
  }
  if (c->reset_random && b->model->nq != nv) return fail(MYO_E_ARG, "reset_random needs a model without free / ball joints");
  HIPCHK(hipMemcpy(b->d_init, c->init_qpos ? c->init_qpos : b->model->qpos0.data(), b->model->nq * 4, hipMemcpyHostToDevice));
  return MYO_OK;
}

int myo_batch_set_geom_override(myo_batch* b, int geom_id, const float* lo, const float* hi) {
  if (!b) return fail(MYO_E_ARG, "myo_batch_set_geom_override: null");
  const myo_model* m = b->model;
  if (!lo || !hi) { b->task.gsize_type = 0; b->db.gsize_cg = -1; return MYO_OK; }
  if (!(m->wave_ok && m->wave_cfg == 1) || m->leg_sizes || m->dw.hf.on) return fail(MYO_E_UNSUPPORTED, "geom override: generic large-kernel models only");
  int cg = -1;
  for (size_t i = 0; i < m->cg_geom.size(); i++) if (m->cg_geom[i] == geom_id) cg = (int)i;
  if (cg < 0) return fail(MYO_E_ARG, "geom override: not a collision geom of this model");
  const int ty = m->cg_type_h[cg];
  if (ty != GEOM_SPHERE && ty != GEOM_CAPSULE && ty != GEOM_ELLIPSOID && ty != GEOM_CYLINDER) return fail(MYO_E_UNSUPPORTED, "geom override: sphere / capsule / ellipsoid / cylinder geoms only");
  if (!b->db.gsize) {
    int rc = balloc(b, (void**)&b->db.gsize, (size_t)b->db.B * 4 * 4);
    if (rc) return rc;
  }
  b->db.gsize_cg = cg;
  b->task.gsize_type = ty;
  for (int k = 0; k < 3; k++) { b->task.gsize_lo[k] = lo[k]; b->task.gsize_hi[k] = hi[k]; }
  return MYO_OK;
}

int myo_batch_configure_walk(myo_batch* b, const myo_walk_config* c) {
  if (!b || !c) return fail(MYO_E_ARG, "myo_batch_configure_walk: null");
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
  w.obs_dim = (nq - 2) + nv + 16 + 4 * nu;
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
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(b->d_walk, &w, sizeof w, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_init, c->init_qpos, (size_t)nq * 4, hipMemcpyHostToDevice));
  if (c->init_qvel) HIPCHK(hipMemcpy(b->d_initv, c->init_qvel, (size_t)nv * 4, hipMemcpyHostToDevice));
  TaskDev& T = b->task;
  T.task = MYO_TASK_WALK; T.frame_skip = c->frame_skip; T.reset_random = 0; T.target_generate = 0; T.ntarget = 0; T.ntip = 0;
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

int myo_batch_configure_track(myo_batch* b, const myo_track_config* c) {
  if (!b || !c) return fail(MYO_E_ARG, "myo_batch_configure_track: null");
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
  DevTrack K{};
  K.ref_type = c->ref_type; K.horizon = c->horizon; K.robot_horizon = c->robot_horizon; K.object_horizon = c->object_horizon;
  K.robot_dim = c->robot_dim; K.object_dim = c->object_dim; K.has_vel = c->ref_robot_vel != nullptr;
  K.extrapolate = c->motion_extrapolation; K.linear = c->interpolation_linear; K.autoreset = c->autoreset;
  K.term_obj = c->terminate_obj_fail; K.term_pose = c->terminate_pose_fail; K.start_time = c->motion_start_time; K.max_steps = c->max_episode_steps;
  int rc;
  auto up = [&](const void* src, size_t nbytes, const void** dst) -> int {
    void* p = nullptr;
    if ((rc = balloc(b, &p, nbytes ? nbytes : 8))) return rc;
    if (nbytes) HIPCHK(hipMemcpy(p, src, nbytes, hipMemcpyHostToDevice));
    *dst = p;
    return 0;
  };
  if ((rc = up(c->ref_time, (size_t)c->horizon * 8, (const void**)&K.T))) return rc;
  if ((rc = up(c->ref_robot, (size_t)c->robot_horizon * c->robot_dim * 8, (const void**)&K.robot))) return rc;
  if (K.has_vel) { if ((rc = up(c->ref_robot_vel, (size_t)c->robot_horizon * c->robot_dim * 8, (const void**)&K.robot_vel))) return rc; } else K.robot_vel = nullptr;
  if ((rc = up(c->ref_object, (size_t)c->object_horizon * c->object_dim * 8, (const void**)&K.object))) return rc;
  if ((rc = up(c->init_qpos, (size_t)nq * 4, (const void**)&K.init_qpos)) || (rc = up(c->ctrl_lo, (size_t)nu * 4, (const void**)&K.lo)) ||
      (rc = up(c->ctrl_hi, (size_t)nu * 4, (const void**)&K.hi))) return rc;
  K.obj_link = c->object_link; K.wrist_link = c->wrist_link;
  for (int k = 0; k < 3; k++) { K.obj_p[k] = c->object_ipos[k]; K.wrist_p[k] = c->wrist_ipos[k]; }
  for (int k = 0; k < 9; k++) K.obj_R[k] = c->object_imat[k];
  K.lift_z = c->lift_z; K.obj_err_scale = c->obj_err_scale; K.base_err_scale = c->base_err_scale; K.lift_bonus_mag = c->lift_bonus_mag;
  K.qpos_w = c->qpos_reward_weight; K.qpos_err_scale = c->qpos_err_scale; K.qvel_w = c->qvel_reward_weight; K.qvel_err_scale = c->qvel_err_scale;
  K.obj_fail2 = c->obj_fail_thresh * c->obj_fail_thresh; K.base_fail2 = c->base_fail_thresh * c->base_fail_thresh; K.qpos_fail = c->qpos_fail_thresh;
  K.w_pose = c->w_pose; K.w_object = c->w_object; K.w_bonus = c->w_bonus; K.w_penalty = c->w_penalty;
  K.ref_pitch = 2 * c->robot_dim + c->object_dim;
  K.seed = c->seed;
  { void* p = nullptr; if ((rc = balloc(b, &p, (size_t)B * K.ref_pitch * 4))) return rc; K.ref = (float*)p; }
  if (!b->d_metrics) { void* p = nullptr; if ((rc = balloc(b, &p, (size_t)B * 4 * 4))) return rc; b->d_metrics = (float*)p; }
  K.metrics = b->d_metrics;
  if (!b->d_track) { void* p = nullptr; if ((rc = balloc(b, &p, sizeof(DevTrack)))) return rc; b->d_track = (DevTrack*)p; }
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

static int launch_reset(myo_batch* b, const uint8_t* mask_dev, uint64_t seed, void* stream, int max_episode_steps) {
  b->reset_seed = seed;
  const DevModel& dm = b->model->dm;
  HIPCHK(hipSetDevice(b->model->device));
  hipLaunchKernelGGL(reset_kernel, dim3(b->db.B), dim3(64), 0, (hipStream_t)stream, b->db, b->task, b->model->nq, dm.nv, dm.nu, dm.qpos0, mask_dev, seed,
                     b->env_offset, max_episode_steps);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

int myo_reset(myo_batch* b, const uint8_t* mask_dev, uint64_t seed, void* stream) {
  if (!b) return fail(MYO_E_ARG, "myo_reset: null");
  return launch_reset(b, mask_dev, seed, stream, 0);
}

int myo_autoreset(myo_batch* b, int max_episode_steps, uint64_t seed, void* stream) {
  if (!b || max_episode_steps <= 0) return fail(MYO_E_ARG, "myo_autoreset: bad arguments");
  return launch_reset(b, nullptr, seed, stream, max_episode_steps);
}

int myo_set_env_offset(myo_batch* b, int env_offset) {
  if (!b) return fail(MYO_E_ARG, "null batch");
  b->env_offset = env_offset;
  b->db.env_offset = env_offset;
  return MYO_OK;
}

int myo_set_state(myo_batch* b, const float* qpos, const float* qvel, const float* act, const float* time, void* stream) {
  if (!b) return fail(MYO_E_ARG, "myo_set_state: null");
  const DevModel& dm = b->model->dm;
  size_t B = b->db.B;
  hipStream_t s = (hipStream_t)stream;
  if (qpos) HIPCHK(hipMemcpyAsync(b->db.qpos, qpos, B * b->model->nq * 4, hipMemcpyDeviceToDevice, s));
  if (qvel) HIPCHK(hipMemcpyAsync(b->db.qvel, qvel, B * dm.nv * 4, hipMemcpyDeviceToDevice, s));
  if (act) HIPCHK(hipMemcpyAsync(b->db.act, act, B * dm.nu * 4, hipMemcpyDeviceToDevice, s));
  if (time) HIPCHK(hipMemcpyAsync(b->db.time, time, B * 4, hipMemcpyDeviceToDevice, s));
  return MYO_OK;
}

// The instantiations of step_kernel_w<NVT, KC, NC, NTR, WPE, SCHED, SPEC, HF, TRK, RK4>, each with its template arguments and the name
// rocprofv3 prints for it (myo_bench_last_kernel_name; bench.py reports it next to the kernel time).  The per-device attribute pass, the
// name and the launch all come from this one list.
#define MYO_WAVE_KERNELS(X)                                                                                             \
  X(WK_HAND, "step_kernel_w<24,8,32,1,3,false,0,false>", 24, 8, 32, 1, 3, false, 0)                                      \
  X(WK_HAND_SPEC, "step_kernel_w<24,8,32,1,4,false,1,false>", 24, 8, 32, 1, 4, false, 1)                                 \
  X(WK_LEG, "step_kernel_w<36,20,32,2,2,false,0,false>", 36, 20, 32, 2, 2, false, 0)                                     \
  X(WK_LEG_SCHED, "step_kernel_w<36,20,32,2,2,true,0,false>", 36, 20, 32, 2, 2, true, 0)                                 \
  X(WK_LEG_SPEC_SCHED, "step_kernel_w<36,20,32,2,2,true,2,false>", 36, 20, 32, 2, 2, true, 2)                            \
  X(WK_LEG_SPEC, "step_kernel_w<36,20,32,2,2,false,2,false>", 36, 20, 32, 2, 2, false, 2)                                \
  X(WK_TERRAIN, "step_kernel_w<36,20,32,2,2,false,0,true>", 36, 20, 32, 2, 2, false, 0, true)                            \
  X(WK_TERRAIN_SPEC_SCHED, "step_kernel_w<36,20,32,2,2,true,3,true>", 36, 20, 32, 2, 2, true, 3, true)                   \
  X(WK_TERRAIN_SPEC, "step_kernel_w<36,20,32,2,2,false,3,true>", 36, 20, 32, 2, 2, false, 3, true)                       \
  X(WK_TRK, "step_kernel_w<36,20,32,2,2,false,0,false,true>", 36, 20, 32, 2, 2, false, 0, false, true)                   \
  X(WK_HAND_RK4, "step_kernel_w<24,8,32,1,3,false,0,false,false,true>", 24, 8, 32, 1, 3, false, 0, false, false, true)   \
  X(WK_LEG_RK4, "step_kernel_w<36,20,32,2,2,false,0,false,false,true>", 36, 20, 32, 2, 2, false, 0, false, false, true)
struct WaveKernel {
  const char* name;
  void (*fn)(const DevModel*, const DevModelW*, DevBatch, const float*, int, int, long long*, const int*, const DevWalk*, int, SchedDev);
};
enum WaveKernelId {
#define X(id, name, ...) id,
  MYO_WAVE_KERNELS(X)
#undef X
};
static const WaveKernel wave_kernels[] = {
#define X(id, name, ...) {name, step_kernel_w<__VA_ARGS__>},
  MYO_WAVE_KERNELS(X)
#undef X
};

// the instantiation a launch of model m runs: bm = the per-env body-mass override is on (only the run-time-sized instantiations read its
// link tables), sched = the substep scheduler is on (large-kernel models without RK4; terrain models only with their specialised sizes)
static WaveKernelId select_wave_kernel(const myo_model* m, bool bm, bool sched) {
  const bool hand_sizes = m->hand_sizes && !bm, leg_sizes = m->leg_sizes && !bm;
  if (sched) return m->dw.hf.on ? WK_TERRAIN_SPEC_SCHED : (leg_sizes ? WK_LEG_SPEC_SCHED : WK_LEG_SCHED);
  if (m->rk4) return m->wave_cfg == 0 ? WK_HAND_RK4 : WK_LEG_RK4;
  if (m->wave_cfg == 2) return WK_TRK;   // TrackEnv model class
  if (m->wave_cfg == 0) return hand_sizes ? WK_HAND_SPEC : WK_HAND;
  if (m->dw.hf.on) return m->terrain_sizes ? WK_TERRAIN_SPEC : WK_TERRAIN;   // terrain models: the instantiations with the height-field narrow phase
  return leg_sizes ? WK_LEG_SPEC : WK_LEG;
}

// The forward twins (myo_kernel_forward.h): forward_kernel_w<NVT, KC, NC, NTR, WPE, HF, TRK> with the template arguments of the run-time-sized
// step kernel of each size class.  A model the loader routes to a SPEC, SCHED or RK4 step kernel uses the twin of its class.
#define MYO_FORWARD_KERNELS(X)                                       \
  X(FK_HAND, "forward_kernel_w<24,8,32,1,3,false,false>", 24, 8, 32, 1, 3, false, false)       \
  X(FK_LEG, "forward_kernel_w<36,20,32,2,2,false,false>", 36, 20, 32, 2, 2, false, false)      \
  X(FK_TERRAIN, "forward_kernel_w<36,20,32,2,2,true,false>", 36, 20, 32, 2, 2, true, false)    \
  X(FK_TRK, "forward_kernel_w<36,20,32,2,2,false,true>", 36, 20, 32, 2, 2, false, true)
struct ForwardKernel {
  const char* name;
  void (*fn)(const DevModel*, const DevModelW*, DevBatch, FwdDev);
};
enum ForwardKernelId {
#define X(id, name, ...) id,
  MYO_FORWARD_KERNELS(X)
#undef X
};
static const ForwardKernel forward_kernels[] = {
#define X(id, name, ...) {name, forward_kernel_w<__VA_ARGS__>},
  MYO_FORWARD_KERNELS(X)
#undef X
};
static ForwardKernelId select_forward_kernel(const myo_model* m) {
  if (m->wave_cfg == 2) return FK_TRK;
  if (m->wave_cfg == 0) return FK_HAND;
  return m->dw.hf.on ? FK_TERRAIN : FK_LEG;
}

static int launch_forward(myo_batch* b, hipStream_t s) {
  const myo_model* m = b->model;
  int rc = fwd_check(b);
  if (rc || (rc = fwd_start(b))) return rc;
  {  // kernel attributes are per device
    static std::mutex attr_mu;
    static bool attr_dev[64] = {};
    std::lock_guard<std::mutex> attr_lock(attr_mu);
    bool& attr = attr_dev[m->device & 63];
    if (!attr) {
      for (const ForwardKernel& k : forward_kernels) HIPCHK(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      attr = true;
    }
  }
  FwdDev F{};
  F.nbody = m->fwd_nbody; F.nsite = m->fwd_nsite; F.ngeom = m->fwd_ngeom; F.ncap = m->fwd_ncap; F.has_site_mat = m->fwd_site_mat;
  F.bq_body = b->bq_body;
  // die task: the goal offset moves the target body's exported frames.  Only for a target without collision geoms (the collision stages
  // would not move them): otherwise the offset stays out of the frames, as it stays out of the contacts
  bool target_collides = false;
  for (int cb : m->cg_body) if (cb == b->bq_body) target_collides = true;
  F.goal_off = (b->task.task == MYO_TASK_DIE && b->task.ntarget == 3 && b->bq_body > 0 && !target_collides) ? b->db.target : nullptr;
  F.body_rec = (gpf4)(const float4*)m->d_fwd_body; F.site_rec = (gpf4)(const float4*)m->d_fwd_site; F.geom_rec = (gpf4)(const float4*)m->d_fwd_geom;
  F.cg_geom = (gpi)m->d_fwd_cg_geom;
  F.xpos = (float*)b->fwd_buf[MYO_FWD_XPOS]; F.xmat = (float*)b->fwd_buf[MYO_FWD_XMAT]; F.xipos = (float*)b->fwd_buf[MYO_FWD_XIPOS];
  F.site_xpos = (float*)b->fwd_buf[MYO_FWD_SITE_XPOS]; F.site_xmat = (float*)b->fwd_buf[MYO_FWD_SITE_XMAT];
  F.geom_xpos = (float*)b->fwd_buf[MYO_FWD_GEOM_XPOS]; F.geom_xmat = (float*)b->fwd_buf[MYO_FWD_GEOM_XMAT];
  F.contact = (float*)b->fwd_buf[MYO_FWD_CONTACT]; F.ncon = (int*)b->fwd_buf[MYO_FWD_NCON];
  const ForwardKernel& k = forward_kernels[select_forward_kernel(m)];
  hipLaunchKernelGGL(k.fn, dim3(b->db.B), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm, (const DevModelW*)m->d_dw, b->db, F);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

static int launch_step(myo_batch* b, const float* action, int actmap, int nsub, hipStream_t s, int kflags = 0) {
  const myo_model* m = b->model;
  const DevWalk* wk = b->task.task == MYO_TASK_WALK ? b->d_walk : nullptr;
  if (kflags && !(wk && g_lanes == 64)) return fail(MYO_E_ARG, "observation pass: walk task on the wave kernel only");
  // models the wave kernel cannot take fall back to 16 lanes; models only the wave kernel can take always use it
  const int G = (g_lanes == 64 && !m->wave_ok) ? 16 : ((g_lanes != 64 && !m->generic_ok) ? 64 : g_lanes), EPW = 64 / G;
  int grid = (b->db.B + EPW - 1) / EPW;
  size_t lds = (size_t)EPW * m->env_lds_bytes;
  {  // kernel attributes are per device: one flag per device ordinal for the lanes kernels and the reach observation kernel too
    static std::mutex attr_g_mu;
    static bool attr_g_dev[64] = {};
    std::lock_guard<std::mutex> attr_g_lock(attr_g_mu);
    bool& attr_set = attr_g_dev[m->device & 63];
    if (!attr_set) {
      for (const void* k : {(const void*)step_kernel<16>, (const void*)step_kernel<32>, (const void*)step_kernel<64>, (const void*)reach_obs_kernel<16>})
        HIPCHK(hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      attr_set = true;
    }
  }
  long long* st = b->d_stamps;
#if MYO_POISON
  {  // MYO_POISON_MODE (diagnostic build only): bit 0 scratch memory, bit 1 vector registers, bit 2 scalar registers; default all
    static const int pmode = [] { const char* e = getenv("MYO_POISON_MODE"); return e ? atoi(e) : 7; }();
    if (pmode & 1) hipLaunchKernelGGL(scratch_poison_kernel, dim3(16384), dim3(64), 0, s, (float*)b->d_stamps, 0);
    if (pmode & 2) hipLaunchKernelGGL(vgpr_poison_kernel, dim3(8192), dim3(64), 0, s, 0x7fc0dead);
    if (pmode & 4) hipLaunchKernelGGL(sgpr_poison_kernel, dim3(32768), dim3(64), 0, s);
  }
#endif
  if (!(G == 64 && m->wave_ok) && !m->generic_ok)
    return fail(MYO_E_UNSUPPORTED, "this model (tendon limits / free joint / equalities / plane contacts) needs the wave-per-env kernel (lanes = 64)");
  // per-env body masses: link tables of every env recomposed once per launch; the step runs on the run-time-sizes instantiation of the
  // model's class (the only ones that read them)
  if (b->sens_on) { int rc = sens_check(b); if (rc) return rc; }   // (lanes may have changed since the sensors were enabled)
  const bool bm = b->bm_on;
  if (bm) {
    int rc = bm_check(b);
    if (rc) return rc;
    const int n = b->db.B * m->dm.nl;
    hipLaunchKernelGGL(link_compose_kernel, dim3((n + 255) / 256), dim3(256), 0, s, b->db, m->dm.nl, m->d_lm_adr, m->d_lm_body, m->d_lm_tab);
  }
  if (G == 64 && m->wave_ok) {
    // kernel attributes are per device: one flag per device ordinal (a process that opens models on two GPUs)
    static std::mutex attr_mu;
    static bool attr_w_dev[64] = {};
    std::lock_guard<std::mutex> attr_lock(attr_mu);
    bool& attr_w = attr_w_dev[m->device & 63];
    if (!attr_w) {
      for (const WaveKernel& k : wave_kernels) HIPCHK(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      attr_w = true;
    }
    const int* order = nullptr;
    int Bn = b->db.B;
    // substep scheduler: MYO_SCHED=1 forces it, 0 disables it; default (auto) uses it where it was measured to pay: when the launch
    // holds at least twice as many envs as the chip holds waves of this kernel (MyoLeg: 8 waves per CU; +6 % at 4096 envs).  With as
    // many waves as envs every wave just re-takes its own env and only the overhead is left (MyoHand at 4096 envs: -15 %)
    static const int sched_mode = [] { const char* e = getenv("MYO_SCHED"); return e ? atoi(e) : -1; }();   // process-wide configuration (environment)
    const int n_cu = m->n_cu > 0 ? m->n_cu : 256;                                                        // per model = per device
    const int resident = n_cu * (m->wave_cfg == 0 ? 16 : (m->wave_cfg == 1 ? 8 : std::max(1, (160 * 1024) / std::max(1, m->env_lds_bytes_w))));
    const bool sched_ok = !kflags && Bn >= 64 && Bn <= SCHED_ENV_MASK && nsub + (wk ? 1 : 0) <= 15 && nsub > 0;
    const bool sched = sched_ok && !bm && m->wave_cfg == 1 && !m->rk4 && !(m->dw.hf.on && !m->terrain_sizes) && (sched_mode == 1 || (sched_mode == -1 && m->wave_cfg == 1 && Bn >= 2 * resident));
    if (b->balance && Bn >= 1024 && Bn % 4 == 0 && !kflags && !sched) {
      static const int prio_mode = [] { const char* e = getenv("MYO_PRIO"); return e ? atoi(e) : 2; }();
      hipLaunchKernelGGL(balance_kernel, dim3(1), dim3(1024), 0, s, (const int*)b->db.diag, Bn, b->d_order, Bn / 4, prio_mode);
      order = b->d_order;
    }
    // one queue per XCD the device (or its partition) shows: MI355X has 32 CUs per XCD, 8 XCDs in SPX mode (a queue keyed on
    // XCC_ID & 7 would never be drained on a DPX / QPX / CPX partition)
    const int nqueue = std::max(1, std::min(8, n_cu / 32));
    SchedDev S{b->d_sched, b->d_sched + 32, nqueue == 8 ? b->sched_stride : (Bn + nqueue - 1) / nqueue + 1, nsub + (wk ? 1 : 0), nqueue};
    const WaveKernel& k = wave_kernels[select_wave_kernel(m, bm, sched)];
    if (!kflags) b->last_kernel = k.name;
    int wgrid = Bn;
    if (sched) {
      hipLaunchKernelGGL(sched_init_kernel, dim3(1), dim3(1024), 0, s, (const int*)b->db.diag, Bn, S);
      wgrid = Bn < resident ? Bn : resident;    // persistent waves: no more workgroups than the chip holds at once
      static const int grid_override = [] { const char* e = getenv("MYO_SCHED_GRID"); return e ? atoi(e) : 0; }();
      if (grid_override > 0 && grid_override < wgrid) wgrid = grid_override;
    }
    // (order is set only without the scheduler; wk and kflags are null / 0 for every model outside the large-kernel class: the walk task needs wave_cfg == 1)
    hipLaunchKernelGGL(k.fn, dim3(wgrid), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm, (const DevModelW*)m->d_dw, b->db, action, actmap,
                       nsub, st, order, wk, kflags, S);
    HIPCHK(hipGetLastError());
    // walk task with the term row on: the row and MYO_F_REWARD of every launch whose fused pass wrote the reward
    if (wk && b->db.rwd && !(kflags & KF_OBS_ONLY)) return walk_terms_launch(b, s);
    return MYO_OK;
  }
  if (G == 16) hipLaunchKernelGGL(step_kernel<16>, dim3(grid), dim3(64), lds, s, m->dm, b->db, action, actmap, nsub, st);
  else if (G == 32) hipLaunchKernelGGL(step_kernel<32>, dim3(grid), dim3(64), lds, s, m->dm, b->db, action, actmap, nsub, st);
  else hipLaunchKernelGGL(step_kernel<64>, dim3(grid), dim3(64), lds, s, m->dm, b->db, action, actmap, nsub, st);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

int myo_step(myo_batch* b, const float* action_dev, int actmap, int nsubsteps, void* stream) {
  if (!b || nsubsteps < 0) return fail(MYO_E_ARG, "myo_step: bad arguments");
  if (b->task.task == MYO_TASK_TRACK && b->track_flavour == 1 && actmap == MYO_ACTMAP_CTRLRANGE)
    return fail(MYO_E_ARG, "myo_step: MYO_ACTMAP_CTRLRANGE is the MJX TrackEnv's action map; a batch of the classic flavour steps with MYO_ACTMAP_MUSCLE_SIGMOID");
  HIPCHK(hipSetDevice(b->model->device));
  return launch_step(b, action_dev, actmap, nsubsteps, (hipStream_t)stream);
}

// ---- forward pass (include/myo_hip_forward.h; kernel, tables and buffers in myo_kernel_forward.h)
int myo_forward(myo_batch* b, void* stream) {
  if (!b) return fail(MYO_E_ARG, "myo_forward: null");
  HIPCHK(hipSetDevice(b->model->device));
  return launch_forward(b, (hipStream_t)stream);
}

int myo_model_forward_dims(const myo_model* m, int* nbody, int* nsite, int* ngeom, int* ncon_max) {
  if (!m) return fail(MYO_E_ARG, "myo_model_forward_dims: null");
  if (const int rc = fwd_model_check(m)) return rc;
  if (nbody) *nbody = m->fwd_nbody;
  if (nsite) *nsite = m->fwd_nsite;
  if (ngeom) *ngeom = m->fwd_ngeom;
  if (ncon_max) *ncon_max = m->fwd_ncap;
  return MYO_OK;
}

int myo_forward_buffer(myo_batch* b, int which, void** dev_ptr, size_t* pitch, size_t* width) {
  if (!b || !dev_ptr || !pitch || !width) return fail(MYO_E_ARG, "myo_forward_buffer: null");
  if (which < 0 || which >= MYO_FWD_COUNT) return fail(MYO_E_ARG, "myo_forward_buffer: unknown buffer id");
  if (!b->fwd_on) return fail(MYO_E_ARG, "myo_forward_buffer: no forward pass has run on this batch (myo_forward)");
  if (which == MYO_FWD_SITE_XMAT && !b->model->fwd_site_mat) return fail(MYO_E_UNSUPPORTED, "MYO_FWD_SITE_XMAT: the model blob carries no site_quat");
  *dev_ptr = b->fwd_buf[which];
  *pitch = *width = fwd_width(b->model, which);
  return MYO_OK;
}

int myo_forward_read(myo_batch* b, int which, void* host, size_t nbytes) {
  if (!b || !host) return fail(MYO_E_ARG, "myo_forward_read: null");
  void* p; size_t pitch, width;
  const int rc = myo_forward_buffer(b, which, &p, &pitch, &width);
  if (rc) return rc;
  if (nbytes != (size_t)b->db.B * width * 4) return fail(MYO_E_ARG, "myo_forward_read: size mismatch");
  HIPCHK(hipSetDevice(b->model->device));
  HIPCHK(hipDeviceSynchronize());
  if (nbytes) HIPCHK(hipMemcpy(host, p, nbytes, hipMemcpyDeviceToHost));
  return MYO_OK;
}

int myo_forward_host_tables(const void* blobv, size_t nbytes, int table, double* out, size_t capacity, int* n) {
  if (!blobv || nbytes < 16 || !n || table < 0 || table > 2) return fail(MYO_E_ARG, "myo_forward_host_tables: bad arguments");
  const Blob B{(const uint8_t*)blobv};
  uint32_t ver;
  memcpy(&ver, B.p + 4, 4);
  if (memcmp(B.p, "MYOB", 4) || ver != 3) return fail(MYO_E_BLOB, "myo_forward_host_tables: not a MYOB v3 blob");
  FwdTables T;
  const int rc = fwd_build_tables(B, &T);
  if (rc) return rc;
  const std::vector<double>& v = table == 0 ? T.body : (table == 1 ? T.site : T.geom);
  *n = (int)(v.size() / FWD_REC);
  if (out && capacity >= v.size() && !v.empty()) memcpy(out, v.data(), v.size() * sizeof(double));
  return MYO_OK;
}

// the table of all tasks: every record but the walk's sits in its myo_task_<name>.h.  The walk observation lives in the step kernel: run it
// with zero substeps as an observation-only pass (configured by myo_batch_configure_walk; in myo_bench_rollout the step launch itself observes)
static int walk_obs(myo_batch* b, hipStream_t s, int obs_only, int reset_only) {
  return launch_step(b, nullptr, MYO_ACTMAP_NONE, 0, s, KF_AUX | (obs_only ? KF_OBS_ONLY : 0) | (reset_only ? KF_RESET_ONLY : 0));
}
static const TaskHooks walk_hooks = {nullptr, walk_obs, nullptr};

static const TaskHooks* task_hooks(int task) {
  switch (task) {
    case MYO_TASK_POSE: return &pose_hooks;
    case MYO_TASK_REACH: return &reach_hooks;
    case MYO_TASK_WALK: return &walk_hooks;
    case MYO_TASK_STAND: return &stand_hooks;
    case MYO_TASK_HOLD: return &hold_hooks;
    case MYO_TASK_TRACK: return &track_hooks;
    case MYO_TASK_KEYTURN: return &keyturn_hooks;
    case MYO_TASK_PEN: return &pen_hooks;
    case MYO_TASK_BAODING: return &baoding_hooks;
    case MYO_TASK_DIE: return &die_hooks;
    default: return nullptr;   // MYO_TASK_NONE
  }
}

static int launch_obs(myo_batch* b, hipStream_t s, int obs_only = 0, int reset_only = 0) {
  const TaskHooks* hooks = task_hooks(b->task.task);
  if (!hooks) return fail(MYO_E_ARG, "myo_obs: no task configured");
  const int rc = hooks->obs(b, s, obs_only, reset_only);
  if (rc) return rc;
  HIPCHK(hipGetLastError());
  return MYO_OK;
}


int myo_obs(myo_batch* b, void* stream) {
  if (!b) return fail(MYO_E_ARG, "myo_obs: null");
  HIPCHK(hipSetDevice(b->model->device));
  return launch_obs(b, (hipStream_t)stream);
}

int myo_obs_only(myo_batch* b, void* stream) {
  if (!b) return fail(MYO_E_ARG, "myo_obs_only: null");
  HIPCHK(hipSetDevice(b->model->device));
  return launch_obs(b, (hipStream_t)stream, 1);
}

int myo_batch_set_condition(myo_batch* b, int frame_skip, int epl_actuator, int eip_actuator) {
  if (!b || frame_skip <= 0) return fail(MYO_E_ARG, "myo_batch_set_condition: bad arguments");
  const int nu = b->model->dm.nu;
  if (epl_actuator >= nu || eip_actuator >= nu) return fail(MYO_E_ARG, "myo_batch_set_condition: actuator id out of range");
  b->db.fat_dt = (float)frame_skip * b->model->dm.timestep;
  b->db.reaf_epl = epl_actuator; b->db.reaf_eip = eip_actuator;
  return MYO_OK;
}

int myo_batch_set_fatigue_reset(myo_batch* b, int mode, const float* fatigue_vec) {
  if (!b || mode < 0 || mode > 2 || (mode == 2 && !fatigue_vec)) return fail(MYO_E_ARG, "myo_batch_set_fatigue_reset: mode 0 / 1 / 2 (+ vector)");
  HIPCHK(hipSetDevice(b->model->device));
  if (mode == 2) { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipMemcpy(b->d_fatvec, fatigue_vec, (size_t)b->model->dm.nu * 4, hipMemcpyHostToDevice)); }
  b->task.fatigue_mode = mode; b->task.fatigue_vec = mode == 2 ? b->d_fatvec : nullptr;
  return MYO_OK;
}

int myo_obs_reset_only(myo_batch* b, void* stream) {
  if (!b) return fail(MYO_E_ARG, "myo_obs_reset_only: null");
  HIPCHK(hipSetDevice(b->model->device));
  return launch_obs(b, (hipStream_t)stream, 1, 1);
}

int myo_status(myo_batch* b, int32_t* host_flags) {
  if (!b || !host_flags) return fail(MYO_E_ARG, "myo_status: null");
  HIPCHK(hipSetDevice(b->model->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host_flags, b->db.flags, (size_t)b->db.B * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemset(b->db.flags, 0, (size_t)b->db.B * 4));
  return MYO_OK;
}

int myo_random_action(myo_batch* b, float* action_dev, uint64_t seed, uint64_t step, int env_offset, void* stream) {
  if (!b || !action_dev) return fail(MYO_E_ARG, "myo_random_action: null");
  size_t n = (size_t)b->db.B * b->model->dm.nu;
  hipLaunchKernelGGL(random_action_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, action_dev, b->db.B,
                     b->model->dm.nu, seed, step, env_offset);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

int myo_set_balance(myo_batch* b, int on) {
  if (!b) return fail(MYO_E_ARG, "null batch");
  b->balance = on;
  return MYO_OK;
}

int myo_set_lanes(int lanes) {
  if (lanes != 16 && lanes != 32 && lanes != 64) return fail(MYO_E_ARG, "lanes per env must be 16, 32 or 64");
  g_lanes = lanes;
  return MYO_OK;
}

/* diagnostic build only (MYO_STAMPS=1): per-workgroup clock64 totals of the 10 stages of the last myo_step */
int myo_read_stamps(myo_batch* b, long long* host, int nwg) {
  if (!b || !host) return fail(MYO_E_ARG, "myo_read_stamps: null");
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host, b->d_stamps, (size_t)nwg * 12 * sizeof(long long), hipMemcpyDeviceToHost));
  return MYO_STAMPS ? MYO_OK : 1;
}

int myo_sync(void* stream) {
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return MYO_OK;
}

int myo_bench_rollout(myo_batch* b, int steps, int nsubsteps, uint64_t seed, int mode, int max_episode_steps, void* stream, float* ms_out) {
  if (!b || steps <= 0) return fail(MYO_E_ARG, "myo_bench_rollout: bad arguments");
  HIPCHK(hipSetDevice(b->model->device));
  hipStream_t s = (hipStream_t)stream;
  int rc;
  if (!(mode & MYO_BENCH_FRESH_ACTIONS)) { rc = myo_random_action(b, b->d_action, seed, b->bench_step, b->env_offset, stream); if (rc) return rc; }
  // ms_out == NULL: asynchronous -- the launches are only enqueued (a multi-GPU caller interleaves its collective on the same stream)
  // and their kernel event pairs pile up until myo_bench_last_kernel_ms collects them
  const int base = ms_out ? 0 : b->kev_pending;
  while ((int)b->kev.size() < 2 * (base + steps)) { hipEvent_t e; HIPCHK(hipEventCreate(&e)); b->kev.push_back(e); }
  if (ms_out) { b->kev_pending = 0; HIPCHK(hipEventRecord(b->ev0, s)); }
  for (int i = 0; i < steps; i++) {
    if (mode & MYO_BENCH_FRESH_ACTIONS) { rc = myo_random_action(b, b->d_action, seed, b->bench_step++, b->env_offset, stream); if (rc) return rc; }
    HIPCHK(hipEventRecord(b->kev[2 * (base + i)], s));       // brackets the dominant kernel (+ its tiny placement kernel) on its own stream
    const bool mjx_track = b->task.task == MYO_TASK_TRACK && b->track_flavour == 0;
    rc = launch_step(b, b->d_action, mjx_track ? MYO_ACTMAP_CTRLRANGE : MYO_ACTMAP_MUSCLE_SIGMOID, nsubsteps, s);
    if (rc) return rc;
    HIPCHK(hipEventRecord(b->kev[2 * (base + i) + 1], s));
    const TaskHooks* hooks = task_hooks(b->task.task);
    if (mjx_track) continue;   // observation, reward, done and the masked reset are the step kernel's own epilogue
    if ((mode & MYO_BENCH_OBS) && (mode & MYO_BENCH_AUTORESET) && max_episode_steps > 0 && hooks && hooks->post) {
      // observation + auto-reset + first observation of the new episodes in ONE launch (task_post_kernel)
      if ((rc = hooks->post(b, s, seed, max_episode_steps))) return rc;
      HIPCHK(hipGetLastError());
      continue;
    }
    if ((mode & MYO_BENCH_OBS) && b->task.task != MYO_TASK_NONE && b->task.task != MYO_TASK_WALK) { rc = launch_obs(b, s); if (rc) return rc; }   // walk: fused into the step launch
    if ((mode & MYO_BENCH_AUTORESET) && max_episode_steps > 0) {
      rc = myo_autoreset(b, max_episode_steps, seed, stream); if (rc) return rc;
      if ((mode & MYO_BENCH_OBS) && b->task.task != MYO_TASK_NONE) { rc = launch_obs(b, s, 1, 1); if (rc) return rc; }
    }
  }
  if (!ms_out) { b->kev_pending = base + steps; return MYO_OK; }
  HIPCHK(hipEventRecord(b->ev1, s));
  HIPCHK(hipEventSynchronize(b->ev1));
  HIPCHK(hipEventElapsedTime(ms_out, b->ev0, b->ev1));
  float tot = 0.f;
  for (int i = 0; i < steps; i++) { float t; HIPCHK(hipEventElapsedTime(&t, b->kev[2 * i], b->kev[2 * i + 1])); tot += t; }
  b->last_kernel_ms = tot;
  return MYO_OK;
}

/* total HIP-event milliseconds spent in the step kernel launches of the last synchronous myo_bench_rollout call, or -- after
 * asynchronous calls (ms_out == NULL) -- of all launches enqueued since the last collection (waits for them) */
const char* myo_bench_last_kernel_name(const myo_batch* b) { return b ? b->last_kernel : ""; }

/* measured VALU issue peak of the device at `waves_per_simd` resident waves per SIMD (1, 2, 4 or 8): wave64 v_fma_f32 instructions per second,
 * chip-wide.  One workgroup of 4 * waves_per_simd waves per CU (the LDS request keeps a second workgroup off the CU). */
int myo_probe_valu(int device, int waves_per_simd, int iters, double* wave_insts_per_s, int* n_cu_out) {
  if (!wave_insts_per_s || !(waves_per_simd >= 1 && waves_per_simd <= 4 || waves_per_simd == 8) || iters < 1) return fail(MYO_E_ARG, "myo_probe_valu: waves_per_simd must be 1..4 or 8");
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  const int ncu = prop.multiProcessorCount;
  const size_t lds = 60 * 1024;   // with 160 KB per CU at most two such workgroups fit: grid = ncu keeps it to one in practice, 2 * ncu gives 8 waves / SIMD
  HIPCHK(hipFuncSetAttribute((const void*)valu_probe_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
  float* out = nullptr;
  const int wg_per_cu = waves_per_simd == 8 ? 2 : 1;      // 8 waves per SIMD = two 1024-thread workgroups per CU (2 x 60 KB of LDS fit)
  const int threads = 256 * (waves_per_simd / wg_per_cu);
  HIPCHK(hipMalloc(&out, (size_t)2 * ncu * threads * 4));
  hipEvent_t e0, e1;
  HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
  hipLaunchKernelGGL(valu_probe_kernel, dim3(ncu * wg_per_cu), dim3(threads), lds, 0, out, iters / 8 + 1, 1.0f);   // warm-up (clocks, code cache)
  HIPCHK(hipEventRecord(e0, 0));
  hipLaunchKernelGGL(valu_probe_kernel, dim3(ncu * wg_per_cu), dim3(threads), lds, 0, out, iters, 1.0f);
  HIPCHK(hipEventRecord(e1, 0));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  (void)hipFree(out); (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  *wave_insts_per_s = (double)ncu * 4.0 * waves_per_simd * (double)iters * 256.0 / ((double)ms * 1e-3);
  if (n_cu_out) *n_cu_out = ncu;
  return MYO_OK;
}

int myo_bench_last_kernel_ms(myo_batch* b, float* ms_out) {
  if (!b || !ms_out) return fail(MYO_E_ARG, "null");
  if (b->kev_pending > 0) {
    HIPCHK(hipSetDevice(b->model->device));
    HIPCHK(hipEventSynchronize(b->kev[2 * b->kev_pending - 1]));
    float tot = 0.f;
    for (int i = 0; i < b->kev_pending; i++) { float t; HIPCHK(hipEventElapsedTime(&t, b->kev[2 * i], b->kev[2 * i + 1])); tot += t; }
    b->last_kernel_ms = tot;
    b->kev_pending = 0;
  }
  *ms_out = b->last_kernel_ms;
  return MYO_OK;
}

struct myo_policy {
  int device = 0;
  PolicyDev pd{};
  std::vector<void*> dev_allocs;
};

int myo_policy_load(int device, int obs_dim, int act_dim, int nlayers, const int* layer_out, const float* obs_mean, const float* obs_std,
                    const float* const* kernels, const float* const* biases, myo_policy** out) {
  if (!out || !layer_out || !obs_mean || !obs_std || !kernels || !biases || obs_dim <= 0 || act_dim <= 0 || nlayers <= 0 || nlayers > 8)
    return fail(MYO_E_ARG, "myo_policy_load: bad arguments");
  if (layer_out[nlayers - 1] != 2 * act_dim) return fail(MYO_E_ARG, "myo_policy_load: last layer must have 2*act_dim outputs (loc, scale)");
  for (int l = 0; l < nlayers; l++) if (layer_out[l] <= 0 || layer_out[l] > 512) return fail(MYO_E_UNSUPPORTED, "myo_policy_load: layer width must be in 1..512");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MYO_E_HIP, "myo_policy_load: no such HIP device");
  HIPCHK(hipSetDevice(device));
  myo_policy* p = new myo_policy();
  p->device = device;
  PolicyDev& P = p->pd;
  P.obs_dim = obs_dim; P.act_dim = act_dim; P.nlayers = nlayers;
  auto up = [&](const float* src, size_t n, const float** dst) -> int {
    void* d = nullptr;
    if (hipMalloc(&d, n * 4) != hipSuccess) return fail(MYO_E_NOMEM, "hipMalloc policy");
    p->dev_allocs.push_back(d);
    if (hipMemcpy(d, src, n * 4, hipMemcpyHostToDevice) != hipSuccess) return fail(MYO_E_HIP, "hipMemcpy policy");
    *dst = (const float*)d;
    return 0;
  };
  int rc = 0, nin = obs_dim;
  if ((rc = up(obs_mean, obs_dim, &P.mean)) || (rc = up(obs_std, obs_dim, &P.std))) { myo_policy_free(p); return rc; }
  for (int l = 0; l < nlayers; l++) {
    P.width[l] = layer_out[l];
    if ((rc = up(kernels[l], (size_t)nin * layer_out[l], &P.W[l])) || (rc = up(biases[l], layer_out[l], &P.b[l]))) { myo_policy_free(p); return rc; }
    nin = layer_out[l];
  }
  *out = p;
  return MYO_OK;
}

void myo_policy_free(myo_policy* p) {
  if (!p) return;
  for (void* d : p->dev_allocs) (void)hipFree(d);
  delete p;
}

int myo_policy_act(myo_policy* p, const float* obs_dev, int B, float* action_dev, int deterministic, uint64_t seed, uint64_t step,
                   int env_offset, void* stream) {
  if (!p || !obs_dev || !action_dev || B <= 0) return fail(MYO_E_ARG, "myo_policy_act: bad arguments");
  HIPCHK(hipSetDevice(p->device));
  int stride = p->pd.obs_dim > POL_MAXW ? p->pd.obs_dim : POL_MAXW;
  for (int l = 0; l < p->pd.nlayers; l++) if (p->pd.width[l] > stride) stride = p->pd.width[l];
  size_t lds = (size_t)2 * POL_ENVS * stride * 4;
  if (lds > 64 * 1024) return fail(MYO_E_UNSUPPORTED, "myo_policy_act: observation too wide for the LDS tile");
  hipLaunchKernelGGL(policy_kernel, dim3((B + POL_ENVS - 1) / POL_ENVS), dim3(POL_ENVS * POL_MAXW), lds, (hipStream_t)stream, p->pd, obs_dev, B,
                     action_dev, deterministic, seed, step, env_offset);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

// ---- PPO training (include/myo_hip_ppo.h; kernels in myo_kernels_ppo.h)
int myo_policy_update(myo_policy* p, const float* obs_mean, const float* obs_std, const float* const* kernels, const float* const* biases,
                      int src_is_device, void* stream) {
  if (!p) return fail(MYO_E_ARG, "myo_policy_update: null policy");
  HIPCHK(hipSetDevice(p->device));
  const PolicyDev& P = p->pd;
  const hipMemcpyKind kind = src_is_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
  auto put = [&](const float* dst, const float* src, size_t n) -> hipError_t {
    return src ? hipMemcpyAsync(const_cast<float*>(dst), src, n * 4, kind, (hipStream_t)stream) : hipSuccess;
  };
  HIPCHK(put(P.mean, obs_mean, P.obs_dim));
  HIPCHK(put(P.std, obs_std, P.obs_dim));
  int nin = P.obs_dim;
  for (int l = 0; l < P.nlayers; l++) {
    if (kernels) HIPCHK(put(P.W[l], kernels[l], (size_t)nin * P.width[l]));
    if (biases) HIPCHK(put(P.b[l], biases[l], P.width[l]));
    nin = P.width[l];
  }
  if (!src_is_device) HIPCHK(hipStreamSynchronize((hipStream_t)stream));      // the caller may free its host arrays on return
  return MYO_OK;
}

int myo_policy_sample(myo_policy* p, const float* obs_dev, int B, float* action_dev, float* raw_dev, float* logp_dev, uint64_t seed,
                      uint64_t step, int env_offset, void* stream) {
  if (!p || !obs_dev || !action_dev || !raw_dev || !logp_dev || B <= 0) return fail(MYO_E_ARG, "myo_policy_sample: bad arguments");
  HIPCHK(hipSetDevice(p->device));
  int stride = p->pd.obs_dim > POL_MAXW ? p->pd.obs_dim : POL_MAXW;
  for (int l = 0; l < p->pd.nlayers; l++) if (p->pd.width[l] > stride) stride = p->pd.width[l];
  size_t lds = (size_t)2 * POL_ENVS * stride * 4;
  if (lds > 64 * 1024) return fail(MYO_E_UNSUPPORTED, "myo_policy_sample: observation too wide for the LDS tile");
  hipLaunchKernelGGL(policy_sample_kernel, dim3((B + POL_ENVS - 1) / POL_ENVS), dim3(POL_ENVS * POL_MAXW), lds, (hipStream_t)stream, p->pd, obs_dev, B,
                     action_dev, raw_dev, logp_dev, seed, step, env_offset);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

int myo_ppo_gae(const float* rewards, const float* values, const float* bootstrap, const float* termination, const float* truncation,
                int T, int B, float discount, float lambda, float* vs_out, float* adv_out, void* stream) {
  if (!rewards || !values || !bootstrap || !termination || !truncation || !vs_out || !adv_out || T <= 0 || B <= 0)
    return fail(MYO_E_ARG, "myo_ppo_gae: bad arguments");
  hipLaunchKernelGGL(ppo_gae_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, rewards, values, bootstrap, termination, truncation,
                     T, B, discount, lambda, vs_out, adv_out);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

// ---- the learner (include/myo_hip_ppo.h; kernels in myo_kernels_learner.h)
struct LearnerNet {
  int nlayers = 0, width[8] = {};
  size_t off[8] = {};                 // of layer l's kernel in the flat parameter array; its bias follows at off + in * out
  float* Z[8] = {};                   // pre-activations [rows][width], and the loss's derivative with respect to them
  float* dZ[8] = {};
  int in(int l, int obs_dim) const { return l ? width[l - 1] : obs_dim; }
};

struct myo_ppo_learner {
  int device = 0;
  myo_ppo_config cfg{};
  LearnerNet net[2];                  // 0 policy, 1 value
  size_t total = 0;                   // floats in the flat parameter array
  float* flat = nullptr;              // [4][total]: parameters, gradients, Adam's m and v
  float* partial = nullptr;           // [LRN_MAXSPLIT or fewer][total]: the dW launches' split sums
  float *vs = nullptr, *adv = nullptr, *rowloss = nullptr, *stats = nullptr;
  long long steps = 0;
  std::vector<void*> dev_allocs;
};

static int learner_splits(int rows) { return std::min(LRN_MAXSPLIT, (rows + LRN_CHUNK - 1) / LRN_CHUNK); }

int myo_ppo_learner_create(int device, const myo_ppo_config* c, const float* const* policy_kernels, const float* const* policy_biases,
                           const float* const* value_kernels, const float* const* value_biases, myo_ppo_learner** out) {
  if (!out || !c || !policy_kernels || !policy_biases || !value_kernels || !value_biases || c->obs_dim < 1 || c->act_dim < 1 ||
      c->policy_nlayers < 1 || c->value_nlayers < 1 || c->max_unroll < 1 || c->max_minibatch < 1)
    return fail(MYO_E_ARG, "myo_ppo_learner_create: bad arguments");
  if (c->policy_nlayers > 8 || c->value_nlayers > 8) return fail(MYO_E_UNSUPPORTED, "myo_ppo_learner_create: at most 8 layers per network");
  const float* const* ks[2] = {policy_kernels, value_kernels};
  const float* const* bs[2] = {policy_biases, value_biases};
  for (int n = 0; n < 2; n++) {
    const int L = n ? c->value_nlayers : c->policy_nlayers;
    const int* w = n ? c->value_out : c->policy_out;
    for (int l = 0; l < L; l++) {
      if (w[l] < 1 || !ks[n][l] || !bs[n][l]) return fail(MYO_E_ARG, "myo_ppo_learner_create: a layer without width, kernel or bias");
      if (w[l] > 512) return fail(MYO_E_UNSUPPORTED, "myo_ppo_learner_create: layer width must be in 1..512");
    }
    if (w[L - 1] != (n ? 1 : 2 * c->act_dim)) return fail(MYO_E_ARG, "myo_ppo_learner_create: the policy head is 2 * act_dim wide, the value head 1");
  }
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MYO_E_HIP, "myo_ppo_learner_create: no such HIP device");
  HIPCHK(hipSetDevice(device));
  myo_ppo_learner* p = new myo_ppo_learner();
  p->device = device;
  p->cfg = *c;
  const size_t rows = ((size_t)c->max_unroll + 1) * c->max_minibatch;
  if (rows > (size_t)1 << 30) { delete p; return fail(MYO_E_UNSUPPORTED, "myo_ppo_learner_create: more than 2^30 rows"); }
  auto alloc = [&](size_t n, float** dst) -> int {
    void* d = nullptr;
    if (hipMalloc(&d, n * 4) != hipSuccess) return fail(MYO_E_NOMEM, "hipMalloc learner");
    p->dev_allocs.push_back(d);
    if (hipMemset(d, 0, n * 4) != hipSuccess) return fail(MYO_E_HIP, "hipMemset learner");
    *dst = (float*)d;
    return 0;
  };
  int rc = 0;
  for (int n = 0; n < 2 && !rc; n++) {
    LearnerNet& N = p->net[n];
    N.nlayers = n ? c->value_nlayers : c->policy_nlayers;
    for (int l = 0; l < N.nlayers && !rc; l++) {
      N.width[l] = (n ? c->value_out : c->policy_out)[l];
      N.off[l] = p->total;
      p->total += ((size_t)N.in(l, c->obs_dim) + 1) * N.width[l];
      if ((rc = alloc(rows * N.width[l], &N.Z[l]))) break;
      rc = alloc(rows * N.width[l], &N.dZ[l]);
    }
  }
  if (!rc) rc = alloc(4 * p->total, &p->flat);
  if (!rc) rc = alloc((size_t)learner_splits((int)rows) * p->total, &p->partial);
  if (!rc) rc = alloc(rows, &p->vs);
  if (!rc) rc = alloc(rows, &p->adv);
  if (!rc) rc = alloc(3 * rows, &p->rowloss);
  if (!rc) rc = alloc(2, &p->stats);
  for (int n = 0; n < 2 && !rc; n++)
    for (int l = 0; l < p->net[n].nlayers && !rc; l++) {
      const LearnerNet& N = p->net[n];
      const size_t nk = (size_t)N.in(l, c->obs_dim) * N.width[l];
      if (hipMemcpy(p->flat + N.off[l], ks[n][l], nk * 4, hipMemcpyHostToDevice) != hipSuccess ||
          hipMemcpy(p->flat + N.off[l] + nk, bs[n][l], (size_t)N.width[l] * 4, hipMemcpyHostToDevice) != hipSuccess)
        rc = fail(MYO_E_HIP, "hipMemcpy learner");
    }
  if (rc) { myo_ppo_learner_free(p); return rc; }
  *out = p;
  return MYO_OK;
}

void myo_ppo_learner_free(myo_ppo_learner* p) {
  if (!p) return;
  for (void* d : p->dev_allocs) (void)hipFree(d);
  delete p;
}

int myo_ppo_learner_tensor(myo_ppo_learner* p, int net, int layer, int what, int which, float** dev_ptr, size_t* count) {
  if (!p || !dev_ptr || !count || net < 0 || net > 1 || what < 0 || what > 1 || which < 0 || which > 3 || layer < 0 || layer >= p->net[net].nlayers)
    return fail(MYO_E_ARG, "myo_ppo_learner_tensor: bad arguments");
  const LearnerNet& N = p->net[net];
  const size_t nk = (size_t)N.in(layer, p->cfg.obs_dim) * N.width[layer];
  *dev_ptr = p->flat + (size_t)which * p->total + N.off[layer] + (what ? nk : 0);
  *count = what ? (size_t)N.width[layer] : nk;
  return MYO_OK;
}

int myo_ppo_learner_step(myo_ppo_learner* p, const float* obs, const float* u, const float* logp, const float* rewards, const float* termination,
                         const float* truncation, int T, int B, const int64_t* idx, int mb, const float* obs_mean, const float* obs_std,
                         const float* entropy_noise, float* loss_sums, void* stream) {
  if (!p || !obs || !u || !logp || !rewards || !termination || !truncation || !idx || !obs_mean || !obs_std || !entropy_noise)
    return fail(MYO_E_ARG, "myo_ppo_learner_step: null pointer");
  if (T < 1 || mb < 1 || T > p->cfg.max_unroll || mb > p->cfg.max_minibatch || mb > B)
    return fail(MYO_E_ARG, "myo_ppo_learner_step: T in 1..max_unroll and mb in 1..min(max_minibatch, B)");
  HIPCHK(hipSetDevice(p->device));
  const myo_ppo_config& c = p->cfg;
  hipStream_t st = (hipStream_t)stream;
  const int rows_of[2] = {T * mb, (T + 1) * mb};
  const int S = learner_splits(rows_of[1]);
  const dim3 blk(256);
  auto tiles = [](int n) { return (unsigned)((n + LRN_TILE - 1) / LRN_TILE); };
  auto gemm = [&](int n, int l) {
    const LearnerNet& N = p->net[n];
    LearnerGemm g{};
    g.X = l ? N.Z[l - 1] : nullptr;
    g.W = p->flat + N.off[l];
    g.dZ = N.dZ[l];
    g.Zprev = g.X;
    g.obs = obs; g.idx = idx; g.mean = obs_mean; g.std = obs_std;
    g.rows = rows_of[n]; g.kdim = N.in(l, c.obs_dim); g.n = N.width[l]; g.mb = mb; g.B = B;
    g.chunk = ((rows_of[n] + S - 1) / S + LRN_TK - 1) / LRN_TK * LRN_TK;
    g.split_stride = p->total;
    return g;
  };
  // forward: Z_l = in_l W_l + b_l
  for (int n = 0; n < 2; n++)
    for (int l = 0; l < p->net[n].nlayers; l++) {
      LearnerGemm g = gemm(n, l);
      g.out = p->net[n].Z[l];
      const dim3 grid(tiles(g.rows), tiles(g.n));
      if (l) hipLaunchKernelGGL((learner_gemm_kernel<LRN_FWD, LRN_SRC_SWISH>), grid, blk, 0, st, g);
      else hipLaunchKernelGGL((learner_gemm_kernel<LRN_FWD, LRN_SRC_OBS>), grid, blk, 0, st, g);
    }
  // the loss and its derivative at the two heads
  const LearnerNet &P = p->net[0], &V = p->net[1];
  hipLaunchKernelGGL(learner_gae_kernel, dim3(1), blk, 0, st, V.Z[V.nlayers - 1], rewards, termination, truncation, idx, T, mb, B, c.discounting,
                     c.gae_lambda, c.reward_scaling, c.normalize_advantage, p->vs, p->adv, p->stats);
  hipLaunchKernelGGL(learner_loss_kernel, dim3((unsigned)((rows_of[1] + 3) / 4)), blk, 0, st, P.Z[P.nlayers - 1], V.Z[V.nlayers - 1], u, logp, entropy_noise,
                     idx, p->vs, p->adv, p->stats, T, mb, B, c.act_dim, c.clipping_epsilon, c.entropy_cost, P.dZ[P.nlayers - 1], V.dZ[V.nlayers - 1],
                     p->rowloss);
  hipLaunchKernelGGL(learner_loss_sum_kernel, dim3(1), blk, 0, st, p->rowloss, rows_of[0], c.entropy_cost, loss_sums);
  // backward: [dW_l; db_l] = [in_l 1]^T dZ_l in S splits, dZ_{l-1} = (dZ_l W_l^T) swish'(Z_{l-1})
  for (int n = 0; n < 2; n++)
    for (int l = p->net[n].nlayers - 1; l >= 0; l--) {
      LearnerGemm g = gemm(n, l);
      g.out = p->partial + p->net[n].off[l];
      const dim3 grid(tiles(g.kdim + 1), tiles(g.n), (unsigned)S);
      if (l) hipLaunchKernelGGL((learner_gemm_kernel<LRN_DW, LRN_SRC_SWISH>), grid, blk, 0, st, g);
      else hipLaunchKernelGGL((learner_gemm_kernel<LRN_DW, LRN_SRC_OBS>), grid, blk, 0, st, g);
      if (l) {
        g.out = p->net[n].dZ[l - 1];
        hipLaunchKernelGGL((learner_gemm_kernel<LRN_DX, LRN_SRC_SWISH>), dim3(tiles(g.rows), tiles(g.kdim)), blk, 0, st, g);
      }
    }
  p->steps++;
  const double bc1 = 1.0 - std::pow(c.beta1, (double)p->steps), bc2 = 1.0 - std::pow(c.beta2, (double)p->steps);
  hipLaunchKernelGGL(learner_adam_kernel, dim3((unsigned)((p->total + 255) / 256)), blk, 0, st, p->total, S, p->partial, p->flat, p->flat + p->total,
                     p->flat + 2 * p->total, p->flat + 3 * p->total, (float)c.beta1, (float)(1.0 - c.beta1), (float)c.beta2, (float)(1.0 - c.beta2),
                     (float)(c.learning_rate / bc1), (float)std::sqrt(bc2), (float)c.adam_eps);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

}  // extern "C"
