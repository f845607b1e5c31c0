// myo_hip.hip -- MI355X (gfx950) batched musculoskeletal stepper: kernels + C ABI (include/myo_hip.h).
//
// One translation unit, split over csrc/ for readability:
//   myo_common.h        limits, device-side structs (model tables, per-env batch arrays, task records), vector math
//   myo_physics.h       tendon wrapping, muscle model, action map (+ muscle conditions), impedance, contact frames, MPR
//   myo_task_track.h    MyoDM TrackEnv as a fused task of the TRK step kernel: reference lookup, reward / done, masked reset
//   myo_kernel_lanes.h  step_kernel<G>: the first kernel, G = 16 / 32 / 64 lanes per env, all state in LDS (cross-check / fallback)
//   myo_kernel_wave.h   step_kernel_w: one env per 64-lane wavefront (default), substep scheduler, size-specialised instantiations
//   myo_ldl_mfma.h      dense LDL^T of the Newton Hessian on the FP32 matrix cores (included by myo_kernel_wave.h)
//   myo_kernels_aux.h   RNG, placement hint, random actions, policy inference, reset, state-only observations, task_obs_kernel / task_post_kernel
//   myo_host.h          host records: myo_model, myo_batch, the per-task hook record (TaskHooks) and its generic launchers
//   myo_task_*.h        key-turn, pen, baoding, die, classic MyoDM: a task's observation body, its configure checks and its hook record
//   myo_host_model.h    myo_model_load in pieces: blob view, table upload, packing of the per-lane records, kernel class
//   myo_hip.hip         host side: batches, the table of step-kernel instantiations, launches, the task table, the extern "C" entry points
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
#include "myo_host.h"
#include "myo_task_keyturn.h"
#include "myo_task_pen.h"
#include "myo_task_baoding.h"
#include "myo_task_die.h"
#include "myo_task_myodm.h"
#include "myo_host_model.h"

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
  const int rc = load_model(m.get(), B);
  if (rc) return rc;
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

static int balloc(myo_batch* b, void** p, size_t nbytes) {
  HIPCHK(hipMalloc(p, nbytes));
  HIPCHK(hipMemset(*p, 0, nbytes));
  b->dev_allocs.push_back(*p);
  return 0;
}

int myo_batch_create(const myo_model* m, int B, myo_batch** out) {
  if (!m || !out || B <= 0) return fail(MYO_E_ARG, "myo_batch_create: bad arguments");
  HIPCHK(hipSetDevice(m->device));
  myo_batch* b = new myo_batch();
  b->model = m;
  DevBatch& d = b->db;
  d.B = B;
  int nv = m->dm.nv, nu = m->dm.nu, nq = m->nq, rc;
  b->ntarget_alloc = nv > 24 ? nv : 24;
  b->obs_alloc = 3 * nv + 4 * nu + 64;
#define BA(ptr, n) if ((rc = balloc(b, (void**)&ptr, (size_t)(n) * 4))) { myo_batch_free(b); return rc; }
  BA(d.qpos, (size_t)B * nq) BA(d.qvel, (size_t)B * nv) BA(d.act, (size_t)B * nu) BA(d.ctrl, (size_t)B * nu) BA(d.warm, (size_t)B * nv)
  BA(d.time, B) BA(d.target, (size_t)B * b->ntarget_alloc) BA(d.obs, (size_t)B * b->obs_alloc) BA(d.reward, B) BA(d.done, B)
  BA(d.solved, B) BA(d.qacc, (size_t)B * nv) BA(d.tenlen, (size_t)B * nu) BA(d.actforce, (size_t)B * nu) BA(d.sitexpos, (size_t)B * 24)
  BA(d.flags, B) BA(d.diag, (size_t)B * 8) BA(d.elapsed, B) BA(d.episode, B) BA(d.mprw, (size_t)B * 64)
  BA(b->d_tlo, b->ntarget_alloc) BA(b->d_thi, b->ntarget_alloc) BA(b->d_init, nq) BA(b->d_jlo, nv) BA(b->d_jhi, nv) BA(b->d_rnd, 4 * (size_t)nq)
  BA(b->d_action, (size_t)B * nu)
  BA(d.fatigue, (size_t)B * 3 * nu)
  d.hfield = nullptr; d.gsize = nullptr; d.gsize_cg = -1;
  d.sens = nullptr; d.cfrc = nullptr; d.ntouch = 0;
  d.ovf = nullptr; d.ovf_cand = nullptr; d.ovf_row = 0; d.ovf_rows = 0; d.linkx = nullptr; d.track = nullptr; d.env_offset = 0;
  if (m->trk) { BA(d.linkx, (size_t)B * 12 * m->dm.nl) }
  if (m->wave_ok) {   // contact-table overflow rows of the wave kernel (instantiations <24,8,...> and <36,20,...>)
    const int kc = m->wave_cfg == 0 ? 8 : 20, nj = m->trk ? 4 : 3;
    d.ovf_row = 8 + nj * kc + (kc + 3) / 4 + (m->trk ? TRK_STATE : 0);
    d.ovf_rows = m->trk ? NCX2 : NCX;
    BA(d.ovf, (size_t)B * d.ovf_rows * d.ovf_row) BA(d.ovf_cand, (size_t)B * NCANDX)
  }
  if (m->dw.hf.on) { BA(d.hfield, (size_t)B * m->dw.hf.nrow * m->dw.hf.ncol) }   // zero-filled: flat terrain at the geom's height
  BA(b->d_initv, nv) BA(b->d_init2, nq) BA(b->d_initv2, nv) BA(b->d_fatvec, nu)
  { void* pw = nullptr; if ((rc = balloc(b, &pw, sizeof(DevWalk)))) { myo_batch_free(b); return rc; } b->d_walk = (DevWalk*)pw; }
  BA(b->d_stamps, (size_t)B * 12 * 3 * 2)      // 3 x 12 long long per workgroup (diagnostic build)
  BA(b->d_order, B)
  b->sched_stride = (B + 7) / 8 + 1;                 // per queue with 8 queues; launch_step widens it when the device shows fewer XCDs
  BA(b->d_sched, 32 + B + 64)
#undef BA
  if (const char* e = getenv("MYO_LANES")) { int g = atoi(e); if (g == 16 || g == 32 || g == 64) g_lanes = g; }
  HIPCHK(hipMemcpy(b->d_jlo, m->jnt_lo.data(), nv * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_jhi, m->jnt_hi.data(), nv * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(b->d_init, m->qpos0.data(), nq * 4, hipMemcpyHostToDevice));
  // default: every env at qpos0
  std::vector<float> q((size_t)B * nq);
  for (int e = 0; e < B; e++) memcpy(&q[(size_t)e * nq], m->qpos0.data(), nq * 4);
  HIPCHK(hipMemcpy(d.qpos, q.data(), q.size() * 4, hipMemcpyHostToDevice));
  {
    std::vector<float> f((size_t)B * 3 * nu, 0.f);
    for (int e = 0; e < B; e++) for (int i = 0; i < nu; i++) f[(size_t)e * 3 * nu + nu + i] = 1.f;      // MR = 1
    HIPCHK(hipMemcpy(d.fatigue, f.data(), f.size() * 4, hipMemcpyHostToDevice));
    d.fat_dt = m->dm.timestep; d.reaf_epl = d.reaf_eip = -1;
  }
  b->task.task = MYO_TASK_NONE; b->task.frame_skip = 1; b->task.obs_dim = 0; b->task.ntarget = 0;
  b->task.jnt_lo = b->d_jlo; b->task.jnt_hi = b->d_jhi; b->task.init_qpos = b->d_init; b->task.target_lo = b->d_tlo; b->task.target_hi = b->d_thi;
  b->task.init_qvel = nullptr;
  b->task.init_qpos_alt = nullptr; b->task.init_qvel_alt = nullptr; b->task.reset_noise_std = 0.f; b->task.fatigue_mode = 0; b->task.fatigue_vec = nullptr;
  HIPCHK(hipEventCreate(&b->ev0));
  HIPCHK(hipEventCreate(&b->ev1));
  *out = b;
  return MYO_OK;
}

void myo_batch_free(myo_batch* b) {
  if (!b) return;
  for (hipEvent_t e : b->kev) (void)hipEventDestroy(e);
  for (void* p : b->dev_allocs) (void)hipFree(p);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  delete b;
}

int myo_batch_size(const myo_batch* b) { return b ? b->db.B : 0; }

static int set_quat_body(myo_batch* b, int body);   // (below, with the rest of MYO_F_BODYQUAT)
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

// per-env body-mass override (MYO_F_BODYMASS / MYO_F_BODYMASS_RANGE): the refusals, shared by its start and the launches after it
static int bm_check(const myo_batch* b) {
  const myo_model* m = b->model;
  if (m->rk4) return fail(MYO_E_UNSUPPORTED, "per-env body masses: RK4 models are not supported");
  if (m->trk) return fail(MYO_E_UNSUPPORTED, "per-env body masses: models of the TrackEnv class are not supported");
  if (m->dw.hf.on) return fail(MYO_E_UNSUPPORTED, "per-env body masses: height-field models are not supported");
  if (!m->wave_ok || g_lanes != 64) return fail(MYO_E_UNSUPPORTED, "per-env body masses: wave-per-env kernel only (lanes = 64)");
  const int t = b->task.task;
  if (t == MYO_TASK_WALK || t == MYO_TASK_STAND || t == MYO_TASK_TRACK)
    return fail(MYO_E_UNSUPPORTED, "per-env body masses: the walk / stand / track tasks use model-wide mass totals");
  if (m->body_mass0.empty() || !m->d_lm_adr) return fail(MYO_E_UNSUPPORTED, "per-env body masses: the model blob lacks the body tables");
  return MYO_OK;
}

static int bm_start(myo_batch* b) {
  if (b->bm_on) return MYO_OK;
  int rc = bm_check(b);
  if (rc) return rc;
  const myo_model* m = b->model;
  DevBatch& d = b->db;
  const int nb = (int)m->body_mass0.size();
  float *bm = nullptr, *br = nullptr, *lc = nullptr;
  if ((rc = balloc(b, (void**)&bm, (size_t)d.B * nb * 4)) || (rc = balloc(b, (void**)&br, (size_t)d.B * 2 * nb * 4)) ||
      (rc = balloc(b, (void**)&lc, (size_t)d.B * m->dm.nl * 10 * 4))) return rc;
  std::vector<float> v((size_t)d.B * nb);
  for (int e = 0; e < d.B; e++) memcpy(&v[(size_t)e * nb], m->body_mass0.data(), nb * 4);
  HIPCHK(hipSetDevice(m->device));
  HIPCHK(hipMemcpy(bm, v.data(), v.size() * 4, hipMemcpyHostToDevice));
  d.bmass = bm; d.bmass_range = br; d.linkc = lc; d.nbody = nb;
  b->bm_on = true;
  return MYO_OK;
}

// per-env root-body offset (MYO_F_BODYPOS / MYO_F_BODYPOS_RANGE): TrackEnv-class models whose last joint sits on a root body only
static int bp_check(const myo_batch* b) {
  const myo_model* m = b->model;
  if (!(m->wave_ok && m->trk)) return fail(MYO_E_UNSUPPORTED, "per-env body position: models of the TrackEnv class only");
  if (m->bp_link < 0) return fail(MYO_E_UNSUPPORTED, "per-env body position: the body of the model's last joint is not a root body (a child of the world heading its link)");
  return MYO_OK;
}

static int bp_start(myo_batch* b) {
  if (b->bp_on) return MYO_OK;
  int rc = bp_check(b);
  if (rc) return rc;
  DevBatch& d = b->db;
  float *bp = nullptr, *br = nullptr;
  HIPCHK(hipSetDevice(b->model->device));
  if ((rc = balloc(b, (void**)&bp, (size_t)d.B * 3 * 4)) || (rc = balloc(b, (void**)&br, (size_t)d.B * 6 * 4))) return rc;   // zero: no offset
  d.bpos = bp; d.bpos_range = br; d.bpos_link = b->model->bp_link;
  b->bp_on = true;
  return MYO_OK;
}

// per-env orientation of one world-welded body (MYO_F_BODYQUAT / MYO_F_BODYQUAT_RANGE): TrackEnv-class models, the body selected first
// (myo_task_config.quat_body)
static int set_quat_body(myo_batch* b, int body) {
  const myo_model* m = b->model;
  if (!(m->wave_ok && m->trk)) return fail(MYO_E_UNSUPPORTED, "per-env body orientation: models of the TrackEnv class only");
  if (body <= 0 || body >= (int)m->body_parent.size()) return fail(MYO_E_ARG, "quat_body: body id out of range");
  if (m->body_parent[body] != 0 || m->body_jntnum[body] != 0) return fail(MYO_E_UNSUPPORTED, "per-env body orientation: a jointless child of the world only");
  if (b->bq_on && body != b->bq_body) return fail(MYO_E_ARG, "quat_body: the orientation of another body has started");
  b->bq_body = body;
  return MYO_OK;
}

static int bq_check(const myo_batch* b) {
  const myo_model* m = b->model;
  if (!(m->wave_ok && m->trk)) return fail(MYO_E_UNSUPPORTED, "per-env body orientation: models of the TrackEnv class only");
  if (b->bq_body < 0) return fail(MYO_E_ARG, "per-env body orientation: no body selected (myo_task_config.quat_body)");
  return MYO_OK;
}

static int bq_start(myo_batch* b) {
  if (b->bq_on) return MYO_OK;
  int rc = bq_check(b);
  if (rc) return rc;
  const myo_model* m = b->model;
  DevBatch& d = b->db;
  const int bd = b->bq_body, ncg = m->dm.ncg, ns = m->dims.nsite;
  std::vector<float> q((size_t)d.B * 4), c(12);
  double R0[9];
  quat2mat_d(R0, &m->body_quat0[4 * (size_t)bd]);
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) c[3 * i + j] = (float)R0[3 * j + i];   // R(q0)^T
  for (int k = 0; k < 3; k++) c[9 + k] = (float)(m->body_pos0[3 * (size_t)bd + k] - m->dm.origin[k]);   // (lowered coordinates)
  for (int e = 0; e < d.B; e++) for (int k = 0; k < 4; k++) q[4 * (size_t)e + k] = (float)m->body_quat0[4 * (size_t)bd + k];
  std::vector<int> fl((size_t)ncg + ns, 0);
  for (int g = 0; g < ncg; g++) fl[g] = m->cg_body[g] == bd;
  for (int s2 = 0; s2 < ns; s2++) fl[ncg + s2] = m->site_body[s2] == bd;
  float *bq = nullptr, *br = nullptr, *bc = nullptr;
  int* bf = nullptr;
  HIPCHK(hipSetDevice(m->device));
  if ((rc = balloc(b, (void**)&bq, (size_t)d.B * 4 * 4)) || (rc = balloc(b, (void**)&br, (size_t)d.B * 6 * 4)) ||
      (rc = balloc(b, (void**)&bc, 12 * 4)) || (rc = balloc(b, (void**)&bf, fl.size() * 4))) return rc;
  HIPCHK(hipMemcpy(bq, q.data(), q.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(bc, c.data(), c.size() * 4, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(bf, fl.data(), fl.size() * 4, hipMemcpyHostToDevice));
  d.bquat = bq; d.bquat_range = br; d.bq_c = bc; d.bq_flag = bf;
  b->bq_on = true;
  return MYO_OK;
}

// touch sensors and contact forces (MYO_F_SENSORDATA / MYO_F_CFRC): the refusals, shared by the start and the launches after it.  Host
// side only: a refused model never reaches the GPU
static int sens_check(const myo_batch* b) {
  const myo_model* m = b->model;
  if (m->dw.ntouch <= 0) return fail(MYO_E_UNSUPPORTED, "sensors: the model blob has no touch sensors (no hip_touch table)");
  if (m->rk4) return fail(MYO_E_UNSUPPORTED, "sensors: RK4 models are not supported");
  if (m->trk) return fail(MYO_E_UNSUPPORTED, "sensors: models of the TrackEnv class are not supported");
  if (!m->wave_ok || m->wave_cfg != 1) return fail(MYO_E_UNSUPPORTED, "sensors: models of the hand class (24-dof step kernels) are not supported");
  if (g_lanes != 64) return fail(MYO_E_UNSUPPORTED, "sensors: wave-per-env kernel only (lanes = 64)");
  return MYO_OK;
}

int myo_batch_enable_sensors(myo_batch* b) {
  if (!b) return fail(MYO_E_ARG, "myo_batch_enable_sensors: null");
  int rc = sens_check(b);
  if (rc) return rc;
  if (b->sens_on) return MYO_OK;
  DevBatch& d = b->db;
  const int n = b->model->dw.ntouch;
  float *sd = nullptr, *cf = nullptr;
  HIPCHK(hipSetDevice(b->model->device));
  if ((rc = balloc(b, (void**)&sd, (size_t)d.B * n * 4)) || (rc = balloc(b, (void**)&cf, (size_t)d.B * 3 * (n + 1) * 4))) return rc;
  d.sens = sd; d.cfrc = cf; d.ntouch = n;
  b->sens_on = true;
  return MYO_OK;
}

static int field_info(myo_batch* b, int f, void** p, size_t* pitch, size_t* width) {
  const DevModel& dm = b->model->dm;
  DevBatch& d = b->db;
  size_t nv = dm.nv, nu = dm.nu;
  switch (f) {
    case MYO_F_QPOS: *p = d.qpos; *pitch = *width = (size_t)b->model->nq; break;
    case MYO_F_QVEL: *p = d.qvel; *pitch = *width = nv; break;
    case MYO_F_ACT: *p = d.act; *pitch = *width = nu; break;
    case MYO_F_CTRL: *p = d.ctrl; *pitch = *width = nu; break;
    case MYO_F_WARMSTART: *p = d.warm; *pitch = *width = nv; break;
    case MYO_F_TIME: *p = d.time; *pitch = *width = 1; break;
    case MYO_F_TARGET: *p = d.target; *pitch = *width = b->task.ntarget > 0 ? b->task.ntarget : 1; break;
    case MYO_F_OBS: *p = d.obs; *pitch = *width = b->task.obs_dim > 0 ? b->task.obs_dim : 1; break;
    case MYO_F_REWARD: *p = d.reward; *pitch = *width = 1; break;
    case MYO_F_DONE: *p = d.done; *pitch = *width = 1; break;
    case MYO_F_SOLVED: *p = d.solved; *pitch = *width = 1; break;
    case MYO_F_FLAGS: *p = d.flags; *pitch = *width = 1; break;
    case MYO_F_DIAG: *p = d.diag; *pitch = *width = 8; break;
    case MYO_F_QACC: *p = d.qacc; *pitch = *width = nv; break;
    case MYO_F_TENLEN: *p = d.tenlen; *pitch = *width = nu; break;
    case MYO_F_ACTFORCE: *p = d.actforce; *pitch = *width = nu; break;
    case MYO_F_ELAPSED: *p = d.elapsed; *pitch = *width = 1; break;
    case MYO_F_LINKX:
      if (!d.linkx) return fail(MYO_E_ARG, "MYO_F_LINKX: this model's kernel does not export link frames");
      *p = d.linkx; *pitch = *width = (size_t)12 * b->model->dm.nl; break;
    case MYO_F_ACTION: *p = b->d_action; *pitch = *width = nu; break;
    case MYO_F_FATIGUE: *p = d.fatigue; *pitch = *width = 3 * nu; break;
    case MYO_F_GEOMSIZE:
      if (!d.gsize) return fail(MYO_E_ARG, "MYO_F_GEOMSIZE: no geom override set (myo_batch_set_geom_override)");
      *p = d.gsize; *pitch = *width = 4; break;
    case MYO_F_HFIELD:
      if (!d.hfield) return fail(MYO_E_ARG, "MYO_F_HFIELD: the model has no colliding height field");
      *p = d.hfield; *pitch = *width = b->model->dw.hf.nrow * b->model->dw.hf.ncol; break;
    case MYO_F_METRICS:
      if (!b->d_metrics) return fail(MYO_E_ARG, "MYO_F_METRICS: the track task is not configured (myo_batch_configure_track)");
      *p = b->d_metrics; *pitch = *width = 4; break;
    case MYO_F_SITEXPOS: *p = d.sitexpos; *pitch = *width = b->task.ntip > 0 ? 3 * b->task.ntip : 1; break;
    case MYO_F_BODYMASS:
    case MYO_F_BODYMASS_RANGE: {   // (callers start the override first; before that the pointer is NULL)
      const size_t nb = b->model->body_mass0.size();
      *p = f == MYO_F_BODYMASS ? (void*)d.bmass : (void*)d.bmass_range;
      *pitch = *width = f == MYO_F_BODYMASS ? nb : 2 * nb;
      break;
    }
    case MYO_F_BODYPOS: *p = d.bpos; *pitch = *width = 3; break;          // (NULL until the offset is started)
    case MYO_F_BODYPOS_RANGE: *p = d.bpos_range; *pitch = *width = 6; break;
    case MYO_F_BODYQUAT: *p = d.bquat; *pitch = *width = 4; break;         // (NULL until the orientation is started)
    case MYO_F_BODYQUAT_RANGE: *p = d.bquat_range; *pitch = *width = 6; break;
    case MYO_F_SENSORDATA:
    case MYO_F_CFRC:
      if (!b->sens_on) return fail(MYO_E_ARG, "MYO_F_SENSORDATA / MYO_F_CFRC: sensors are not enabled (myo_batch_enable_sensors)");
      *p = f == MYO_F_SENSORDATA ? d.sens : d.cfrc;
      *pitch = *width = f == MYO_F_SENSORDATA ? (size_t)d.ntouch : (size_t)3 * (d.ntouch + 1);
      break;
    default: return fail(MYO_E_ARG, "unknown field");
  }
  return MYO_OK;
}

int myo_batch_field(myo_batch* b, int field, void** dev_ptr, size_t* pitch, size_t* width) {
  if (!b || !dev_ptr || !pitch || !width) return fail(MYO_E_ARG, "myo_batch_field: null");
  if (field == MYO_F_BODYMASS || field == MYO_F_BODYMASS_RANGE) { int rc = bm_start(b); if (rc) return rc; }
  if (field == MYO_F_BODYPOS || field == MYO_F_BODYPOS_RANGE) { int rc = bp_start(b); if (rc) return rc; }
  if (field == MYO_F_BODYQUAT || field == MYO_F_BODYQUAT_RANGE) { int rc = bq_start(b); if (rc) return rc; }
  return field_info(b, field, dev_ptr, pitch, width);
}

int myo_batch_read(myo_batch* b, int field, void* host, size_t nbytes) {
  void* p; size_t pitch, width;
  if (!b || !host) return fail(MYO_E_ARG, "myo_batch_read: null");
  int rc = field_info(b, field, &p, &pitch, &width);
  if (rc) return rc;
  if (nbytes != (size_t)b->db.B * width * 4) return fail(MYO_E_ARG, "myo_batch_read: size mismatch");
  if ((field == MYO_F_BODYMASS || field == MYO_F_BODYMASS_RANGE) && !b->bm_on) {   // not started: the model's masses, empty ranges
    const std::vector<float>& m0 = b->model->body_mass0;
    if (m0.empty()) return fail(MYO_E_UNSUPPORTED, "per-env body masses: the model blob lacks the body tables");
    float* h = (float*)host;
    for (int e = 0; e < b->db.B; e++) {
      if (field == MYO_F_BODYMASS) memcpy(h + (size_t)e * width, m0.data(), width * 4);
      else memset(h + (size_t)e * width, 0, width * 4);
    }
    return MYO_OK;
  }
  if ((field == MYO_F_BODYPOS || field == MYO_F_BODYPOS_RANGE) && !b->bp_on) {   // not started: no offsets, empty ranges
    if ((rc = bp_check(b))) return rc;
    memset(host, 0, nbytes);
    return MYO_OK;
  }
  if ((field == MYO_F_BODYQUAT || field == MYO_F_BODYQUAT_RANGE) && !b->bq_on) {   // not started: the compiled quaternion, empty ranges
    if ((rc = bq_check(b))) return rc;
    float* h = (float*)host;
    for (int e = 0; e < b->db.B; e++)
      for (size_t k = 0; k < width; k++) h[(size_t)e * width + k] = field == MYO_F_BODYQUAT ? (float)b->model->body_quat0[4 * (size_t)b->bq_body + k] : 0.f;
    return MYO_OK;
  }
  HIPCHK(hipSetDevice(b->model->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(host, p, nbytes, hipMemcpyDeviceToHost));
  return MYO_OK;
}

int myo_batch_write(myo_batch* b, int field, const void* host, size_t nbytes) {
  void* p; size_t pitch, width;
  if (!b || !host) return fail(MYO_E_ARG, "myo_batch_write: null");
  if (field == MYO_F_SENSORDATA || field == MYO_F_CFRC) return fail(MYO_E_ARG, "MYO_F_SENSORDATA / MYO_F_CFRC are read-only");
  int rc = field_info(b, field, &p, &pitch, &width);
  if (rc) return rc;
  if (nbytes != (size_t)b->db.B * width * 4) return fail(MYO_E_ARG, "myo_batch_write: size mismatch");
  if (field == MYO_F_BODYMASS || field == MYO_F_BODYMASS_RANGE) {
    if (b->model->body_mass0.empty()) return fail(MYO_E_UNSUPPORTED, "per-env body masses: the model blob lacks the body tables");
    const float* h = (const float*)host;
    const size_t nb = b->model->body_mass0.size();
    for (int e = 0; e < b->db.B; e++)
      for (size_t i = 0; i < nb; i++) {
        if (field == MYO_F_BODYMASS) { if (!(h[e * nb + i] >= 0.f)) return fail(MYO_E_ARG, "MYO_F_BODYMASS: masses must be >= 0"); }
        else {
          const float lo = h[2 * e * nb + i], hi = h[2 * e * nb + nb + i];
          if (!(lo >= 0.f) || !(hi >= lo)) return fail(MYO_E_ARG, "MYO_F_BODYMASS_RANGE: need 0 <= lo <= hi");
        }
      }
    if ((rc = bm_start(b))) return rc;
    if ((rc = field_info(b, field, &p, &pitch, &width))) return rc;
  }
  if (field == MYO_F_BODYPOS || field == MYO_F_BODYPOS_RANGE) {
    if ((rc = bp_check(b))) return rc;
    const float* h = (const float*)host;
    for (size_t i = 0; i < (size_t)b->db.B * width; i++) if (!std::isfinite(h[i])) return fail(MYO_E_ARG, "MYO_F_BODYPOS / MYO_F_BODYPOS_RANGE: values must be finite");
    if (field == MYO_F_BODYPOS_RANGE)
      for (int e = 0; e < b->db.B; e++)
        for (int k = 0; k < 3; k++) if (!(h[6 * e + 3 + k] >= h[6 * e + k])) return fail(MYO_E_ARG, "MYO_F_BODYPOS_RANGE: need lo <= hi");
    if ((rc = bp_start(b))) return rc;
    if ((rc = field_info(b, field, &p, &pitch, &width))) return rc;
  }
  if (field == MYO_F_BODYQUAT || field == MYO_F_BODYQUAT_RANGE) {
    if ((rc = bq_check(b))) return rc;
    const float* h = (const float*)host;
    for (size_t i = 0; i < (size_t)b->db.B * width; i++) if (!std::isfinite(h[i])) return fail(MYO_E_ARG, "MYO_F_BODYQUAT / MYO_F_BODYQUAT_RANGE: values must be finite");
    for (int e = 0; e < b->db.B; e++) {
      const float* r = h + (size_t)e * width;
      if (field == MYO_F_BODYQUAT) {
        const double n = std::sqrt((double)r[0] * r[0] + (double)r[1] * r[1] + (double)r[2] * r[2] + (double)r[3] * r[3]);
        if (!(std::fabs(n - 1.0) <= 1e-4)) return fail(MYO_E_ARG, "MYO_F_BODYQUAT: quaternions must have norm 1");
      } else {
        for (int k = 0; k < 3; k++) if (!(r[3 + k] >= r[k])) return fail(MYO_E_ARG, "MYO_F_BODYQUAT_RANGE: need lo <= hi");
      }
    }
    if ((rc = bq_start(b))) return rc;
    if ((rc = field_info(b, field, &p, &pitch, &width))) return rc;
  }
  HIPCHK(hipSetDevice(b->model->device));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(p, host, nbytes, hipMemcpyHostToDevice));
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

// the hooks of the tasks that live in myo_kernels_aux.h / this file, and the table of all tasks
static int state_configure(myo_batch* b, const myo_task_config* c) {   // pose / stand / hold
  const myo_model* m = b->model;
  const int nv = m->dm.nv, nq = m->nq, na = m->dm.na_obs;
  if (c->task == MYO_TASK_POSE) {
    if (c->ntarget != nv) return fail(MYO_E_ARG, "pose task: ntarget must equal nq");
    b->task.obs_dim = 3 * nv + na;
  } else if (c->task == MYO_TASK_STAND) {
    if (c->ntarget != 3) return fail(MYO_E_ARG, "stand task: ntarget must be 3 (target position)");
    if (!(m->wave_ok && m->dw.has_free && nq == nv + 1)) return fail(MYO_E_UNSUPPORTED, "stand task needs a model with a free root joint");
    b->task.obs_dim = nq + nv + 6 + na;
  } else {
    if (c->ntarget != 3) return fail(MYO_E_ARG, "hold task: ntarget must be 3 (goal position)");
    if (!(m->wave_ok && m->dw.has_free && nq == nv + 1 && nv > 6)) return fail(MYO_E_UNSUPPORTED, "hold task needs a model whose last joint is one free object");
    b->task.obs_dim = (nq - 7) + (nv - 6) + 6 + na;
  }
  return MYO_OK;
}
static const TaskHooks state_hooks = {state_configure, launch_task_obs<StateTask>, launch_task_post<StateTask>};

// reach needs tip positions: its observation reuses the lanes kernel's kinematics stage and has no fused epilogue
static int reach_configure(myo_batch* b, const myo_task_config* c) {
  if (c->ntarget != 3 * c->ntip) return fail(MYO_E_ARG, "reach task: ntarget must be 3*ntip");
  b->task.obs_dim = 2 * b->model->dm.nv + 6 * c->ntip + b->model->dm.na_obs;
  return MYO_OK;
}
static int reach_obs(myo_batch* b, hipStream_t s, int obs_only, int) {
  const int EPW = 4;
  hipLaunchKernelGGL(reach_obs_kernel<16>, dim3((b->db.B + EPW - 1) / EPW), dim3(64), (size_t)EPW * b->model->env_lds_bytes, s, b->model->dm, b->db, b->task, obs_only);
  return MYO_OK;
}
static const TaskHooks reach_hooks = {reach_configure, reach_obs, nullptr};

// the walk observation lives in the step kernel: run it with zero substeps as an observation-only pass (configured by myo_batch_configure_walk;
// in myo_bench_rollout the step launch itself observes)
static int walk_obs(myo_batch* b, hipStream_t s, int obs_only, int reset_only) {
  return launch_step(b, nullptr, MYO_ACTMAP_NONE, 0, s, KF_AUX | (obs_only ? KF_OBS_ONLY : 0) | (reset_only ? KF_RESET_ONLY : 0));
}
static const TaskHooks walk_hooks = {nullptr, walk_obs, nullptr};

static const TaskHooks* task_hooks(int task) {
  switch (task) {
    case MYO_TASK_POSE: case MYO_TASK_STAND: case MYO_TASK_HOLD: return &state_hooks;
    case MYO_TASK_REACH: return &reach_hooks;
    case MYO_TASK_WALK: return &walk_hooks;
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

}  // extern "C"
