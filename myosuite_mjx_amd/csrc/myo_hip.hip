// myo_hip.hip -- MI355X (gfx950) batched musculoskeletal stepper: kernels + C ABI (include/myo_hip.h).
//
// One translation unit, split over csrc/ for readability:
//   myo_common.h        limits, device-side structs (model tables, per-env batch arrays, task records), the counter RNG and the table of its streams, vector math
//   myo_physics.h       tendon wrapping, muscle model, action map (+ muscle conditions), impedance, contact frames, MPR
//   myo_task_track.h    MyoDM TrackEnv as a fused task of the TRK step kernel: reference lookup, reward / done, masked reset
//   myo_kernel_lanes.h  step_kernel<G>: the first kernel, G = 16 / 32 / 64 lanes per env, all state in LDS (cross-check / fallback)
//   myo_kernel_wave.h   step_kernel_w: one env per 64-lane wavefront (default): LDS layout, substep scheduler, size specialisations, the kernel body
//   myo_kernel_wave_body.h  ... the text of the kernel body, compiled into step_kernel_w and into step_kernel_obj (per-env object parameters)
//   myo_wave_util.h     its cross-lane / register helpers, WaveCfg (what the template parameters imply), con_row, the stage context
//   myo_wave_motion.h   its stages: state check, kinematics, tendons and muscles, CRB + RNE, integration
//   myo_wave_collision.h   broad phase, narrow phase
//   myo_wave_solver.h   constraint rows, packed mass matrix, sensor readout, task epilogues (the solver itself is inline in the kernel)
//   myo_ldl_mfma.h      dense LDL^T of the Newton Hessian on the FP32 matrix cores (included by myo_wave_util.h)
//   myo_reset.h         the reset of an env: its pieces (one per owner), reset_body, reset_kernel, ResetArgs; and, compiled by a second inclusion
//                       after myo_host.h (launch_reset needs myo_batch, which holds a ResetArgs), launch_reset, myo_reset and myo_autoreset
//   myo_kernels_aux.h   placement hint, random actions, link recomposition, task_obs_kernel / task_post_kernel
//   myo_kernels_diag.h  the poison kernels of the diagnostic build, the VALU issue-rate probe
//   myo_kernels_ppo.h   policy inference; PPO training: policy sampling with log-probabilities, GAE (include/myo_hip_ppo.h)
//   myo_kernels_learner.h  the PPO SGD step: both MLPs forward and backward on the FP32 MFMA, loss, Adam (include/myo_hip_ppo.h)
// Host side: a subsystem's host record, its launches and the entry points of its public header live in one file
//   myo_host.h          shared by all of them: error reporting, device-memory pool (DevPool), use_device, blob view (Blob, blob_open), kernel
//                       attributes once per device (set_lds_limit), myo_model, myo_batch, the device buffers handed to callers (DevBuf, buf_lookup,
//                       buf_read, the blocking copies), the per-task hook record (TaskHooks) and its launchers
//   myo_rewards.h       reward-term rows and episode statistics (include/myo_hip_rewards.h): walk term kernel, statistics kernel, entry points (a task's columns: its hook record)
//   myo_obs_terms.h     observation-term rows (include/myo_hip_obs.h): column program, obs_terms_kernel, entry points (a task's term table: its hook record)
//   myo_host_tasks.h    the task table: includes the task files below, task_hooks, launch_obs; what a new task consists of
//   myo_task_util.h     what the task files share: link-chain walk, row prologue, site gather, activation term, the table macros, the common configure checks
//   myo_task_<name>.h   pose, reach, walk, stand, hold, keyturn, pen, baoding, die, myodm: a task's row record (the blocks of its observation row; the walk
//                       task's is in myo_common.h), the observation body that writes through it, its configure, its reward columns and observation-term
//                       table, and the hook record that carries them
//   myo_host_model.h    myo_model_load in pieces: table upload, packing of the per-lane records, kernel class
//   myo_host_batch.h    batch creation, the per-env override records, the table of fields behind myo_batch_field / read / write
//   myo_host_objects.h  per-env object parameters (include/myo_hip_objects.h): selection, tables, the per-launch compose kernel, draw table, entry points
//   myo_host_step.h     the table of step-kernel instantiations, launch_step, myo_bench_rollout and the other timing entry points
//   myo_kernel_forward.h   forward_kernel_w: frames and contact list without a step (include/myo_hip_forward.h), its export tables and buffers
//   myo_host_forward.h  ... its instantiations, launch and entry points
//   myo_host_policy.h   myo_policy: load, act, update, sample; myo_ppo_gae (include/myo_hip.h, include/myo_hip_ppo.h)
//   myo_host_learner.h  myo_ppo_learner: create, tensor views, the SGD step's launches (include/myo_hip_ppo.h)
//   myo_hip.hip         this map, the include list and the core entry points of include/myo_hip.h (and myo_hip_sensors.h): model, batch, configure,
//                       step, observation, status, set-state and the small setters
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
#include "myo_reset.h"
#include "myo_kernels_aux.h"
#include "myo_kernels_diag.h"
#include "myo_kernels_ppo.h"
#include "myo_kernels_learner.h"
#include "myo_host.h"
#include "myo_reset.h"   // its host half (see the map)
#include "myo_rewards.h"
#include "myo_host_tasks.h"
#include "myo_obs_terms.h"
#include "myo_host_model.h"
#include "myo_host_batch.h"
#include "../../include/myo_hip_objects.h"
#include "myo_host_objects.h"
#include "myo_host_step.h"
#include "../../include/myo_hip_forward.h"
#include "myo_kernel_forward.h"
#include "myo_host_forward.h"
#include "myo_host_policy.h"
#include "myo_host_learner.h"

extern "C" {

const char* myo_last_error(void) { return g_err.c_str(); }
int myo_version(void) { return 1; }

int myo_model_load(const void* blobv, size_t nbytes, int device, myo_model** out) {
  if (!blobv || !out || nbytes < 16) return fail(MYO_E_ARG, "myo_model_load: bad arguments");
  Blob B{};
  int rc = blob_open(blobv, nbytes, "myo_model_load", &B);
  if (rc || (rc = use_device(device, "myo_model_load", " (a GPU is required; there is no CPU fallback)"))) return rc;
  std::unique_ptr<myo_model> m(new myo_model());   // a failed load frees what it had uploaded
  m->device = device;
  { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess) m->n_cu = prop.multiProcessorCount; }
  if ((rc = load_model(m.get(), B)) || (rc = fwd_model_tables(m.get(), B)) || (rc = obj_model_tables(m.get(), B))) return rc;
  *out = m.release();
  return MYO_OK;
}

void myo_model_free(myo_model* m) { delete m; }

int myo_model_dims(const myo_model* m, myo_dims* out) {
  if (!m || !out) return fail(MYO_E_ARG, "myo_model_dims: null");
  *out = m->dims;
  return MYO_OK;
}

int myo_model_nsensor(const myo_model* m) { return m ? m->dw.ntouch : 0; }

int myo_model_set_switch(myo_model* m, int dc, int dl, int de) {
  if (!m) return fail(MYO_E_ARG, "null model");
  m->dm.disable_contact = dc; m->dm.disable_limit = dl; m->dm.disable_ellipsoid = de;
  return m->d_dm ? copy_to_device(m->device, m->d_dm, &m->dm, sizeof(DevModel)) : MYO_OK;
}

// batches, per-env fields and overrides: myo_host_batch.h
int myo_batch_create(const myo_model* m, int B, myo_batch** out) { return m && out && B > 0 ? batch_create(m, B, out) : fail(MYO_E_ARG, "myo_batch_create: bad arguments"); }
void myo_batch_free(myo_batch* b) { delete b; }
int myo_batch_enable_sensors(myo_batch* b) { return b ? enable_sensors(b) : fail(MYO_E_ARG, "myo_batch_enable_sensors: null"); }
int myo_batch_field(myo_batch* b, int field, void** p, size_t* pitch, size_t* width) { return b && p && pitch && width ? batch_field(b, field, p, pitch, width) : fail(MYO_E_ARG, "myo_batch_field: null"); }
int myo_batch_read(myo_batch* b, int field, void* host, size_t nbytes) { return b && host ? batch_read(b, field, host, nbytes) : fail(MYO_E_ARG, "myo_batch_read: null"); }
int myo_batch_write(myo_batch* b, int field, const void* host, size_t nbytes) { return b && host ? batch_write(b, field, host, nbytes) : fail(MYO_E_ARG, "myo_batch_write: null"); }

int myo_batch_size(const myo_batch* b) { return b ? b->db.B : 0; }

int myo_batch_configure(myo_batch* b, const myo_task_config* c) {
  if (!b || !c) return fail(MYO_E_ARG, "myo_batch_configure: null");
  if (b->obs_terms.terms) return fail(MYO_E_ARG, OBS_TERMS_CONFIGURED);
  if (b->bm_on && c->task == MYO_TASK_STAND) return fail(MYO_E_UNSUPPORTED, "per-env body masses: the stand task uses model-wide mass totals");
  const DevModel& dm = b->model->dm;
  TaskDev& T = b->task;
  int nv = dm.nv, nu = dm.nu;
  if (c->ntarget > b->ntarget_alloc || c->ntip > 8) return fail(MYO_E_ARG, "myo_batch_configure: ntarget/ntip too large");
  if (c->quat_body > 0) { int rc = set_quat_body(b, c->quat_body); if (rc) return rc; }
  if (c->task == MYO_TASK_WALK) return fail(MYO_E_ARG, "use myo_batch_configure_walk for the walk task");
  if (b->db.rwd && rwd_cols(c->task).n != b->db.rwd_n) return fail(MYO_E_ARG, "reward terms are enabled for a task with other columns");
  T.init_qvel = nullptr; T.rnd = nullptr;
  T.terrain = 0; T.hf_n = 0; T.target_floor = -1;
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
    int rc = b->pool.alloc(&b->db.gsize, (size_t)b->db.B * 4 * 4);
    if (rc) return rc;
  }
  b->db.gsize_cg = cg;
  b->task.gsize_type = ty;
  for (int k = 0; k < 3; k++) { b->task.gsize_lo[k] = lo[k]; b->task.gsize_hi[k] = hi[k]; }
  return MYO_OK;
}

// the two tasks with a config record of their own: myo_task_walk.h, myo_task_myodm.h
int myo_batch_configure_walk(myo_batch* b, const myo_walk_config* c) {
  if (!b || !c) return fail(MYO_E_ARG, "myo_batch_configure_walk: null");
  return b->obs_terms.terms ? fail(MYO_E_ARG, OBS_TERMS_CONFIGURED) : walk_configure(b, c);
}
int myo_batch_configure_track(myo_batch* b, const myo_track_config* c) {
  if (!b || !c) return fail(MYO_E_ARG, "myo_batch_configure_track: null");
  return b->obs_terms.terms ? fail(MYO_E_ARG, OBS_TERMS_CONFIGURED) : track_configure(b, c);
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

int myo_step(myo_batch* b, const float* action_dev, int actmap, int nsubsteps, void* stream) {
  if (!b || nsubsteps < 0) return fail(MYO_E_ARG, "myo_step: bad arguments");
  if (b->task.task == MYO_TASK_TRACK && b->track_flavour == 1 && actmap == MYO_ACTMAP_CTRLRANGE)
    return fail(MYO_E_ARG, "myo_step: MYO_ACTMAP_CTRLRANGE is the MJX TrackEnv's action map; a batch of the classic flavour steps with MYO_ACTMAP_MUSCLE_SIGMOID");
  HIPCHK(hipSetDevice(b->model->device));
  return launch_step(b, action_dev, actmap, nsubsteps, (hipStream_t)stream);
}

// the task's observation pass (launch_obs, myo_host_tasks.h): with reward / done / solved, the row alone, or the row of the envs just reset
static int obs_entry(myo_batch* b, void* stream, int obs_only, int reset_only, const char* null_text) {
  if (!b) return fail(MYO_E_ARG, null_text);
  HIPCHK(hipSetDevice(b->model->device));
  const int rc = launch_obs(b, (hipStream_t)stream, obs_only, reset_only);
  // the observation-term rows follow MYO_F_OBS (the walk task's observation is a step launch: launch_wave has run the kernel)
  return !rc && b->obs_terms.terms && b->task.task != MYO_TASK_WALK ? obs_terms_launch(b, (hipStream_t)stream) : rc;
}
int myo_obs(myo_batch* b, void* stream) { return obs_entry(b, stream, 0, 0, "myo_obs: null"); }
int myo_obs_only(myo_batch* b, void* stream) { return obs_entry(b, stream, 1, 0, "myo_obs_only: null"); }
int myo_obs_reset_only(myo_batch* b, void* stream) { return obs_entry(b, stream, 1, 1, "myo_obs_reset_only: null"); }

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
  if (mode == 2) { const int rc = copy_to_device(b->model->device, b->d_fatvec, fatigue_vec, (size_t)b->model->dm.nu * 4); if (rc) return rc; }
  b->task.fatigue_mode = mode; b->task.fatigue_vec = mode == 2 ? b->d_fatvec : nullptr;
  return MYO_OK;
}

int myo_status(myo_batch* b, int32_t* host_flags) {
  if (!b || !host_flags) return fail(MYO_E_ARG, "myo_status: null");
  if (const int rc = copy_to_host(b->model->device, host_flags, b->db.flags, (size_t)b->db.B * 4)) return rc;
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
  if (const int rc = copy_to_host(b->model->device, host, b->d_stamps, (size_t)nwg * 12 * sizeof(long long))) return rc;
  return MYO_STAMPS ? MYO_OK : 1;
}

int myo_sync(void* stream) {
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  return MYO_OK;
}

}  // extern "C"
