// myo_host.h -- what every host file shares: error reporting, the helpers each subsystem would otherwise write out again (device-memory
// pool, device selection, blob view, kernel attributes), myo_model, myo_batch, and the per-task hook record with its two generic launchers.
#ifndef MYO_HOST_H
#define MYO_HOST_H

#include <memory>

static int g_lanes = 64;  // lanes per env (16 / 32 / 64); MYO_LANES env var or myo_set_lanes(); 64 = wave-per-env kernel
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(MYO_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// The device memory of one host object (model, batch, policy, learner): allocations live as long as the object and are freed with it, so a
// half-built object held in a unique_ptr frees what it had allocated on any failure path.  Sizes are in bytes; alloc zero-fills
struct DevPool {
  std::vector<void*> ptrs;
  DevPool() = default;
  DevPool(const DevPool&) = delete;
  DevPool& operator=(const DevPool&) = delete;
  ~DevPool() { for (void* p : ptrs) (void)hipFree(p); }
  template <class T> int alloc(T** out, size_t nbytes, bool zero = true) {
    void* p = nullptr;
    const hipError_t e = hipMalloc(&p, nbytes);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? MYO_E_NOMEM : MYO_E_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    ptrs.push_back(p);
    if (zero) HIPCHK(hipMemset(p, 0, nbytes));
    *out = (T*)p;
    return MYO_OK;
  }
  // n elements of src followed by `pad` zero elements (at least 8 bytes, so an empty table still has an address).  (out is a template so
  // that the device-side address-space types of the struct fields do not matter to this host code)
  template <class T, class P> int upload(P* out, const T* src, size_t n, size_t pad = 0) {
    T* p = nullptr;
    const int rc = alloc(&p, std::max<size_t>((n + pad) * sizeof(T), 8));
    if (rc) return rc;
    if (n) HIPCHK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    *out = (P)(const T*)p;
    return MYO_OK;
  }
};

// `device` is an ordinal of this machine: make it the calling thread's current device
static int use_device(int device, const char* who, const char* note = "") {
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MYO_E_HIP, std::string(who) + ": no such HIP device" + note);
  HIPCHK(hipSetDevice(device));
  return MYO_OK;
}

struct BlobRec { char name[32]; uint32_t dtype, ndim, shape[4]; uint64_t nbytes, offset; };

// Read-only view of a MYOB v3 blob.  ints / floats / doubles return host vectors and allocate nothing on the device.  A missing or mistyped
// array comes back empty and leaves the first such error in rc (MYO_E_BLOB, the array's name in the message): read, then check rc, then use
struct Blob {
  const uint8_t* p;
  mutable int rc = MYO_OK;
  const BlobRec* find(const char* name) const {
    uint32_t n;
    memcpy(&n, p + 8, 4);
    for (uint32_t i = 0; i < n; i++) {
      const BlobRec* r = (const BlobRec*)(p + 16 + (size_t)i * sizeof(BlobRec));
      if (!strncmp(r->name, name, 32)) return r;
    }
    return nullptr;
  }
  bool has(const char* name) const { return find(name) != nullptr; }
  template <class Src, class Dst> std::vector<Dst> read(const char* name, uint32_t dtype) const {
    const BlobRec* r = find(name);
    if (!r || r->dtype != dtype) {
      if (!rc) rc = fail(MYO_E_BLOB, std::string("model blob lacks ") + (dtype ? "i32" : "f64") + " array " + name);
      return {};
    }
    const Src* s = (const Src*)(p + r->offset);
    return std::vector<Dst>(s, s + r->nbytes / sizeof(Src));
  }
  std::vector<int> ints(const char* name) const { return read<int, int>(name, 1); }
  std::vector<float> floats(const char* name) const { return read<double, float>(name, 0); }   // f64 narrowed to float
  std::vector<double> doubles(const char* name) const { return read<double, double>(name, 0); }
};
// the view of a caller's blob, after the magic and version check
static int blob_open(const void* blobv, size_t nbytes, const char* who, Blob* B) {
  uint32_t ver = 0;
  if (nbytes >= 16) memcpy(&ver, (const uint8_t*)blobv + 4, 4);
  if (nbytes < 16 || memcmp(blobv, "MYOB", 4) || ver != 3) return fail(MYO_E_BLOB, std::string(who) + ": not a MYOB v3 blob");
  B->p = (const uint8_t*)blobv;
  return MYO_OK;
}

// hipFuncAttributeMaxDynamicSharedMemorySize for every kernel of a list, once per device: kernel attributes are per device, so each list
// keeps one flag per device ordinal (a process that opens models on two GPUs).  A list holds records with the kernel in `fn`
struct OncePerDevice { std::mutex mu; bool done[64] = {}; };
template <class Kernels> static int set_lds_limit(OncePerDevice& once, const Kernels& kernels, int nbytes, int device) {
  std::lock_guard<std::mutex> lock(once.mu);
  bool& done = once.done[device & 63];
  if (done) return MYO_OK;
  for (const auto& k : kernels) HIPCHK(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, nbytes));
  done = true;
  return MYO_OK;
}

struct myo_model {
  int device = 0;
  DevModel dm{};
  DevModelW dw{};
  DevModel* d_dm = nullptr;     // device copies of the model structs for the wave kernel
  DevModelW* d_dw = nullptr;
  int env_lds_bytes_w = 0;
  bool wave_ok = false, generic_ok = false;
  int n_cu = 0;                 // compute units of the model's device (scheduler sizing)
  int kin_floats = 0;           // LDS scratch the two-phase kinematics needs (lowering.py hip_kin_size)
  bool rk4 = false;             // <option integrator="RK4">: the RK4 instantiations of the wave kernel (generic sizes, no scheduler)
  bool trk = false;             // TrackEnv model class: step_kernel_w<36,20,32,2,2,false,0,false,true>
  bool hand_sizes = false, leg_sizes = false, terrain_sizes = false;   // table sizes equal Sizes<1> / Sizes<2> / Sizes<3>: the size-specialised instantiations may be used
  int wave_cfg = 0;             // 0: step_kernel_w<24,8,32,1,...> (hand / finger), 1: step_kernel_w<36,20,32,2,2,...> (legs), 2: the TRK instantiation
  int nq = 0;
  int has_tl = 0;
  bool has_affine = false;   // some actuator is a stateless affine one (motor / position / velocity): wave kernel only
  myo_dims dims{};
  DevPool pool;
  std::vector<float> qpos0, jnt_lo, jnt_hi;
  std::vector<int> dof_type, dof_link, link_parent, link_dofnum, site_link;   // host copies of the uploaded tables the task checks read
  std::vector<int> cg_geom, cg_type_h;   // collision geom -> compiled geom id, and its type (host copies)
  std::vector<int> body_link;                       // body -> link, pose of the body inside the link frame (walk task)
  std::vector<float> body_lpos, body_lquat, mass;   // mass = [total, static bodies' mass-weighted COM xyz]
  float* d_qpos0 = nullptr;
  int env_lds_bytes = 0;
  // per-env body masses (MYO_F_BODYMASS): the compiled body_mass and, per link, its member bodies (CSR) with their COM (3), inertia
  // about the COM (6) in the link frame and compiled mass -- the per-body constants of lowering.py's link recomposition (link_compose_kernel)
  std::vector<float> body_mass0;
  const int *d_lm_adr = nullptr, *d_lm_body = nullptr;
  const double* d_lm_tab = nullptr;
  // per-env translation of one root body (MYO_F_BODYPOS): the link headed by the body that carries the model's last joint, when that body
  // is a child of the world heading a root link of a TrackEnv-class model; -1 otherwise
  int bp_link = -1;
  // per-env orientation of one world-welded body (MYO_F_BODYQUAT): compiled body tree, poses and the bodies of the collision geoms / sites
  std::vector<int> body_parent, body_jntnum, cg_body, site_body;
  std::vector<double> body_pos0, body_quat0;
  std::vector<double> site_pos0;   // compiled site_pos (site in its body's frame): the baoding task's moving targets keep its z
  // forward pass (myo_kernel_forward.h): the per-body / site / geom export records and the collision geoms' model ids, built at load
  bool fwd_ok = false, fwd_site_mat = false;
  int fwd_nbody = 0, fwd_nsite = 0, fwd_ngeom = 0, fwd_ncap = 0;
  const float *d_fwd_body = nullptr, *d_fwd_site = nullptr, *d_fwd_geom = nullptr;
  const int* d_fwd_cg_geom = nullptr;
  // per-env object parameters (myo_host_objects.h): the compiled geom and body arrays a selection is checked against and starts from, as
  // the blob has them (all optional there: a blob without them refuses the subsystem)
  bool obj_ok = false;
  std::vector<int> geom_type0, geom_body0, geom_priority0;
  std::vector<double> geom_size0, geom_pos0, geom_friction0, body_mass_d;
};

// episode statistics (myo_batch_enable_episode_stats): running and last-finished rows [B][4] = dense return, sparse return, length, solved
// steps; a byte per env raised by the update that ended its episode; episodes ended per env.  run == nullptr: off
struct myo_episode { float *run = nullptr, *last = nullptr; uint8_t* finished = nullptr; int* count = nullptr; };

// observation terms (myo_batch_enable_obs_terms, myo_obs_terms.h): the three rows [B][wt] all terms, [B][ws] the obs_keys concatenation, [B][wp]
// the proprio_keys one (prop == nullptr, wp == 0: none), the column program (one (source, index) record per float of the three rows laid
// end to end) and the constant table.  terms == nullptr: off
struct myo_obs_terms { float *terms = nullptr, *sel = nullptr, *prop = nullptr; const int2* prog = nullptr; const float* cst = nullptr; int wt = 0, ws = 0, wp = 0; };

struct myo_batch {
  const myo_model* model = nullptr;
  DevBatch db{};
  TaskDev task{};
  int ntarget_alloc = 0, obs_alloc = 0, env_offset = 0;
  DevPool pool;
  float *d_tlo = nullptr, *d_thi = nullptr, *d_init = nullptr, *d_jlo = nullptr, *d_jhi = nullptr, *d_action = nullptr, *d_rnd = nullptr;
  float* d_initv = nullptr;
  float *d_init2 = nullptr, *d_initv2 = nullptr, *d_fatvec = nullptr;   // walk reset "random": second keyframe; fatigue reset vector
  const char* last_kernel = "step_kernel";   // name of the step-kernel instantiation of the last myo_step / bench launch
  DevWalk* d_walk = nullptr;
  DevTrack* d_track = nullptr;    // MYO_TASK_TRACK: device copy of the task record (tables hang off it)
  float* d_metrics = nullptr;     // [B][4]
  int track_frames = 0;
  int track_flavour = 0;          // myo_track_config.flavour: 0 MJX (fused into the step kernel), 1 classic gym TrackEnv (task_obs_kernel<MyodmTask>)
  ResetArgs *d_reset = nullptr, reset_args{};   // task_post_kernel's copy of (db, task) in device memory, and what was last uploaded to it (launch_task_post)
  uint64_t reset_seed = 0;        // seed of the last myo_reset / myo_autoreset (classic flavour: keys the RANDOM reference draws)
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  uint64_t bench_step = 0;
  long long* d_stamps = nullptr;
  int* d_order = nullptr;
  int* d_sched = nullptr;       // substep scheduler: 8 queues x (4 control words + ring)
  int sched_stride = 0;
  int balance = 1;
  bool bm_on = false;            // per-env body-mass override started (DevBatch.bmass / bmass_range / linkc allocated)
  bool bp_on = false;            // per-env root-body offset started (DevBatch.bpos / bpos_range allocated)
  int bq_body = -1;              // body of MYO_F_BODYQUAT (myo_task_config.quat_body; -1: none selected)
  bool sens_on = false;          // touch sensors / contact forces enabled (DevBatch.sens / cfrc allocated)
  myo_episode episode;           // episode statistics (device buffers in pool)
  myo_obs_terms obs_terms;       // observation-term rows (device buffers in pool)
  bool bq_on = false;            // per-env body orientation started (DevBatch.bquat / bquat_range / bq_c / bq_flag allocated)
  bool fwd_on = false;           // forward buffers allocated (the first myo_forward)
  void* fwd_buf[16] = {};        // ... one per MYO_FWD_* id
  bool obj_on = false;           // per-env object parameters enabled (myo_objects_enable: DevBatch.obj* allocated)
  std::vector<int> obj_geoms, obj_bodies;   // ... the selection, model ids
  float *d_objk = nullptr, *d_obj_draw = nullptr;   // ... the composed rows and the draw table (non-const twins of DevBatch.objk / obj_draw)
  int* d_obj_draw_k = nullptr;
  std::vector<hipEvent_t> kev;   // per-launch event pairs around the step kernel (bench only)
  int kev_pending = 0;           // pairs recorded by asynchronous bench calls and not collected yet
  float last_kernel_ms = 0.f;
  ~myo_batch() {
    for (hipEvent_t e : kev) (void)hipEventDestroy(e);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
  }
};

// ---- device buffers handed to the caller.  Every family (batch fields, reward row, episode buffers, observation-term rows, forward buffers, object tables) keeps
// one function with its own refusals that yields a DevBuf; the lookup, read and write entry points are argument checks plus the pieces below.
struct DevBuf { void* p; size_t width, elem; };   // device pointer, elements per env row (pitch = width everywhere), bytes per element
typedef int (*BufFamily)(const myo_batch*, int which, DevBuf*);
static int buf_out(const DevBuf& d, void** dev_ptr, size_t* pitch, size_t* width) { *dev_ptr = d.p; *pitch = *width = d.width; return MYO_OK; }
// blocking copies: after everything enqueued on `device` has run.  Zero bytes: the wait alone
static int copy_blocking(int device, void* dst, const void* src, size_t nbytes, hipMemcpyKind kind) {
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipDeviceSynchronize());
  if (nbytes) HIPCHK(hipMemcpy(dst, src, nbytes, kind));
  return MYO_OK;
}
static int copy_to_host(int device, void* host, const void* dev, size_t nbytes) { return copy_blocking(device, host, dev, nbytes, hipMemcpyDeviceToHost); }
static int copy_to_device(int device, void* dev, const void* host, size_t nbytes) { return copy_blocking(device, dev, host, nbytes, hipMemcpyHostToDevice); }
// a host array of the whole buffer: B rows of width elements.  `mismatch` is the caller's error text
static int buf_check(const myo_batch* b, const DevBuf& d, const void* host, size_t nbytes, const char* mismatch) {
  return host && nbytes == (size_t)b->db.B * d.width * d.elem ? MYO_OK : fail(MYO_E_ARG, mismatch);
}
// the lookup and the read of a family (a write validates between buf_check and copy_to_device)
static int buf_lookup(BufFamily family, const myo_batch* b, int which, void** dev_ptr, size_t* pitch, size_t* width, const char* null_text) {
  if (!b || !dev_ptr || !pitch || !width) return fail(MYO_E_ARG, null_text);
  DevBuf d;
  const int rc = family(b, which, &d);
  return rc ? rc : buf_out(d, dev_ptr, pitch, width);
}
static int buf_read(BufFamily family, const myo_batch* b, int which, void* host, size_t nbytes, const char* mismatch) {
  DevBuf d; int rc;
  if ((rc = family(b, which, &d)) || (rc = buf_check(b, d, host, nbytes, mismatch))) return rc;
  return copy_to_host(b->model->device, host, d.p, nbytes);
}

// the two tables a task states beside its row record.  Reward columns (include/myo_hip_rewards.h): the keys of the reference's rwd_dict, in
// its order.  Observation terms (include/myo_hip_obs.h): the keys of its get_obs_dict, in its order, one ObsTerm per key: name, width, source,
// index of the term's first float inside the source's row; `dim` is the width of the canonical row.  Widths and indices are arithmetic on
// ObsDims only, so the table needs no batch and no device (myo_obs_term_table)
struct RwdCols { const char* const* name; int n; };
struct ObsDims { int nq, nv, nu, na, ntip, pose_act; };   // na: muscles (MuJoCo's na); pose_act: na, or nq when the model has no muscles
enum { OBS_SRC_ROW = 0,      // MYO_F_OBS, the canonical row (values already scaled: qvel * dt)
       OBS_SRC_TIME = 1,     // MYO_F_TIME
       OBS_SRC_TARGET = 2,   // MYO_F_TARGET
       OBS_SRC_QPOS = 3,     // MYO_F_QPOS
       OBS_SRC_ACT = 4,      // MYO_F_ACT; index = slot in sim.data.act order, mapped to its actuator when the program is built
       OBS_SRC_CONST = 5 };  // the batch's constant table: [0, 3) the pen's eps_ball site, [3, 3 + nq) zeros
struct ObsTerm { const char* name; int width, src, idx; };
struct ObsTable : std::vector<ObsTerm> { int dim = 0; };

// What differs per task on the host, indexed by task id (task_hooks in myo_host_tasks.h); a task's record lives next to its kernel.
struct TaskHooks {
  int (*configure)(myo_batch*, const myo_task_config*);                    // argument and model checks, obs_dim, task-specific TaskDev fields; null: no observation row,
                                                                           // or a task with a config record of its own (walk_configure, track_configure)
  int (*obs)(myo_batch*, hipStream_t, int obs_only, int reset_only);       // observation launch; null: the task has none
  int (*post)(myo_batch*, hipStream_t, uint64_t seed, int auto_max);       // myo_bench_rollout's fused epilogue; null: observation, auto-reset and re-observation are three launches
  RwdCols rwd;                                                             // reward-term columns, `dense` last; {null, 0}: the task has no term row (the MyoDM track task)
  void (*obs_terms)(const ObsDims&, ObsTable&);                            // fills the observation-term table from the task's row record; null: no table (track)
};
static const TaskHooks* task_hooks(int task);   // myo_host_tasks.h
// the step launch (myo_host_step.h): the walk task observes through it
static int launch_step(myo_batch* b, const float* action, int actmap, int nsub, hipStream_t s, int kflags = 0);

template <class Task> static int launch_task_obs(myo_batch* b, hipStream_t s, int obs_only, int reset_only) {
  hipLaunchKernelGGL(task_obs_kernel<Task>, dim3(b->db.B), dim3(64), 0, s, b->model->dm, b->db, b->task, (const DevTrack*)b->d_track, b->reset_seed, obs_only, reset_only);
  return MYO_OK;
}
// the device copy of (db, task) that task_post_kernel's reset reads: uploaded on the launch's stream whenever either record has changed
static int sync_reset_args(myo_batch* b, hipStream_t s) {
  if (!b->d_reset) { const int rc = b->pool.alloc(&b->d_reset, sizeof(ResetArgs), false); if (rc) return rc; }   // (not filled: the copy below writes all of it, on s)
  else if (!memcmp(&b->reset_args.Bt, &b->db, sizeof(DevBatch)) && !memcmp(&b->reset_args.T, &b->task, sizeof(TaskDev))) return MYO_OK;
  memcpy(&b->reset_args.Bt, &b->db, sizeof(DevBatch)); memcpy(&b->reset_args.T, &b->task, sizeof(TaskDev));
  HIPCHK(hipMemcpyAsync(b->d_reset, &b->reset_args, sizeof(ResetArgs), hipMemcpyHostToDevice, s));
  return MYO_OK;
}
template <class Task> static int launch_task_post(myo_batch* b, hipStream_t s, uint64_t seed, int auto_max) {
  const int rc = sync_reset_args(b, s);
  if (rc) return rc;
  hipLaunchKernelGGL(task_post_kernel<Task>, dim3(b->db.B), dim3(64), 0, s, b->model->dm, b->db, b->task, (const DevTrack*)b->d_track,
                     (const ResetArgs*)b->d_reset, b->model->nq, b->model->dm.qpos0, seed, b->env_offset, auto_max);
  return MYO_OK;
}

// the dofs [d0, d0 + n) are all the dofs of one root link: that link, or -1
static int root_link_of_dofs(const myo_model* m, int d0, int n) {
  const int l = m->dof_link[d0];
  if (m->link_parent[l] >= 0 || m->link_dofnum[l] != n) return -1;
  for (int k = 1; k < n; k++) if (m->dof_link[d0 + k] != l) return -1;
  return l;
}

static void quat2mat_d(double* R, const double* q) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = w * w + x * x - y * y - z * z; R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = w * w - x * x + y * y - z * z; R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = w * w - x * x - y * y + z * z;
}

#endif  // MYO_HOST_H
