// myo_hip.hip -- MI355X (gfx950) batched musculoskeletal stepper: kernels + C ABI (include/myo_hip.h).
//
// One translation unit, split over csrc/ for readability:
//   myo_common.h        limits, device-side structs (model tables, per-env batch arrays, task records), vector math
//   myo_physics.h       tendon wrapping, muscle model, action map (+ muscle conditions), impedance, contact frames, MPR
//   myo_task_track.h    MyoDM TrackEnv as a fused task of the TRK step kernel: reference lookup, reward / done, masked reset
//   myo_kernel_lanes.h  step_kernel<G>: the first kernel, G = 16 / 32 / 64 lanes per env, all state in LDS (cross-check / fallback)
//   myo_kernel_wave.h   step_kernel_w: one env per 64-lane wavefront (default), substep scheduler, size-specialised instantiations
//   myo_kernels_aux.h   RNG, placement hint, random actions, policy inference, reset, observation kernels
//   myo_hip.hip         host side: model upload, batches, launches, the extern "C" entry points
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
#include "myo_task_keyturn.h"
#include "myo_task_pen.h"
#include "myo_task_baoding.h"
#include "myo_task_myodm.h"

// ================================================================================================
// host side
// ================================================================================================
static int g_lanes = 64;  // lanes per env (16 / 32 / 64); MYO_LANES env var or myo_set_lanes(); 64 = wave-per-env kernel
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(MYO_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

struct BlobRec { char name[32]; uint32_t dtype, ndim, shape[4]; uint64_t nbytes, offset; };

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
  bool hand_sizes = false, leg_sizes = false, terrain_sizes = false;   // table sizes equal Sizes<1> / Sizes<2>: the size-specialised instantiations may be used
  int wave_cfg = 0;             // 0: step_kernel_w<24,8,32,1,4> (hand / finger), 1: step_kernel_w<36,20,48,2,2> (legs)
  int nq = 0;
  int has_tl = 0;
  bool has_affine = false;   // some actuator is a stateless affine one (motor / position / velocity): wave kernel only
  myo_dims dims{};
  std::vector<void*> dev_allocs;
  std::vector<float> qpos0, jnt_lo, jnt_hi;
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
};

struct myo_batch {
  const myo_model* model = nullptr;
  DevBatch db{};
  TaskDev task{};
  int ntarget_alloc = 0, obs_alloc = 0, env_offset = 0;
  std::vector<void*> dev_allocs;
  float *d_tlo = nullptr, *d_thi = nullptr, *d_init = nullptr, *d_jlo = nullptr, *d_jhi = nullptr, *d_action = nullptr, *d_rnd = nullptr;
  float* d_initv = nullptr;
  float *d_init2 = nullptr, *d_initv2 = nullptr, *d_fatvec = nullptr;   // walk reset "random": second keyframe; fatigue reset vector
  const char* last_kernel = "step_kernel";   // name of the step-kernel instantiation of the last myo_step / bench launch
  DevWalk* d_walk = nullptr;
  DevTrack* d_track = nullptr;    // MYO_TASK_TRACK: device copy of the task record (tables hang off it)
  float* d_metrics = nullptr;     // [B][4]
  int track_frames = 0;
  int track_flavour = 0;          // myo_track_config.flavour: 0 MJX (fused into the step kernel), 1 classic gym TrackEnv (myodm_obs_kernel)
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
  bool bq_on = false;            // per-env body orientation started (DevBatch.bquat / bquat_range / bq_c / bq_flag allocated)
  std::vector<hipEvent_t> kev;   // per-launch event pairs around the step kernel (bench only)
  int kev_pending = 0;           // pairs recorded by asynchronous bench calls and not collected yet
  float last_kernel_ms = 0.f;
};

static const BlobRec* blob_find(const uint8_t* blob, const char* name) {
  uint32_t n;
  memcpy(&n, blob + 8, 4);
  for (uint32_t i = 0; i < n; i++) {
    const BlobRec* r = (const BlobRec*)(blob + 16 + (size_t)i * sizeof(BlobRec));
    if (!strncmp(r->name, name, 32)) return r;
  }
  return nullptr;
}

template <typename T> static int upload(myo_model* m, const std::vector<T>& v, const T** out) {
  void* p = nullptr;
  size_t nb = (v.size() + 4) * sizeof(T);
  HIPCHK(hipMalloc(&p, nb));
  HIPCHK(hipMemset(p, 0, nb));
  if (!v.empty()) HIPCHK(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
  m->dev_allocs.push_back(p);
  *out = (const T*)p;
  return 0;
}
// (out is a template so that the struct fields' device-side address-space types do not matter to this host code)
template <class P> static int load_f(myo_model* m, const uint8_t* blob, const char* name, P* out, std::vector<float>* keep = nullptr) {
  const BlobRec* r = blob_find(blob, name);
  if (!r || r->dtype != 0) return fail(MYO_E_BLOB, std::string("model blob lacks f64 array ") + name);
  size_t n = r->nbytes / 8;
  std::vector<float> v(n);
  const double* src = (const double*)(blob + r->offset);
  for (size_t i = 0; i < n; i++) v[i] = (float)src[i];
  if (keep) *keep = v;
  const float* tmp = nullptr;
  int rc = upload<float>(m, v, &tmp);
  *out = (P)tmp;
  return rc;
}
template <class P> static int load_i(myo_model* m, const uint8_t* blob, const char* name, P* out, std::vector<int>* keep = nullptr) {
  const BlobRec* r = blob_find(blob, name);
  if (!r || r->dtype != 1) return fail(MYO_E_BLOB, std::string("model blob lacks i32 array ") + name);
  size_t n = r->nbytes / 4;
  std::vector<int> v(n);
  memcpy(v.data(), blob + r->offset, n * 4);
  if (keep) *keep = v;
  const int* tmp = nullptr;
  int rc = upload<int>(m, v, &tmp);
  *out = (P)tmp;
  return rc;
}

static void build_layout_w(const DevModel& d, DevModelW& w, int nvt, int kc, int nc, int nj = 3) {
  w.lay = layout_w(w.nq, d.nv, d.nu, d.nl, d.ngt, d.maxnnz, d.ncg, w.has_tl != 0, nvt, kc, nc, nj);   // (myo_kernel_wave.h: shared with the compile-time layouts)
}

static void build_layout(DevModel& d) {
  Lay& Y = d.lay;
  int o = 0;
  auto take = [&](int n) { int r = o; o += n; return r; };
  int nv = d.nv, nu = d.nu, nl = d.nl, ntri = nv * (nv + 1) / 2;
  Y.qpos = take(nv); Y.qvel = take(nv); Y.act = take(nu); Y.ctrl = take(nu); Y.warm = take(nv);
  Y.lpos = take(3 * nl); Y.lmat = take(9 * nl); Y.lquat = take(4 * nl); Y.axis = take(3 * nv); Y.anchor = take(3 * nv);
  Y.tJ = take(d.ngt * d.maxnnz); Y.tlen = take(d.ngt); Y.tforce = take(nu); Y.actdot = take(nu);
  Y.qfa = take(nv); Y.smooth = take(nv); Y.qas = take(nv); Y.qacc = take(nv); Y.Ma = take(nv); Y.grad = take(nv);
  Y.search = take(nv); Y.Mv = take(nv); Y.qfc = take(nv);
  Y.Mp = take(ntri); Y.Hp = take(ntri);
  Y.lsign = take(nv); Y.laref = take(nv); Y.lD = take(nv); Y.ljar = take(nv); Y.ljv = take(nv);
  // region A (spatial dynamics) is dead once Mp / smooth exist; region B (collision + contact rows) aliases it
  int regA = o;
  Y.cdof = take(6 * nv); Y.cinert = take(10 * nl); Y.crb = take(10 * nl); Y.cvel = take(6 * nl); Y.cacc = take(6 * nl); Y.cfrc = take(6 * nl);
  int endA = o;
  o = regA;
  Y.gpos = take(3 * d.ncg); Y.gmat = take(9 * d.ncg); Y.cand = take(NCAND);
  Y.cdist = take(NCON); Y.cpos = take(3 * NCON); Y.cnrm = take(3 * NCON); Y.cpair = take(NCON); Y.cJ = take(NCON * 3 * KCMAX);
  Y.caref = take(4 * NCON); Y.cD = take(NCON); Y.cjar = take(4 * NCON); Y.cjv = take(4 * NCON); Y.cimp = take(NCON);
  if (o < endA) o = endA;
  // pad so that the 64/G env slices start on different LDS banks
  o = (o + 31) / 32 * 32 + 8;
  Y.total = o;
}

extern "C" {

const char* myo_last_error(void) { return g_err.c_str(); }
int myo_version(void) { return 1; }

int myo_model_load(const void* blobv, size_t nbytes, int device, myo_model** out) {
  if (!blobv || !out || nbytes < 16) return fail(MYO_E_ARG, "myo_model_load: bad arguments");
  const uint8_t* blob = (const uint8_t*)blobv;
  uint32_t ver;
  memcpy(&ver, blob + 4, 4);
  if (memcmp(blob, "MYOB", 4) || ver != 3) return fail(MYO_E_BLOB, "myo_model_load: not a MYOB v3 blob");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(MYO_E_HIP, "myo_model_load: no such HIP device (a GPU is required; there is no CPU fallback)");
  HIPCHK(hipSetDevice(device));
  myo_model* m = new myo_model();
  m->device = device;
  { hipDeviceProp_t prop; if (hipGetDeviceProperties(&prop, device) == hipSuccess) m->n_cu = prop.multiProcessorCount; }
  DevModel& d = m->dm;
  const BlobRec* hs = blob_find(blob, "hip_sizes");
  const BlobRec* sz = blob_find(blob, "sizes");
  const BlobRec* op = blob_find(blob, "opt");
  if (!hs || !sz || !op) { delete m; return fail(MYO_E_BLOB, "myo_model_load: blob lacks hip_* tables (run lowering)"); }
  const int* H = (const int*)(blob + hs->offset);
  const int* S = (const int*)(blob + sz->offset);
  const double* O = (const double*)(blob + op->offset);
  d.nl = H[0]; d.nlevel = H[1]; d.nv = H[2]; d.nu = H[3]; d.ngt = H[4]; d.nseg = H[5]; d.maxnnz = H[7]; d.nwg = H[8];
  d.ncg = H[9]; d.npair = H[10]; d.maxkc = H[11]; d.ns = H[12]; d.nM = S[11];
  m->nq = S[0];
  if (d.ngt != d.nu) { delete m; return fail(MYO_E_UNSUPPORTED, "limited-only tendons are not supported by the HIP path yet"); }
  d.timestep = (float)O[0]; d.grav[0] = (float)O[1]; d.grav[1] = (float)O[2]; d.grav[2] = (float)O[3];
  d.tolerance = (float)O[4]; d.iterations = (int)O[5]; d.ls_iterations = (int)O[6]; d.ls_tolerance = (float)O[7];
  d.meaninertia = (float)O[9];
  d.newton_scale = 1.0f / (d.meaninertia * (float)(d.nv > 1 ? d.nv : 1));
  int rc = 0;
  std::vector<float> c0, jl;
  const float* tmp;
#define LF(field, name) if ((rc = load_f(m, blob, name, &d.field))) { myo_model_free(m); return rc; }
#define LI(field, name) if ((rc = load_i(m, blob, name, &d.field))) { myo_model_free(m); return rc; }
  LI(level_adr, "hip_level_adr") LI(link_parent, "hip_link_parent") LI(link_dofadr, "hip_link_dofadr") LI(link_dofnum, "hip_link_dofnum")
  LI(child_adr, "hip_child_adr") LI(child, "hip_child") LI(dof_link, "hip_dof_link") LI(dof_type, "hip_dof_type")
  LI(dof_parent, "dof_parentid") LI(site_link, "hip_site_link") LI(wg_link, "hip_wg_link") LI(gt_seg_adr, "hip_gt_seg_adr")
  LI(gt_seg_num, "hip_gt_seg_num") LI(gt_dofs, "hip_gt_dofs") LI(seg, "hip_seg") LI(dl, "hip_dl") LI(col_adr, "hip_col_adr")
  LI(col, "hip_col") LI(cg_link, "hip_cg_link") LI(cg_type, "hip_cg_type") LI(pair_i, "hip_pair_i") LI(pair_dl, "hip_pair_dl")
  LF(link_pos, "hip_link_pos") LF(link_quat, "hip_link_quat") LF(link_mass, "hip_link_mass") LF(link_com, "hip_link_com")
  LF(link_inertia, "hip_link_inertia") LF(dof_pos, "hip_dof_pos") LF(dof_axis, "hip_dof_axis") LF(dof_damping, "dof_damping")
  LF(dof_armature, "dof_armature") LF(site_lpos, "hip_site_lpos") LF(wg_lpos, "hip_wg_lpos") LF(wg_lmat, "hip_wg_lmat")
  LF(wg_radius, "hip_wg_radius") LF(seg_div, "hip_seg_div") LF(gt_len0, "hip_gt_len0") LF(act, "hip_act") LF(cg_lpos, "hip_cg_lpos") LF(cg_lmat, "hip_cg_lmat")
  LF(cg_size, "hip_cg_size") LF(cg_rbound, "hip_cg_rbound") LF(pair_f, "hip_pair_f")
#undef LF
#undef LI
  if ((rc = load_f(m, blob, "qpos0", &d.qpos0, &m->qpos0))) { myo_model_free(m); return rc; }
  if ((rc = load_f(m, blob, "hip_jl", &d.jl, &jl))) { myo_model_free(m); return rc; }
  if ((rc = load_f(m, blob, "hip_c0", &tmp, &c0))) { myo_model_free(m); return rc; }
  d.c0[0] = c0[0]; d.c0[1] = c0[1]; d.c0[2] = c0[2];
  {
    std::vector<float> org;
    if ((rc = load_f(m, blob, "hip_origin", &tmp, &org))) { myo_model_free(m); return rc; }
    d.origin[0] = org[0]; d.origin[1] = org[1]; d.origin[2] = org[2];
  }
  m->jnt_lo.resize(d.nv); m->jnt_hi.resize(d.nv);
  for (int i = 0; i < d.nv; i++) { m->jnt_lo[i] = jl[12 * i + 1]; m->jnt_hi[i] = jl[12 * i + 2]; }
  build_layout(d);
  m->env_lds_bytes = d.lay.total * 4;
  {  // wave-per-env kernel tables (one env per wavefront, nv <= 24)
    DevModelW& w = m->dw;
    std::vector<int> nws;
    const int* tmpi;
    if ((rc = load_i(m, blob, "hip_seg_order", &w.seg_order)) || (rc = load_i(m, blob, "hip_seg_tendon", &w.seg_tendon)) ||
        (rc = load_i(m, blob, "hip_gt_dl", &w.gt_dl)) || (rc = load_f(m, blob, "hip_link_mat0", &w.link_mat0)) ||
        (rc = load_i(m, blob, "hip_nwrapseg", &tmpi, &nws))) { myo_model_free(m); return rc; }
    w.nwrapseg = nws[0];
    w.ndl = H[6];
    {
      std::vector<float> tlv;
      if ((rc = load_f(m, blob, "hip_tl", &w.tl, &tlv))) { myo_model_free(m); return rc; }
      w.has_tl = 0;
      for (int t = 0; t < d.ngt; t++) if (tlv[12 * t] != 0) w.has_tl = 1;
      m->has_tl = w.has_tl;
    }
    bool plane_pairs = false, condim1 = false;
    {
      std::vector<int> fl, pi;
      if ((rc = load_i(m, blob, "hip_flags", &tmpi, &fl)) || (rc = load_i(m, blob, "hip_link_free", &w.link_free)) ||
          (rc = load_i(m, blob, "hip_dof_qposadr", &w.dof_qposadr)) || (rc = load_i(m, blob, "hip_link_chain_adr", &w.link_chain_adr)) ||
          (rc = load_i(m, blob, "hip_link_chain", &w.link_chain)) || (rc = load_i(m, blob, "hip_eq_i", &w.eq_i)) ||
          (rc = load_i(m, blob, "hip_kin_base", &w.kin_base)) || (rc = load_i(m, blob, "hip_kin_adr", &w.kin_adr)) || (rc = load_i(m, blob, "hip_kin_vec", &w.kin_vec)) ||
          (rc = load_f(m, blob, "hip_eq_f", &w.eq_f)) || (rc = load_i(m, blob, "hip_pair_i", &tmpi, &pi))) { myo_model_free(m); return rc; }
      {
        std::vector<int> ks;
        if ((rc = load_i(m, blob, "hip_kin_size", &tmpi, &ks))) { myo_model_free(m); return rc; }
        m->kin_floats = ks[0];   // checked against the Hessian scratch (nvt x (nvt + 1)) once the kernel class is known
        w.kin_dnmax = ks.size() > 1 ? ks[1] : 6;
      }
      w.has_free = fl[0]; w.nq = fl[1]; w.neq = fl[2];
      if (fl.size() < 6) { myo_model_free(m); return fail(MYO_E_BLOB, "hip_flags: blob predates the actuator-kind tables; recompile the model"); }
      w.has_j0 = fl[3]; d.na_obs = fl[4]; m->has_affine = fl[5] != 0;
      { const int* t2; if ((rc = load_i(m, blob, "hip_cg_geom", &t2, &m->cg_geom)) || (rc = load_i(m, blob, "hip_cg_type", &t2, &m->cg_type_h))) { myo_model_free(m); return rc; } }
      {
        std::vector<int> hi; std::vector<float> hf; const float* tf2;
        if ((rc = load_i(m, blob, "hip_hf_i", &tmpi, &hi)) || (rc = load_f(m, blob, "hip_hf_f", &tf2, &hf))) { myo_model_free(m); return rc; }
        w.hf.on = hi[0]; w.hf.nrow = hi[1]; w.hf.ncol = hi[2]; w.hf.cg = hi[3];
        for (int k = 0; k < 4; k++) w.hf.size[k] = hf[k];
        for (int k = 0; k < 3; k++) w.hf.pos[k] = hf[4 + k];
        if (w.hf.on && (w.hf.nrow > 128 || w.hf.ncol > 100 || d.npair > 1023)) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "height field: at most 128 x 100 cells and 1023 pairs"); }
      }
      if ((rc = load_f(m, blob, "hip_gt_j0", &w.gt_j0)) || (rc = load_i(m, blob, "hip_act_obs", &d.act_obs))) { myo_model_free(m); return rc; }
      const float* tf;
      if ((rc = load_i(m, blob, "hip_body_link", &tmpi, &m->body_link)) || (rc = load_f(m, blob, "hip_body_lpos", &tf, &m->body_lpos)) ||
          (rc = load_f(m, blob, "hip_body_lquat", &tf, &m->body_lquat)) || (rc = load_f(m, blob, "hip_mass", &tf, &m->mass))) { myo_model_free(m); return rc; }
      if (w.nq != m->nq) { myo_model_free(m); return fail(MYO_E_BLOB, "hip_flags disagrees with sizes"); }
      for (int p = 0; p < d.npair; p++) { if (pi[6 * p + 4] >= 2) plane_pairs = true; if (pi[6 * p + 5] == 1) condim1 = true; }
      // the 16/32-lane generic kernel covers fixed-base models with hinge / slide joints and capsule / convex pairs only
      m->generic_ok = !w.has_free && w.neq == 0 && !plane_pairs && !condim1 && w.nq == d.nv && d.maxkc <= KCMAX && !w.has_tl && !m->has_affine;
    }
    // TrackEnv model class (lowering: hip_trk = condim-4 pairs | friction loss | box / hull geoms): tables of the TRK instantiation
    w.fl = nullptr; w.mesh_vert = nullptr; w.mesh_rec = nullptr; w.mesh_startrec = nullptr; w.mesh_aabb = nullptr;
    m->trk = false;
    if (blob_find(blob, "hip_trk")) {
      std::vector<int> tk;
      if ((rc = load_i(m, blob, "hip_trk", &tmpi, &tk)) || (rc = load_f(m, blob, "hip_fl", &w.fl)) || (rc = load_f(m, blob, "hip_mesh_vert", &w.mesh_vert)) ||
          (rc = load_f(m, blob, "hip_mesh_rec", &w.mesh_rec)) || (rc = load_f(m, blob, "hip_mesh_startrec", &w.mesh_startrec)) || (rc = load_f(m, blob, "hip_mesh_aabb", &w.mesh_aabb))) { myo_model_free(m); return rc; }
      m->trk = tk[0] || tk[1] || tk[2];
      if (m->trk) {   // bodies of MYO_F_BODYQUAT: the tree, compiled poses, and the body of every collision geom and site
        auto BI = [&](const char* n) { std::vector<int> v; const BlobRec* r = blob_find(blob, n); if (r && r->dtype == 1) { v.resize(r->nbytes / 4); memcpy(v.data(), blob + r->offset, r->nbytes); } return v; };
        auto BD = [&](const char* n) { std::vector<double> v; const BlobRec* r = blob_find(blob, n); if (r && r->dtype == 0) { v.resize(r->nbytes / 8); memcpy(v.data(), blob + r->offset, r->nbytes); } return v; };
        const std::vector<int> gb = BI("geom_bodyid");
        m->body_parent = BI("body_parentid"); m->body_jntnum = BI("body_jntnum"); m->site_body = BI("site_bodyid");
        m->body_pos0 = BD("body_pos"); m->body_quat0 = BD("body_quat"); m->site_pos0 = BD("site_pos");
        for (int g : m->cg_geom) m->cg_body.push_back(g >= 0 && g < (int)gb.size() ? gb[g] : -1);
      }
      if (m->trk) {   // the root body of MYO_F_BODYPOS: the body of the last joint, a child of the world at the origin of its own root link
        auto BI = [&](const char* n) { std::vector<int> v; const BlobRec* r = blob_find(blob, n); if (r && r->dtype == 1) { v.resize(r->nbytes / 4); memcpy(v.data(), blob + r->offset, r->nbytes); } return v; };
        const std::vector<int> jb = BI("jnt_bodyid"), jt = BI("jnt_type"), bp = BI("body_parentid"), bl = BI("hip_body_link"), lpar = BI("hip_link_parent");
        const int bb = jb.empty() ? -1 : jb.back();
        if (bb > 0 && jt.size() == jb.size() && (jt.back() == 2 || jt.back() == 3)   // a slide / hinge (a free root takes its pose from qpos)
            && bb < (int)bp.size() && bb < (int)bl.size() && bp[bb] == 0) {
          const int l = bl[bb];
          bool head = l >= 0 && l < (int)lpar.size() && lpar[l] < 0;
          for (int k = 1; head && k < bb; k++) if (bl[k] == l) head = false;   // the body heads its link (no earlier body welded into it)
          if (head) m->bp_link = l;
        }
      }
    }
    {  // plane - cylinder and plane - sphere pairs (lowering.py pair types 6 / 7 and 8) have a narrow phase in the TRK instantiation only: never
       // dropped silently
      std::vector<int> pi2;
      const int* t3;
      if ((rc = load_i(m, blob, "hip_pair_i", &t3, &pi2))) { myo_model_free(m); return rc; }
      for (int p = 0; p < d.npair; p++) {
        if ((pi2[6 * p + 4] == 6 || pi2[6 * p + 4] == 7) && !m->trk) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "plane - cylinder pairs need a model of the TrackEnv class"); }
        if (pi2[6 * p + 4] == 8 && !m->trk) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "plane - sphere pairs need a model of the TrackEnv class"); }
      }
    }
    {  // self-contained per-lane records (DevModelW::seg_rec, dl_pk, ...): denormalised copies of the tables loaded above
      auto BI = [&](const char* n) { std::vector<int> v; const BlobRec* r = blob_find(blob, n); if (r && r->dtype == 1) { v.resize(r->nbytes / 4); memcpy(v.data(), blob + r->offset, r->nbytes); } return v; };
      auto BF = [&](const char* n) { std::vector<float> v; const BlobRec* r = blob_find(blob, n); if (r && r->dtype == 0) { v.resize(r->nbytes / 8); const double* sp = (const double*)(blob + r->offset); for (size_t i = 0; i < v.size(); i++) v[i] = (float)sp[i]; } return v; };
      const std::vector<int> seg = BI("hip_seg"), seg_order = BI("hip_seg_order"), seg_tendon = BI("hip_seg_tendon"), site_link = BI("hip_site_link"), wg_link = BI("hip_wg_link"),
                             dl = BI("hip_dl"), dof_type = BI("hip_dof_type");
      const std::vector<float> seg_div = BF("hip_seg_div"), site_lpos = BF("hip_site_lpos"), wg_lpos = BF("hip_wg_lpos"), wg_lmat = BF("hip_wg_lmat"), wg_radius = BF("hip_wg_radius");
      auto fi = [](int v) { float f; memcpy(&f, &v, 4); return f; };
      std::vector<int> dlp(std::max<size_t>(dl.size() / 3, 1), 0);
      for (size_t i = 0; i < dl.size() / 3; i++) {
        const int dd = dl[3 * i], sg = dl[3 * i + 1], slot = dl[3 * i + 2];
        if (dd < 0 || dd > 127 || slot < 0 || slot > 255 || sg < -32768 || sg > 32767) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "moment-arm list entry does not fit the packed word"); }
        dlp[i] = dd | ((dof_type[dd] == 3 ? 1 : 0) << 7) | (slot << 8) | (int)((unsigned)sg << 16);
      }
      // (each segment's three lists are copied to 16-byte rows of their own: a lane reads a list four entries per load, the first row ahead of its use)
      std::vector<int> dl4;
      std::vector<float> rec((size_t)std::max(d.nseg, 1) * SEGR * 4, 0.f);
      for (int idx = 0; idx < d.nseg; idx++) {
        const int si = seg_order[idx];
        const int* S = &seg[12 * (size_t)si];
        float* R = &rec[(size_t)idx * SEGR * 4];
        for (int k = 0; k < 2; k++) { R[4 * k] = fi(site_link[S[k]]); for (int c = 0; c < 3; c++) R[4 * k + 1 + c] = site_lpos[3 * (size_t)S[k] + c]; }
        R[8] = fi(S[2]); R[9] = fi(S[3] >= 0 ? site_link[S[3]] : -2); R[10] = 1.0f / seg_div[si]; R[11] = fi(seg_tendon[si]);
        for (int k = 0; k < 3; k++) {
          const int a0 = S[4 + 2 * k], n = S[5 + 2 * k], adr4 = (int)(dl4.size() / 4);
          if (adr4 >= (1 << 20) || n < 0 || n >= (1 << 11) || (n > 0 && (a0 < 0 || (size_t)(a0 + n) > dl.size() / 3))) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "tendon moment-arm lists too long for the packed segment record"); }
          for (int i = 0; i < n; i++) dl4.push_back(dlp[a0 + i]);
          while (dl4.size() % 4 || dl4.size() == (size_t)adr4 * 4) dl4.push_back(0);     // whole rows; an empty list still owns one (the lane loads it unconditionally)
          R[12 + k] = fi(adr4 | (n << 20));
        }
        R[15] = fi(S[10]);
        if (S[2] >= 0) {
          const int g = S[2];
          if (S[3] >= 0) for (int c = 0; c < 3; c++) R[16 + c] = site_lpos[3 * (size_t)S[3] + c];
          R[19] = wg_radius[g];
          R[20] = fi(wg_link[g]); for (int c = 0; c < 3; c++) R[21 + c] = wg_lpos[3 * (size_t)g + c];
          for (int c = 0; c < 9; c++) R[24 + c] = wg_lmat[9 * (size_t)g + c];
        }
      }
      const float* tf4 = nullptr; const int* ti4 = nullptr;
      if (dl4.empty()) dl4.resize(4, 0);
      if ((rc = upload<float>(m, rec, &tf4)) || (rc = upload<int>(m, dl4, &ti4))) { myo_model_free(m); return rc; }
      w.seg_rec = (decltype(w.seg_rec))tf4; w.dl_pk = (decltype(w.dl_pk))ti4;
      // collision geoms, pairs and the pairs' dof lists
      const std::vector<int> cg_link = BI("hip_cg_link"), cg_type = BI("hip_cg_type"), pair_i = BI("hip_pair_i"), pair_dl = BI("hip_pair_dl");
      const std::vector<float> cg_lpos = BF("hip_cg_lpos"), cg_lmat = BF("hip_cg_lmat"), cg_size = BF("hip_cg_size"), cg_rb = BF("hip_cg_rbound"), pair_f = BF("hip_pair_f");
      std::vector<float> grec((size_t)std::max(d.ncg, 1) * 16, 0.f), prec((size_t)std::max(d.npair, 1) * 16, 0.f);
      for (int g = 0; g < d.ncg; g++) {
        float* R = &grec[(size_t)g * 16];
        R[0] = fi(cg_link[g]); for (int c = 0; c < 3; c++) R[1 + c] = cg_lpos[3 * (size_t)g + c];
        for (int c = 0; c < 9; c++) R[4 + c] = cg_lmat[9 * (size_t)g + c];
        R[13] = fi(cg_type[g]); R[14] = cg_rb[g];
      }
      for (int q = 0; q < d.npair; q++) {
        const int* P = &pair_i[6 * (size_t)q];
        const float* F = &pair_f[12 * (size_t)q];
        if (P[0] > 255 || P[1] > 255 || P[3] > 255 || P[4] > 15 || P[5] > 15) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "collision pair does not fit the packed pair record"); }
        float* R = &prec[(size_t)q * 16];
        R[0] = fi(P[0] | (P[1] << 8) | (P[4] << 16) | (P[5] << 20) | (P[3] << 24)); R[1] = F[0]; R[2] = F[1]; R[3] = fi(P[2]);
        for (int c = 0; c < 3; c++) { R[4 + c] = cg_size[3 * (size_t)P[0] + c]; R[8 + c] = cg_size[3 * (size_t)P[1] + c]; }
        R[7] = cg_rb[P[0]]; R[11] = cg_rb[P[1]];
        R[12] = fi(cg_type[P[0]] | (cg_type[P[1]] << 8));
      }
      // (a contact carries pair | dofs << 11 | dof-list start << 16 in one word: step kernel, narrow phase -> row stage)
      if (d.npair > 2048 || pair_dl.size() / 2 >= (1u << 16) || d.maxkc > 31) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "more than 2048 collision pairs, 65535 contact dof-list entries or 31 dofs per contact"); }
      std::vector<int> pdl(std::max<size_t>(pair_dl.size() / 2, 1), 0);
      for (size_t i = 0; i < pair_dl.size() / 2; i++) {
        const int dd = pair_dl[2 * i], sg = pair_dl[2 * i + 1];
        if (dd < 0 || dd > 127 || sg < -(1 << 22) || sg > (1 << 22)) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "contact dof-list entry does not fit the packed word"); }
        pdl[i] = dd | ((dof_type[dd] == 3 ? 1 : 0) << 7) | (int)((unsigned)sg << 8);
      }
      const float *tg4 = nullptr, *tp4 = nullptr; const int* tq4 = nullptr;
      if ((rc = upload<float>(m, grec, &tg4)) || (rc = upload<float>(m, prec, &tp4)) || (rc = upload<int>(m, pdl, &tq4))) { myo_model_free(m); return rc; }
      w.cg_rec = (decltype(w.cg_rec))tg4; w.pair_rec = (decltype(w.pair_rec))tp4; w.pair_dl_pk = (decltype(w.pair_dl_pk))tq4;
      // tree words: one packed word per lane and round for the sweeps over the kinematic tree (DevModelW::kin_pk, link_desc, link_adof, dof_anc)
      {
        const std::vector<int> lpar = BI("hip_link_parent"), dlink = BI("hip_dof_link"), dpar = BI("dof_parentid"), kadr = BI("hip_kin_adr"), kvec = BI("hip_kin_vec"),
                               chadr = BI("hip_link_chain_adr"), chain = BI("hip_link_chain");
        if (d.nl > 64 || d.nv > 64) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "more than 64 links or dofs"); }
        std::vector<int> kpk;
        for (size_t L = 0; L + 1 < kadr.size(); L++) {
          for (int e0 = kadr[L]; e0 < kadr[L + 1]; e0 += 64) {
            for (int i = 0; i < 64; i++) {
              const int e = e0 + i;
              if (e >= kadr[L + 1]) { kpk.push_back(-1); continue; }
              const int w0 = kvec[2 * (size_t)e], src = kvec[2 * (size_t)e + 1], l = w0 & 255, kind = (w0 >> 8) & 3, ix = w0 >> 16, par1 = lpar[l] + 1;
              if (src < 0 || src >= 2048 || l >= 64 || ix < 0 || ix >= 64 || par1 < 0 || par1 > 64) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "kinematics entry does not fit the packed word"); }
              kpk.push_back((int)((unsigned)src | ((unsigned)l << 11) | ((unsigned)kind << 17) | ((unsigned)ix << 19) | ((unsigned)par1 << 25)));
            }
          }
        }
        w.kin_nround = (int)(kpk.size() / 64);
        kpk.resize(kpk.size() + 64, -1);                       // padding round: the loop prefetches one round ahead
        std::vector<unsigned long long> desc(d.nl, 0), adof(d.nl, 0), anc(d.nv, 0);
        for (int l = d.nl - 1; l >= 0; l--) { desc[l] |= 1ull << l; if (lpar[l] >= 0) { if (lpar[l] >= l) { myo_model_free(m); return fail(MYO_E_BLOB, "links are not in tree order"); } desc[lpar[l]] |= desc[l]; } }
        for (int q = 0; q < d.nv; q++) { if (dpar[q] >= q) { myo_model_free(m); return fail(MYO_E_BLOB, "dofs are not in tree order"); } anc[q] = (1ull << q) | (dpar[q] >= 0 ? anc[dpar[q]] : 0ull); }
        unsigned long long frot = 0, fj3 = 0;
        for (int l = 0; l < d.nl; l++) {
          int prev = -1;
          for (int c = chadr[l]; c < chadr[l + 1]; c++) {
            const int e = chain[c], q = e & 255, j = (e >> 8) & 7, fr = e >> 12;
            if (q <= prev || q >= d.nv) { myo_model_free(m); return fail(MYO_E_BLOB, "link dof chain is not root-first"); }
            prev = q;
            adof[l] |= 1ull << q;
            if (fr && j >= 3) frot |= 1ull << q;
            if (fr && j == 3) fj3 |= 1ull << q;
          }
        }
        w.free_rot[0] = (unsigned)frot; w.free_rot[1] = (unsigned)(frot >> 32); w.free_j3[0] = (unsigned)fj3; w.free_j3[1] = (unsigned)(fj3 >> 32);
        auto split = [](const std::vector<unsigned long long>& v) { std::vector<int> o(std::max<size_t>(2 * v.size(), 2), 0); for (size_t i = 0; i < v.size(); i++) { o[2 * i] = (int)(unsigned)v[i]; o[2 * i + 1] = (int)(unsigned)(v[i] >> 32); } return o; };
        const int *t0 = nullptr, *t1 = nullptr, *t2 = nullptr, *t3 = nullptr;
        if ((rc = upload<int>(m, kpk, &t0)) || (rc = upload<int>(m, split(desc), &t1)) || (rc = upload<int>(m, split(adof), &t2)) || (rc = upload<int>(m, split(anc), &t3))) { myo_model_free(m); return rc; }
        w.kin_pk = (decltype(w.kin_pk))t0; w.link_desc = (decltype(w.link_desc))t1; w.link_adof = (decltype(w.link_adof))t2; w.dof_anc = (decltype(w.dof_anc))t3;
      }
    }
    const bool common = d.nl <= 64 && d.ncg <= (m->trk ? 128 : 64) && w.nq <= 64 && w.neq <= 64 && d.maxnnz <= 20;   // (geom ids are bytes in the pair record; the TRK kernel loops over geoms)
    const bool needs_full = w.has_free || w.neq > 0 || plane_pairs || condim1 || m->trk;
    if (m->trk) {
      if (!(common && d.nv <= 36 && d.nu <= 128 && d.ngt <= 128 && d.maxkc <= 20 && !w.hf.on && !w.has_tl)) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "condim-4 / friction-loss / box / mesh model exceeds the limits of the TRK step kernel"); }
      m->wave_ok = true; m->wave_cfg = 2; m->generic_ok = false;
      build_layout_w(d, w, 36, 20, 32, 4);
    }
    else if (common && !needs_full && d.nv <= 24 && d.nu <= 64 && d.ngt <= 64 && d.maxkc <= 8) {
      m->wave_ok = true; m->wave_cfg = 0;
      build_layout_w(d, w, 24, 8, 32);
    }
    else if (common && d.nv <= 36 && d.nu <= 128 && d.ngt <= 128 && d.maxkc <= 20) { m->wave_ok = true; m->wave_cfg = 1; build_layout_w(d, w, 36, 20, 32); }
    else { m->wave_ok = false; build_layout_w(d, w, 24, 8, 32); }
    m->hand_sizes = m->wave_ok && m->wave_cfg == 0 && sizes_match<1>(w.nq, d.nv, d.nu, d.nl, d.nlevel, d.maxnnz, d.ngt, d.nseg, d.ncg, d.npair);
    if (m->trk) m->generic_ok = false;
    if (blob_find(blob, "integrator")) { std::vector<int> ig; if ((rc = load_i(m, blob, "integrator", &tmpi, &ig))) { myo_model_free(m); return rc; } m->rk4 = !ig.empty() && ig[0] == 1; }
    if (m->rk4) {
      if (!m->wave_ok || m->trk || w.hf.on) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "RK4: wave kernel models without height field / TrackEnv features only"); }
      m->generic_ok = false;
    }
    m->leg_sizes = m->wave_ok && m->wave_cfg == 1 && sizes_match<2>(w.nq, d.nv, d.nu, d.nl, d.nlevel, d.maxnnz, d.ngt, d.nseg, d.ncg, d.npair);
    m->terrain_sizes = m->wave_ok && m->wave_cfg == 1 && w.hf.on && sizes_match<3>(w.nq, d.nv, d.nu, d.nl, d.nlevel, d.maxnnz, d.ngt, d.nseg, d.ncg, d.npair);
    {  // the specialised instantiations also build in the dof tree (tree-sparse factorisation): it must be the model's
      std::vector<int> dpar;
      if ((rc = load_i(m, blob, "dof_parentid", &tmpi, &dpar))) { myo_model_free(m); return rc; }
      auto same_tree = [&](const int* ref, int n) { if ((int)dpar.size() != n) return false; for (int i = 0; i < n; i++) if (dpar[i] != ref[i]) return false; return true; };
      if (m->hand_sizes && !same_tree(SpecTree<1>::parent, SpecTree<1>::nv)) m->hand_sizes = false;
      if ((m->leg_sizes || m->terrain_sizes) && !same_tree(SpecTree<2>::parent, SpecTree<2>::nv)) m->leg_sizes = m->terrain_sizes = false;
    }
    if (m->rk4) m->hand_sizes = m->leg_sizes = m->terrain_sizes = false;
    if (w.has_tl) m->hand_sizes = m->leg_sizes = m->terrain_sizes = false;   // the specialised instantiations compile the tendon-limit rows out
    // ... and their LDS layout in: it must be the one this model was given
    if (m->hand_sizes && !layout_match<1, 24, 8, 32, 3>(w.lay)) m->hand_sizes = false;
    if (m->leg_sizes && !layout_match<2, 36, 20, 32, 3>(w.lay)) m->leg_sizes = false;
    if (m->terrain_sizes && !layout_match<3, 36, 20, 32, 3>(w.lay)) m->terrain_sizes = false;
    if (const char* e = getenv("MYO_NO_SPEC")) if (atoi(e) == 1) m->hand_sizes = m->leg_sizes = m->terrain_sizes = false;   // tests: force the run-time-sized instantiations
    if (!m->wave_ok && !m->generic_ok) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "model exceeds the limits of both step kernels (nv <= 36, nu <= 128, pair dofs <= 20)"); }
    { const int nvt = m->wave_cfg == 0 ? 24 : 36;
      if (m->wave_ok && m->kin_floats > nvt * (nvt + 1)) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "kinematics scratch exceeds the Hessian scratch it borrows"); } }
    m->env_lds_bytes_w = w.lay.total * 4;
    if (m->wave_ok && m->env_lds_bytes_w > 64 * 1024) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "wave kernel working set exceeds 64 KB of LDS"); }
    void* p1 = nullptr; void* p2 = nullptr;
    if (hipMalloc(&p1, sizeof(DevModel)) != hipSuccess || hipMalloc(&p2, sizeof(DevModelW)) != hipSuccess) { myo_model_free(m); return fail(MYO_E_NOMEM, "hipMalloc model structs"); }
    m->dev_allocs.push_back(p1); m->dev_allocs.push_back(p2);
    m->d_dm = (DevModel*)p1; m->d_dw = (DevModelW*)p2;
    if (hipMemcpy(p1, &d, sizeof(DevModel), hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(p2, &w, sizeof(DevModelW), hipMemcpyHostToDevice) != hipSuccess) { myo_model_free(m); return fail(MYO_E_HIP, "upload model structs"); }
  }
  m->dims = myo_dims{S[0], S[1], S[2], d.na_obs, S[4], S[8], S[7], d.nl, 0, m->wave_ok ? m->env_lds_bytes_w : m->env_lds_bytes, 64,
                     m->wave_ok ? (m->wave_cfg >= 1 ? 32 : NCONW) : NCON, d.timestep};
  if (4 * m->env_lds_bytes > 160 * 1024) {
    if (!m->wave_ok) { myo_model_free(m); return fail(MYO_E_UNSUPPORTED, "model working set exceeds 160 KB of LDS per workgroup"); }
    m->generic_ok = false;
  }
  if (m->wave_ok && !m->body_link.empty()) {   // member tables of the per-env body-mass override (lowering.py's link recomposition, per body)
    auto f64 = [&](const char* n) { std::vector<double> v; const BlobRec* r = blob_find(blob, n); if (r && r->dtype == 0) { v.resize(r->nbytes / 8); memcpy(v.data(), blob + r->offset, r->nbytes); } return v; };
    const std::vector<double> bmass = f64("body_mass"), ipos = f64("body_ipos"), iquat = f64("body_iquat"), inert = f64("body_inertia"),
                              lpos = f64("hip_body_lpos"), lquat = f64("hip_body_lquat");
    const int nb = (int)m->body_link.size();
    if ((int)bmass.size() == nb && (int)ipos.size() == 3 * nb && (int)iquat.size() == 4 * nb && (int)inert.size() == 3 * nb &&
        (int)lpos.size() == 3 * nb && (int)lquat.size() == 4 * nb) {
      auto qmat = [](const double* q, double* R) {
        const double w = q[0], x = q[1], y = q[2], z = q[3];
        R[0] = w * w + x * x - y * y - z * z; R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
        R[3] = 2 * (x * y + w * z); R[4] = w * w - x * x + y * y - z * z; R[5] = 2 * (y * z - w * x);
        R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = w * w - x * x - y * y + z * z;
      };
      std::vector<int> adr(d.nl + 1, 0), body;
      std::vector<double> tab;
      for (int l = 0; l < d.nl; l++) {
        adr[l] = (int)body.size();
        for (int b = 1; b < nb; b++) {
          if (m->body_link[b] != l) continue;
          double Rl[9], Rq[9], Ri[9], c[3], I[9];
          qmat(&lquat[4 * b], Rl); qmat(&iquat[4 * b], Rq);
          for (int i = 0; i < 3; i++) {
            c[i] = lpos[3 * b + i];
            for (int j = 0; j < 3; j++) { c[i] += Rl[3 * i + j] * ipos[3 * b + j]; Ri[3 * i + j] = Rl[3 * i] * Rq[j] + Rl[3 * i + 1] * Rq[3 + j] + Rl[3 * i + 2] * Rq[6 + j]; }
          }
          for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) I[3 * i + j] = Ri[3 * i] * inert[3 * b] * Ri[3 * j] + Ri[3 * i + 1] * inert[3 * b + 1] * Ri[3 * j + 1] + Ri[3 * i + 2] * inert[3 * b + 2] * Ri[3 * j + 2];
          body.push_back(b);
          for (double v : {c[0], c[1], c[2], I[0], I[4], I[8], I[1], I[2], I[5], bmass[b]}) tab.push_back(v);
        }
      }
      adr[d.nl] = (int)body.size();
      int rc2;
      if ((rc2 = upload<int>(m, adr, &m->d_lm_adr)) || (rc2 = upload<int>(m, body, &m->d_lm_body)) || (rc2 = upload<double>(m, tab, &m->d_lm_tab))) { myo_model_free(m); return rc2; }
      m->body_mass0.assign(bmass.begin(), bmass.end());
    }
  }
  *out = m;
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
static void quat2mat_d(double* R, const double* q);

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
  if (c->task == MYO_TASK_POSE) { if (c->ntarget != nv) return fail(MYO_E_ARG, "pose task: ntarget must equal nq"); T.obs_dim = 3 * nv + b->model->dm.na_obs; }
  else if (c->task == MYO_TASK_REACH) { if (c->ntarget != 3 * c->ntip) return fail(MYO_E_ARG, "reach task: ntarget must be 3*ntip"); T.obs_dim = 2 * nv + 6 * c->ntip + b->model->dm.na_obs; }
  else if (c->task == MYO_TASK_STAND) {
    if (c->ntarget != 3) return fail(MYO_E_ARG, "stand task: ntarget must be 3 (target position)");
    if (!(b->model->wave_ok && b->model->dw.has_free && b->model->nq == nv + 1)) return fail(MYO_E_UNSUPPORTED, "stand task needs a model with a free root joint");
    T.obs_dim = b->model->nq + nv + 6 + b->model->dm.na_obs;
  }
  else if (c->task == MYO_TASK_KEYTURN) {
    // key_turn_v0.py: the key is the model's last joint, one hinge of a root body; sites = key head, index tip, thumb tip
    const myo_model* m = b->model;
    if (!(m->wave_ok && m->trk) || m->bp_link < 0 || m->nq != nv) return fail(MYO_E_UNSUPPORTED, "key-turn task: a TrackEnv-class model without free / ball joints whose last joint is the hinge of a root body");
    std::vector<int> ltype(1), ldn(1), ldof(1);
    HIPCHK(hipMemcpy(ltype.data(), dm.dof_type + (nv - 1), 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ldn.data(), dm.link_dofnum + m->bp_link, 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ldof.data(), dm.dof_link + (nv - 1), 4, hipMemcpyDeviceToHost));
    if (ltype[0] != 3 || ldn[0] != 1 || ldof[0] != m->bp_link) return fail(MYO_E_UNSUPPORTED, "key-turn task: the last joint must be the one hinge of its root body");
    if (c->ntip != 3 || c->ntarget != 0) return fail(MYO_E_ARG, "key-turn task: ntip = 3 (key head, index tip, thumb tip) and ntarget = 0");
    for (int k = 0; k < 3; k++) if (c->tip_site[k] < 0 || c->tip_site[k] >= m->dims.nsite) return fail(MYO_E_ARG, "key-turn task: site id out of range");
    if (!(c->near_th >= 0.f) || !(c->far_th > 0.f) || !(c->pose_thd == c->pose_thd)) return fail(MYO_E_ARG, "key-turn task: near_th >= 0, far_th > 0, goal_th (pose_thd) a number");
    T.obs_dim = 2 * nv + 6 + dm.na_obs;
  }
  else if (c->task == MYO_TASK_PEN) {
    // pen_v0.py: the pen is the model's last six joints, 3 slides + 3 hinges of one root body; sites = object top / bottom, target top /
    // bottom, eps_ball
    const myo_model* m = b->model;
    if (!(m->wave_ok && m->trk) || m->nq != nv || nv < 7) return fail(MYO_E_UNSUPPORTED, "pen task: a TrackEnv-class model without free / ball joints whose last six joints are the pen's");
    std::vector<int> dtype(6), dlink(6), lpar(1), ldn(1);
    HIPCHK(hipMemcpy(dtype.data(), dm.dof_type + (nv - 6), 24, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(dlink.data(), dm.dof_link + (nv - 6), 24, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(lpar.data(), dm.link_parent + dlink[5], 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ldn.data(), dm.link_dofnum + dlink[5], 4, hipMemcpyDeviceToHost));
    bool ok = lpar[0] < 0 && ldn[0] == 6;
    for (int k = 0; k < 6; k++) ok = ok && dlink[k] == dlink[5] && dtype[k] == (k < 3 ? 2 : 3);
    if (!ok) return fail(MYO_E_UNSUPPORTED, "pen task: the last six joints must be 3 slides + 3 hinges of one root body");
    if (c->ntip != 5 || c->ntarget != 0) return fail(MYO_E_ARG, "pen task: ntip = 5 (object top, object bottom, target top, target bottom, eps_ball) and ntarget = 0");
    for (int k = 0; k < 5; k++) if (c->tip_site[k] < 0 || c->tip_site[k] >= m->dims.nsite) return fail(MYO_E_ARG, "pen task: site id out of range");
    for (int k = 0; k < 3; k++) if (!std::isfinite(c->tip_lpos[k])) return fail(MYO_E_ARG, "pen task: tip_lpos must be finite");
    if (!(c->far_th > 0.f) || !(c->pose_thd == c->pose_thd)) return fail(MYO_E_ARG, "pen task: far_th > 0, pose_thd a number");
    T.obs_dim = (nv - 6) + 21 + dm.na_obs;
  }
  else if (c->task == MYO_TASK_BAODING) {
    // baoding_v1.py: the balls are the model's last two joints, free joints of root bodies (qpos[-14:-7], qpos[-7:]); sites = ball1, ball2,
    // target1, target2.  The targets move in the frame of their body (baoding_v1.py:147-181: site_pos), which lowering folds into its link:
    // T.bd_frame carries that body's x and y axes and, per target, the body origin lifted by the site's compiled z, in the link frame
    const myo_model* m = b->model;
    if (!(m->wave_ok && m->trk) || m->nq != nv + 2 || nv < 13) return fail(MYO_E_UNSUPPORTED, "baoding task: a TrackEnv-class model whose last two joints are free joints (the balls)");
    std::vector<int> dlink(12), lpar(2), ldn(2);
    HIPCHK(hipMemcpy(dlink.data(), dm.dof_link + (nv - 12), 48, hipMemcpyDeviceToHost));
    for (int k = 0; k < 2; k++) {
      HIPCHK(hipMemcpy(lpar.data() + k, dm.link_parent + dlink[6 * k], 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(ldn.data() + k, dm.link_dofnum + dlink[6 * k], 4, hipMemcpyDeviceToHost));
    }
    bool ok = dlink[0] != dlink[6] && lpar[0] < 0 && lpar[1] < 0 && ldn[0] == 6 && ldn[1] == 6;
    for (int k = 0; k < 12; k++) ok = ok && dlink[k] == dlink[k < 6 ? 0 : 6];
    if (!ok) return fail(MYO_E_UNSUPPORTED, "baoding task: the last twelve dofs must be two free joints of root bodies");
    if (c->ntip != 4 || c->ntarget != 5) return fail(MYO_E_ARG, "baoding task: ntip = 4 (ball1, ball2, target1, target2) and ntarget = 5 (goal parameters)");
    for (int k = 0; k < 4; k++) if (c->tip_site[k] < 0 || c->tip_site[k] >= m->dims.nsite) return fail(MYO_E_ARG, "baoding task: site id out of range");
    std::vector<int> slink(4);
    for (int k = 0; k < 4; k++) HIPCHK(hipMemcpy(slink.data() + k, dm.site_link + c->tip_site[k], 4, hipMemcpyDeviceToHost));
    const int tb = m->site_body[c->tip_site[2]];
    if (slink[0] != dlink[0] || slink[1] != dlink[6] || tb != m->site_body[c->tip_site[3]] || slink[2] < 0 || m->body_link[tb] != slink[2])
      return fail(MYO_E_UNSUPPORTED, "baoding task: the ball sites must be on the balls, both target sites on one moving body");
    if (!(c->far_th == c->far_th) || !(c->pose_thd == c->pose_thd)) return fail(MYO_E_ARG, "baoding task: far_th (drop_th) and pose_thd (proximity_th) numbers");
    const float* bq = &m->body_lquat[4 * (size_t)tb];
    const double qd[4] = {bq[0], bq[1], bq[2], bq[3]};
    double R[9];
    quat2mat_d(R, qd);
    for (int k = 0; k < 3; k++) { T.bd_frame[k] = (float)R[3 * k]; T.bd_frame[3 + k] = (float)R[3 * k + 1]; }
    for (int t = 0; t < 2; t++) {
      const double z = m->site_pos0[3 * (size_t)c->tip_site[2 + t] + 2];
      for (int k = 0; k < 3; k++) T.bd_frame[6 + 3 * t + k] = (float)(m->body_lpos[3 * (size_t)tb + k] + R[3 * k + 2] * z);
    }
    T.obs_dim = (nv - 12) + 24;
  }
  else if (c->task == MYO_TASK_HOLD) {
    if (c->ntarget != 3) return fail(MYO_E_ARG, "hold task: ntarget must be 3 (goal position)");
    if (!(b->model->wave_ok && b->model->dw.has_free && b->model->nq == nv + 1 && nv > 6)) return fail(MYO_E_UNSUPPORTED, "hold task needs a model whose last joint is one free object");
    T.obs_dim = (b->model->nq - 7) + (nv - 6) + 6 + b->model->dm.na_obs;
  }
  else T.obs_dim = 0;
  T.nq = b->model->nq;
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

static void quat2mat_d(double* R, const double* q) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = w * w + x * x - y * y - z * z; R[1] = 2 * (x * y - w * z); R[2] = 2 * (x * z + w * y);
  R[3] = 2 * (x * y + w * z); R[4] = w * w - x * x + y * y - z * z; R[5] = 2 * (y * z - w * x);
  R[6] = 2 * (x * z - w * y); R[7] = 2 * (y * z + w * x); R[8] = w * w - x * x - y * y + z * z;
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

int myo_reset(myo_batch* b, const uint8_t* mask_dev, uint64_t seed, void* stream) {
  if (!b) return fail(MYO_E_ARG, "myo_reset: null");
  b->reset_seed = seed;
  const DevModel& dm = b->model->dm;
  HIPCHK(hipSetDevice(b->model->device));
  int B = b->db.B;
  hipLaunchKernelGGL(reset_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, b->db, b->task, b->model->nq, dm.nv, dm.nu, dm.qpos0, mask_dev, seed,
                     b->env_offset, 0);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

int myo_autoreset(myo_batch* b, int max_episode_steps, uint64_t seed, void* stream) {
  if (!b || max_episode_steps <= 0) return fail(MYO_E_ARG, "myo_autoreset: bad arguments");
  b->reset_seed = seed;
  const DevModel& dm = b->model->dm;
  HIPCHK(hipSetDevice(b->model->device));
  int B = b->db.B;
  hipLaunchKernelGGL(reset_kernel, dim3(B), dim3(64), 0, (hipStream_t)stream, b->db, b->task, b->model->nq, dm.nv, dm.nu, dm.qpos0,
                     (const uint8_t*)nullptr, seed, b->env_offset, max_episode_steps);
  HIPCHK(hipGetLastError());
  return MYO_OK;
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
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel<32>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)reach_obs_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
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
  const bool bm = b->bm_on;
  if (bm) {
    int rc = bm_check(b);
    if (rc) return rc;
    const int n = b->db.B * m->dm.nl;
    hipLaunchKernelGGL(link_compose_kernel, dim3((n + 255) / 256), dim3(256), 0, s, b->db, m->dm.nl, m->d_lm_adr, m->d_lm_body, m->d_lm_tab);
  }
  const bool hand_sizes = m->hand_sizes && !bm, leg_sizes = m->leg_sizes && !bm;
  if (G == 64 && m->wave_ok) {
    // kernel attributes are per device: one flag per device ordinal (a process that opens models on two GPUs)
    static std::mutex attr_mu;
    static bool attr_w_dev[64] = {};
    std::lock_guard<std::mutex> attr_lock(attr_mu);
    bool& attr_w = attr_w_dev[m->device & 63];
    if (!attr_w) {
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel_w<24, 8, 32, 1, 3, false, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel_w<24, 8, 32, 1, 4, false, 1>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel_w<36, 20, 32, 2, 2, false, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel_w<36, 20, 32, 2, 2, true, 0>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel_w<36, 20, 32, 2, 2, true, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel_w<36, 20, 32, 2, 2, false, 2>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel_w<36, 20, 32, 2, 2, false, 0, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel_w<36, 20, 32, 2, 2, true, 3, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel_w<36, 20, 32, 2, 2, false, 3, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel_w<36, 20, 32, 2, 2, false, 0, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel_w<24, 8, 32, 1, 3, false, 0, false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
      HIPCHK(hipFuncSetAttribute((const void*)step_kernel_w<36, 20, 32, 2, 2, false, 0, false, false, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024));
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
    if (!kflags)   // instantiation chosen below, as rocprofv3 prints it (bench.py reports it next to the kernel time)
      b->last_kernel = m->rk4 ? (m->wave_cfg == 0 ? "step_kernel_w<24,8,32,1,3,false,0,false,false,true>" : "step_kernel_w<36,20,32,2,2,false,0,false,false,true>") :
                       m->wave_cfg == 2 ? "step_kernel_w<36,20,32,2,2,false,0,false,true>" :
                       sched ? (m->dw.hf.on ? "step_kernel_w<36,20,32,2,2,true,3,true>" : (leg_sizes ? "step_kernel_w<36,20,32,2,2,true,2,false>" : "step_kernel_w<36,20,32,2,2,true,0,false>"))
                             : (m->wave_cfg == 0 ? (hand_sizes ? "step_kernel_w<24,8,32,1,4,false,1,false>" : "step_kernel_w<24,8,32,1,3,false,0,false>")
                                                 : (m->dw.hf.on ? (m->terrain_sizes ? "step_kernel_w<36,20,32,2,2,false,3,true>" : "step_kernel_w<36,20,32,2,2,false,0,true>") : (leg_sizes ? "step_kernel_w<36,20,32,2,2,false,2,false>" : "step_kernel_w<36,20,32,2,2,false,0,false>")));
    if (sched) {
      hipLaunchKernelGGL(sched_init_kernel, dim3(1), dim3(1024), 0, s, (const int*)b->db.diag, Bn, S);
      int grid = Bn < resident ? Bn : resident;    // persistent waves: no more workgroups than the chip holds at once
      static const int grid_override = [] { const char* e = getenv("MYO_SCHED_GRID"); return e ? atoi(e) : 0; }();
      if (grid_override > 0 && grid_override < grid) grid = grid_override;
      if (m->dw.hf.on)
        hipLaunchKernelGGL((step_kernel_w<36, 20, 32, 2, 2, true, 3, true>), dim3(grid), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm,
                           (const DevModelW*)m->d_dw, b->db, action, actmap, nsub, st, (const int*)nullptr, wk, 0, S);
      else if (leg_sizes)
        hipLaunchKernelGGL((step_kernel_w<36, 20, 32, 2, 2, true, 2>), dim3(grid), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm,
                           (const DevModelW*)m->d_dw, b->db, action, actmap, nsub, st, (const int*)nullptr, wk, 0, S);
      else
        hipLaunchKernelGGL((step_kernel_w<36, 20, 32, 2, 2, true, 0>), dim3(grid), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm,
                           (const DevModelW*)m->d_dw, b->db, action, actmap, nsub, st, (const int*)nullptr, wk, 0, S);
    } else if (m->rk4 && m->wave_cfg == 0)
      hipLaunchKernelGGL((step_kernel_w<24, 8, 32, 1, 3, false, 0, false, false, true>), dim3(Bn), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm,
                         (const DevModelW*)m->d_dw, b->db, action, actmap, nsub, st, order, (const DevWalk*)nullptr, 0, S);
    else if (m->rk4)
      hipLaunchKernelGGL((step_kernel_w<36, 20, 32, 2, 2, false, 0, false, false, true>), dim3(Bn), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm,
                         (const DevModelW*)m->d_dw, b->db, action, actmap, nsub, st, order, wk, kflags, S);
    else if (m->wave_cfg == 2)   // TrackEnv model class
      hipLaunchKernelGGL((step_kernel_w<36, 20, 32, 2, 2, false, 0, false, true>), dim3(Bn), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm,
                         (const DevModelW*)m->d_dw, b->db, action, actmap, nsub, st, order, wk, kflags, S);
    else if (m->wave_cfg == 0 && hand_sizes)
      hipLaunchKernelGGL((step_kernel_w<24, 8, 32, 1, 4, false, 1>), dim3(Bn), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm,
                         (const DevModelW*)m->d_dw, b->db, action, actmap, nsub, st, order, (const DevWalk*)nullptr, 0, S);
    else if (m->wave_cfg == 0)
      hipLaunchKernelGGL((step_kernel_w<24, 8, 32, 1, 3, false, 0>), dim3(Bn), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm,
                         (const DevModelW*)m->d_dw, b->db, action, actmap, nsub, st, order, (const DevWalk*)nullptr, 0, S);
    else if (m->dw.hf.on && m->terrain_sizes)     // terrain models: the instantiations with the height-field narrow phase
      hipLaunchKernelGGL((step_kernel_w<36, 20, 32, 2, 2, false, 3, true>), dim3(Bn), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm,
                         (const DevModelW*)m->d_dw, b->db, action, actmap, nsub, st, order, wk, kflags, S);
    else if (m->dw.hf.on)
      hipLaunchKernelGGL((step_kernel_w<36, 20, 32, 2, 2, false, 0, true>), dim3(Bn), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm,
                         (const DevModelW*)m->d_dw, b->db, action, actmap, nsub, st, order, wk, kflags, S);
    else if (leg_sizes)
      hipLaunchKernelGGL((step_kernel_w<36, 20, 32, 2, 2, false, 2>), dim3(Bn), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm,
                         (const DevModelW*)m->d_dw, b->db, action, actmap, nsub, st, order, wk, kflags, S);
    else
      hipLaunchKernelGGL((step_kernel_w<36, 20, 32, 2, 2, false, 0>), dim3(Bn), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm,
                         (const DevModelW*)m->d_dw, b->db, action, actmap, nsub, st, order, wk, kflags, S);
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

static int launch_obs(myo_batch* b, hipStream_t s, int obs_only = 0, int reset_only = 0) {
  const myo_model* m = b->model;
  int B = b->db.B;
  if (b->task.task == MYO_TASK_WALK) {
    // the walk observation lives in the step kernel: run it with zero substeps as an observation-only pass
    return launch_step(b, nullptr, MYO_ACTMAP_NONE, 0, s, KF_AUX | (obs_only ? KF_OBS_ONLY : 0) | (reset_only ? KF_RESET_ONLY : 0));
  } else if (b->task.task == MYO_TASK_TRACK && b->track_flavour == 1) {
    hipLaunchKernelGGL(myodm_obs_kernel, dim3(B), dim3(64), 0, s, m->dm, b->db, b->task, (const DevTrack*)b->d_track, b->reset_seed, obs_only, reset_only);
  } else if (b->task.task == MYO_TASK_POSE || b->task.task == MYO_TASK_HOLD || b->task.task == MYO_TASK_STAND || b->task.task == MYO_TASK_TRACK) {
    hipLaunchKernelGGL(obs_kernel, dim3(B), dim3(64), 0, s, m->dm, b->db, b->task, obs_only, reset_only);
  } else if (b->task.task == MYO_TASK_KEYTURN) {
    hipLaunchKernelGGL(keyturn_obs_kernel, dim3(B), dim3(64), 0, s, m->dm, b->db, b->task, obs_only, reset_only);
  } else if (b->task.task == MYO_TASK_PEN) {
    hipLaunchKernelGGL(pen_obs_kernel, dim3(B), dim3(64), 0, s, m->dm, b->db, b->task, obs_only, reset_only);
  } else if (b->task.task == MYO_TASK_BAODING) {
    hipLaunchKernelGGL(baoding_obs_kernel, dim3(B), dim3(64), 0, s, m->dm, b->db, b->task, obs_only, reset_only);
  } else if (b->task.task == MYO_TASK_REACH) {
    const int EPW = 4;
    hipLaunchKernelGGL(reach_obs_kernel<16>, dim3((B + EPW - 1) / EPW), dim3(64), (size_t)EPW * m->env_lds_bytes, s, m->dm, b->db, b->task, obs_only);
  } else {
    return fail(MYO_E_ARG, "myo_obs: no task configured");
  }
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
    const int tk = b->task.task;
    if (mjx_track) continue;   // observation, reward, done and the masked reset are the step kernel's own epilogue
    if ((mode & MYO_BENCH_OBS) && (mode & MYO_BENCH_AUTORESET) && max_episode_steps > 0 && tk == MYO_TASK_TRACK) {     // ... the classic MyoDM flavour
      b->reset_seed = seed;
      hipLaunchKernelGGL(myodm_post_kernel, dim3(b->db.B), dim3(64), 0, s, b->model->dm, b->db, b->task, (const DevTrack*)b->d_track, b->model->nq,
                         b->model->dm.qpos0, seed, b->env_offset, max_episode_steps);
      HIPCHK(hipGetLastError());
      continue;
    }
    if ((mode & MYO_BENCH_OBS) && (mode & MYO_BENCH_AUTORESET) && max_episode_steps > 0 && (tk == MYO_TASK_POSE || tk == MYO_TASK_HOLD || tk == MYO_TASK_STAND)) {
      // state-only observations: observation + auto-reset + first observation of the new episodes in ONE launch (post_kernel)
      hipLaunchKernelGGL(post_kernel, dim3(b->db.B), dim3(64), 0, s, b->model->dm, b->db, b->task, b->model->nq, b->model->dm.qpos0, seed, b->env_offset, max_episode_steps);
      HIPCHK(hipGetLastError());
      continue;
    }
    if ((mode & MYO_BENCH_OBS) && (mode & MYO_BENCH_AUTORESET) && max_episode_steps > 0 && tk == MYO_TASK_KEYTURN) {   // the same for the key-turn task
      hipLaunchKernelGGL(keyturn_post_kernel, dim3(b->db.B), dim3(64), 0, s, b->model->dm, b->db, b->task, b->model->nq, b->model->dm.qpos0, seed, b->env_offset, max_episode_steps);
      HIPCHK(hipGetLastError());
      continue;
    }
    if ((mode & MYO_BENCH_OBS) && (mode & MYO_BENCH_AUTORESET) && max_episode_steps > 0 && tk == MYO_TASK_PEN) {       // ... and the pen task
      hipLaunchKernelGGL(pen_post_kernel, dim3(b->db.B), dim3(64), 0, s, b->model->dm, b->db, b->task, b->model->nq, b->model->dm.qpos0, seed, b->env_offset, max_episode_steps);
      HIPCHK(hipGetLastError());
      continue;
    }
    if ((mode & MYO_BENCH_OBS) && (mode & MYO_BENCH_AUTORESET) && max_episode_steps > 0 && tk == MYO_TASK_BAODING) {   // ... and the baoding task
      hipLaunchKernelGGL(baoding_post_kernel, dim3(b->db.B), dim3(64), 0, s, b->model->dm, b->db, b->task, b->model->nq, b->model->dm.qpos0, seed, b->env_offset, max_episode_steps);
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
