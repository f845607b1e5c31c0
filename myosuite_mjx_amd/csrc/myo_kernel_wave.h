// myo_kernel_wave.h -- wave-per-env kernel step_kernel_w (default path): its LDS layout, substep scheduler, size specialisations and the kernel body,
// a sequence of stage calls (the stages: myo_wave_motion.h, myo_wave_collision.h, myo_wave_solver.h; helpers and WaveCfg: myo_wave_util.h).
// Part of the single translation unit myo_hip.hip (included there, in this order); not a stand-alone header.
#ifndef MYO_KERNEL_WAVE_H
#define MYO_KERNEL_WAVE_H

// ================================================================================================
// WAVE-PER-ENV KERNEL (lanes_per_env = 64): one wavefront steps one environment.
//  * per-dof quantities (qacc, M rows, gradient, search direction, limit rows ...) live in the registers of lane = dof;
//    contact rows live in lane = contact; dense Cholesky / triangular solves / M*v run on registers with v_readlane
//    broadcasts -- no barriers, no LDS round trips;
//  * J^T f and J^T D J are scattered with LDS float atomics (one wave => deterministic order);
//  * tendons run lane = segment (wrapping segments first, then straight ones) instead of lane = tendon;
//  * the LDS slice is <= 10 KB so 16 envs (= 16 waves, 4 per SIMD) are resident per CU.
// ================================================================================================
#define NCONW 32
#define MPRW 14    // entries of the MPR warm-start table (pair id + normal): 224 B, the hand slice stays within 10 240 B = 16 waves per CU
static_assert(4 * MPRW <= 62, "the scheduler carries the table in a 64-word row (word 63 = entry count, word 62 = env reset in this launch)");
struct LayW {
  int qpos, qvel, act, ctrl, lpos, lmat, axis, anchor, xv, qfc, sq, mprw, X;
  int tJ, tlen, tforce;                           // region X, tendon phase
  int cdof, cinert, crb, cvel, cacc, cfrc;        // region X, dynamics phase
  int gpos, gax, cand, cdist, cpos, cnrm, cpair, cJ, cdofs;  // region X, collision + solver phase
  int Mp;                                                     // packed mass matrix, aliases gpos/gax/cand once the contact rows exist
  int tJp;                                                    // persistent sparse tendon rows (only for models with tendon limits)
  int total;
};
// The one definition of the wave kernel's LDS layout: myo_model_load runs it on the model's sizes, the size-specialised instantiations
// evaluate it at compile time on Sizes<SPEC> (every LDS address is then an immediate: round 2 read ~250 layout words per substep
// through scalar loads, each behind an s_waitcnt that also drains the LDS queue).
__host__ __device__ constexpr LayW layout_w(int nq, int nv, int nu, int nl, int ngt, int maxnnz, int ncg, bool has_tl, int nvt, int kc, int nc, int nj) {
  LayW Y{};
  int o = 0;
  Y.qpos = o; o += nq; Y.qvel = o; o += nv; Y.act = o; o += nu; Y.ctrl = o; o += nu;
  Y.lpos = o; o += 3 * nl; Y.lmat = o; o += 9 * nl; Y.axis = o; o += 3 * nv; Y.anchor = o; o += 3 * nv;
  Y.xv = o; o += nvt; Y.qfc = o; o += nvt; Y.sq = o; o += nvt * (nvt + 1); Y.mprw = o; o += 4 * MPRW;
  Y.tJp = 0;
  if (has_tl) { Y.tJp = o; o += ngt * maxnnz + 2 * ngt; }   // + tendon lengths and velocities, read again by the tendon-limit rows
  Y.X = o;
  Y.tJ = o; o += ngt * maxnnz; Y.tlen = o; o += ngt; Y.tforce = o; o += nu;
  const int endT = o;
  o = Y.X;
  Y.cdof = o; o += 6 * nv; Y.cinert = o; o += 10 * nl; Y.crb = o; o += 10 * nl; Y.cvel = o; o += 6 * nl; Y.cacc = o; o += 6 * nl; Y.cfrc = o; o += 6 * nl;
  const int endD = o;
  o = Y.X;
  Y.Mp = o;
  Y.gpos = o; o += 3 * ncg; Y.gax = o; o += 3 * ncg;
  Y.cand = o; o += NCAND;
  if (o - Y.Mp < (nvt * (nvt + 1)) / 2) o = Y.Mp + (nvt * (nvt + 1)) / 2;
  Y.cdist = o; o += nc; Y.cpos = o; o += 3 * nc; Y.cnrm = o; o += 3 * nc; Y.cpair = o; o += nc;
  Y.cJ = o; o += nc * nj * kc; Y.cdofs = o; o += nc * ((kc + 3) / 4);   // nj jacobian rows of kc entries per contact; kc dof ids per contact, one byte each
  if (o < endT) o = endT;
  if (o < endD) o = endD;
  Y.total = o;
  return Y;
}
// colliding height field (terrain models): world-fixed, axis-aligned; elevation data lives per env in DevBatch.hfield
struct HfDev { int on, nrow, ncol, cg; float size[4], pos[3]; };
struct DevModelW {
  LayW lay;
  gpi seg_order, seg_tendon, gt_dl;
  gpf link_mat0;
  int nwrapseg, ndl, has_tl;
  gpf tl;
  int nq, has_free, neq;          // free-floating root (nq = nv + 1), joint-coupling equalities
  int has_j0;                     // some actuator drives a joint directly: constant moment arms gt_j0 [ngt][maxnnz]
  gpf gt_j0;
  HfDev hf;                       // (kept last: the field offsets of the tables above feed the hot loops' scalar loads)
  gpi link_free, dof_qposadr, eq_i, link_chain_adr, link_chain;
  int kin_dnmax;                    // longest joint chain of a non-free link (uniform trip count of the phase-1 loop)
  gpi kin_base, kin_adr, kin_vec;   // two-phase kinematics (lowering.py hip_kin_*): scratch base per link, per-level lists of (link, vector) entries
  gpf eq_f;
  gpf mesh_rec, mesh_startrec, mesh_aabb;   // hull vertex graphs as float4 records (lowering.py hip_mesh_rec / hip_mesh_startrec); [nmesh][6] vertex bounding boxes
  gpf fl, mesh_vert;    // TRK models: friction-loss rows [nv][4] = loss, D, B, -; hull vertices of the mesh geoms
  // Self-contained per-lane records (built by myo_model_load from the tables above, 16-byte rows): what a lane needs for its item arrives
  // in a few independent 16-byte loads instead of a chain of index -> table -> table reads of single words (round 2: 3.1 k vector and 4.2 k
  // scalar loads per wave and env step, nearly every one with its latency exposed).
  gpf4 seg_rec;         // [nseg, in seg_order][SEGR]: site 0 (link, lpos) | site 1 | wrap geom, side link, 1 / divisor, tendon | three dof-list words,
                        //   wrap type | side lpos, radius | wrap geom link, lpos | its rotation (9)
  gpi dl_pk;            // moment-arm lists, one word per entry: dof | hinge << 7 | row slot << 8 | sign << 16; every list of a segment starts a 16-byte row of its own
  gpf4 cg_rec;          // [ncg][4]: link, lpos | rotation (9) | type, bounding radius
  gpf4 pair_rec;        // [npair][4]: g1 | g2 << 8 | narrow-phase type << 16 | condim << 20 | dofs << 24, margin, gap, dof-list start |
                        //   size 1, bounding radius 1 | size 2, bounding radius 2 | type 1 | type 2 << 8
  gpi pair_dl_pk;       // contact dof lists in one word per entry: dof | hinge << 7 | sign << 8
  // Tree words (built by myo_model_load): the sweeps over the kinematic tree take one packed word per lane and round, loaded ahead of the stage,
  // instead of walking level_adr -> child_adr -> child, link_chain_adr -> link_chain or dof_parent chains of dependent loads
  gpi kin_pk;           // phase 2 of the kinematics: [round][64] scratch offset | link << 11 | kind << 17 | ix << 19 | (parent + 1) << 25; all ones = idle lane;
  int kin_nround;       //   the rounds of a level are contiguous, one padding round closes the table (the loop prefetches a round ahead)
  gpi link_desc;        // [nl][2] links in the subtree of link l, itself included (64-bit mask, low word first)
  gpi link_adof;        // [nl][2] dofs on the path root -> link l, its own included
  gpi dof_anc;          // [nv][2] dof d and its ancestors
  unsigned int free_rot[2], free_j3[2];   // dofs that are rotations of a free joint / the first rotation of one
  // touch sensors (lowering.py hip_touch / hip_cg_body; ntouch = 0: the blob has none)
  int ntouch;
  gpf touch;            // [ntouch][TOUCHR]: link of the site (bits) | site position (3) | site rotation (9) in that link's frame | type (bits) | half sizes (3) | body (bits)
  gpi cg_body;          // [ncg] body id of every collision geom
};
#define TOUCHR 20
#define MYO_MAX_TOUCH 8
#define SEGR 9
#ifndef MPR_TOL
#define MPR_TOL 1e-8f      // portal refinement stops when the support plane gains less than this (metres)
#endif
// Dof trees of the size-specialised instantiations (parent dof of each dof; myo_model_load checks the model's dof_parentid against them
// before it selects a specialised instantiation).  The mass matrix M and M + h D couple a dof only with its ancestors and descendants:
// factorised LEAVES FIRST (lane i <-> dof nv - 1 - i) the Cholesky factor keeps exactly that pattern, no fill-in (Featherstone; MuJoCo's
// L^T D L does the same) -- MyoHand 93 of 253 entries below the diagonal, MyoLeg 317 of 561.
template <int SPEC> struct SpecTree { static constexpr int nv = 0; static constexpr int parent[1] = {-1}; };
template <> struct SpecTree<1> { static constexpr int nv = 23;
  static constexpr int parent[23] = {-1, 0, 1, 2, 3, 4, 5, 2, 7, 8, 9, 2, 11, 12, 13, 2, 15, 16, 17, 2, 19, 20, 21}; };
template <> struct SpecTree<2> { static constexpr int nv = 34;
  static constexpr int parent[34] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 8, 17, 18, 5, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29, 22, 31, 32}; };
template <> struct SpecTree<3> : SpecTree<2> {};
#include "myo_wave_util.h"

// Substep-granular dynamic scheduling (opt-in, MYO_SCHED=1).  With one workgroup per env, a launch of B = 4096 envs fills every
// wave slot of the chip exactly once and lasts as long as its slowest SIMD (env work varies +-12 %).  Here the waves are
// persistent instead: the unit of work is ONE substep of one env.  Each XCD owns a FIFO ring of its envs (state stays in that
// XCD's L2); a wave takes a ticket, waits until the ticket's slot is published, loads the env's state, runs the substep, stores
// the state and publishes the env's next substep at the tail.  Envs advance in near lock-step, so the imbalance that is left is
// that of a single substep.  No wave ever waits while it holds work, published work is always held by a running wave, and the
// ticket count is fixed (envs x substeps), so every wave terminates; spins are capped anyway and a timeout raises a flag.
struct SchedDev {
  int* ctl;      // [8][4]: head (next ticket), tail (next publish index), n (envs of this queue), error
  int* ring;     // [nqueue][stride]: gen << 24 | substep << 20 | env
  int stride, nsubtot;
  int nqueue;    // queues in use = XCDs of the device (or of its partition: 8 in SPX mode, 4 / 2 / 1 in DPX / QPX / CPX, from the CU count):
                 // a wave serves queue XCC_ID % nqueue, so no queue is left without waves when fewer than 8 XCDs are visible
};
#define SCHED_ENV_MASK 0xFFFFF
__global__ void __launch_bounds__(1024) sched_init_kernel(const int* __restrict__ diag, int B, SchedDev S) {
  __shared__ int hist[256], start[256];
  __shared__ int cmax_s;
  const int t = threadIdx.x;
  if (t < 256) hist[t] = 0;
  if (t == 0) cmax_s = 1;
  const int nqu = S.nqueue;
  if (t < 8) { int n = t < nqu ? (B - t + nqu - 1) / nqu : 0; S.ctl[4 * t] = 0; S.ctl[4 * t + 1] = n; S.ctl[4 * t + 2] = n; S.ctl[4 * t + 3] = 0; }
  __syncthreads();
  int cm = 1;
  for (int e = t; e < B; e += 1024) cm = max(cm, diag[(size_t)e * 8 + 3]);
  atomicMax(&cmax_s, cm);
  __syncthreads();
  const int cmax = cmax_s;
  for (int e = t; e < B; e += 1024) atomicAdd(&hist[255 - min(255, (int)(255LL * diag[(size_t)e * 8 + 3] / cmax))], 1);   // bucket 0 = heaviest
  __syncthreads();
  if (t == 0) { int acc = 0; for (int k = 0; k < 256; k++) { start[k] = acc; acc += hist[k]; } }
  __syncthreads();
  for (int e = t; e < B; e += 1024) {
    int b = 255 - min(255, (int)(255LL * diag[(size_t)e * 8 + 3] / cmax));
    int r = atomicAdd(&start[b], 1);                  // rank by descending predicted cost: heavy envs are served first
    S.ring[(r % nqu) * S.stride + r / nqu] = e;       // generation 0, substep 0
  }
}

// table sizes of the compiled config models (after lowering): SPEC = 1 (MyoHand, myohand_pose.xml) and SPEC = 2 (MyoLeg, myolegs.xml)
// instantiations of the wave kernel take their loop bounds from here; SPEC = 0 reads them from the model at run time
template <int SPEC> struct Sizes { static constexpr int nq = 0, nv = 0, nu = 0, nl = 0, nlevel = 0, maxnnz = 0, nseg = 0, ncg = 0, npair = 0; };
template <> struct Sizes<1> { static constexpr int nq = 23, nv = 23, nu = 39, nl = 17, nlevel = 5, maxnnz = 7, nseg = 116, ncg = 27, npair = 289; };
template <> struct Sizes<2> { static constexpr int nq = 35, nv = 34, nu = 80, nl = 13, nlevel = 6, maxnnz = 11, nseg = 100, ncg = 32, npair = 45; };
template <> struct Sizes<3> { static constexpr int nq = 35, nv = 34, nu = 80, nl = 13, nlevel = 6, maxnnz = 11, nseg = 100, ncg = 33, npair = 76; };   // MyoLeg + colliding height field
template <int SPEC> static bool sizes_match(int nq, int nv, int nu, int nl, int nlevel, int maxnnz, int ngt, int nseg, int ncg, int npair) {
  typedef Sizes<SPEC> Z;
  return nq == Z::nq && nv == Z::nv && nu == Z::nu && nl == Z::nl && nlevel == Z::nlevel && maxnnz == Z::maxnnz && ngt == Z::nu && nseg == Z::nseg &&
         ncg == Z::ncg && npair == Z::npair;
}

// compile-time layout of a size-specialised instantiation (SPEC models have no tendon limits: myo_model_load checks it)
template <int SPEC, int NVT, int KC, int NC, int NJ> struct LayC {
  typedef Sizes<SPEC> Z;
  static constexpr LayW L = layout_w(Z::nq, Z::nv, Z::nu, Z::nl, Z::nu, Z::maxnnz, Z::ncg, false, NVT, KC, NC, NJ);
  static constexpr int qpos = L.qpos, qvel = L.qvel, act = L.act, ctrl = L.ctrl, lpos = L.lpos, lmat = L.lmat, axis = L.axis, anchor = L.anchor, xv = L.xv,
                       qfc = L.qfc, sq = L.sq, mprw = L.mprw, X = L.X, tJ = L.tJ, tlen = L.tlen, tforce = L.tforce, cdof = L.cdof, cinert = L.cinert, crb = L.crb,
                       cvel = L.cvel, cacc = L.cacc, cfrc = L.cfrc, gpos = L.gpos, gax = L.gax, cand = L.cand, cdist = L.cdist, cpos = L.cpos, cnrm = L.cnrm,
                       cpair = L.cpair, cJ = L.cJ, cdofs = L.cdofs, Mp = L.Mp, tJp = L.tJp, total = L.total;
};
template <int SPEC, int NVT, int KC, int NC, int NJ> static bool layout_match(const LayW& a) {
  const LayW b = layout_w(Sizes<SPEC>::nq, Sizes<SPEC>::nv, Sizes<SPEC>::nu, Sizes<SPEC>::nl, Sizes<SPEC>::nu, Sizes<SPEC>::maxnnz, Sizes<SPEC>::ncg, false, NVT, KC, NC, NJ);
  return memcmp(&a, &b, sizeof(LayW)) == 0;
}

#include "myo_wave_motion.h"
#include "myo_wave_collision.h"
#include "myo_wave_solver.h"

// TRK (MyoDM TrackEnv model class): condim-4 contacts (6 pyramid rows, a 4th jacobian row for the spin about the normal), joint friction-loss
// rows, box / convex-hull shapes in the narrow phase.  All of it sits behind `if constexpr (TRK)`: the other instantiations compile as before.
// RK4: mj_RungeKutta(4) instead of mj_Euler -- every substep runs the whole forward pass four times (state X0 + h a F[i-1], a = 1/2, 1/2, 1)
// and ends on X0 + h (F0 + 2 F1 + 2 F2 + F3) / 6; the saved state and the weighted derivative sums live in the registers of lane = dof /
// lane = actuator.  No implicit joint damping (an Euler-only feature of MuJoCo).
// The body of the kernel is the text of myo_kernel_wave_body.h, compiled inside two kernel templates:
//   step_kernel_w        OBJ = false.  Its instantiations are the step kernels of every model and compile to the code they had before OBJ existed.
//   step_kernel_obj      OBJ = true: per-env object parameters (include/myo_hip_objects.h) -- the selected geoms' size, centre and friction and
//                        the selected bodies' mass come from the batch's rows (DevBatch.objk / obj_mass), each behind a wave-uniform null
//                        test.  One instantiation, with the TRK arguments: what a TrackEnv-class batch runs after myo_objects_enable.
// (A textual include rather than a shared __device__ function: through a function boundary, even a force-inlined one, the compiler lays the
// other instantiations out differently -- other register counts and code sizes, which tests/test_forward_resources.py pins.)
template <int NVT, int KC, int NC, int NTR, int WPE, bool SCHED, int SPEC, bool HF = false, bool TRK = false, bool RK4 = false>
__global__ void __launch_bounds__(64, WPE) step_kernel_w(const DevModel* __restrict__ Mp, const DevModelW* __restrict__ Wp, DevBatch Bt,
                                                        const float* __restrict__ action, int actmap, int nsub, long long* stamps,
                                                        const int* __restrict__ order, const DevWalk* __restrict__ wk, int kflags, SchedDev S) {
  constexpr bool OBJ = false;
#include "myo_kernel_wave_body.h"
}
template <int NVT, int KC, int NC, int NTR, int WPE, bool SCHED, int SPEC, bool HF, bool TRK, bool RK4>
__global__ void __launch_bounds__(64, WPE) step_kernel_obj(const DevModel* __restrict__ Mp, const DevModelW* __restrict__ Wp, DevBatch Bt,
                                                          const float* __restrict__ action, int actmap, int nsub, long long* stamps,
                                                          const int* __restrict__ order, const DevWalk* __restrict__ wk, int kflags, SchedDev S) {
  constexpr bool OBJ = true;
#include "myo_kernel_wave_body.h"
}

#undef lane_id
#endif  // MYO_KERNEL_WAVE_H