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
template <int NVT, int KC, int NC, int NTR, int WPE, bool SCHED, int SPEC, bool HF = false, bool TRK = false, bool RK4 = false>
__global__ void __launch_bounds__(64, WPE) step_kernel_w(const DevModel* __restrict__ Mp, const DevModelW* __restrict__ Wp, DevBatch Bt,
                                                        const float* __restrict__ action, int actmap, int nsub, long long* stamps,
                                                        const int* __restrict__ order, const DevWalk* __restrict__ wk, int kflags, SchedDev S) {
  extern __shared__ __align__(16) float E[];
  // the model structs stay in (scalar-cached) global memory: fields are s_load-ed where they are used instead of
  // pinning ~150 SGPRs for the whole kernel
  const DevModel& M = *Mp;
  const DevModelW& W = *Wp;
  // LDS layout: compile-time constants in the size-specialised instantiations (every LDS address an immediate), read from the model otherwise
  const LayC<SPEC, NVT, KC, NC, (TRK ? 4 : 3)> Yc{};
  const auto& Y = [&]() -> const auto& { if constexpr (SPEC != 0) return Yc; else return W.lay; }();
  // workgroup -> env map: a speed-only placement hint (envs sorted by last step's cost, see balance_kernel); results of an
  // env never depend on which workgroup steps it
  const int oe = (!SCHED && order) ? order[blockIdx.x] : blockIdx.x;
  int env = oe & 0x0FFFFFFF;
  // the four waves of a SIMD come from different cost quartiles (balance_kernel); the predicted-heavy ones get a higher issue
  // priority so that the launch's critical path -- its heaviest waves -- is not slowed down by lighter neighbours that have slack
  if (!SCHED) {
    switch (oe >> 28) {
      case 3: __builtin_amdgcn_s_setprio(3); break;
      case 2: __builtin_amdgcn_s_setprio(2); break;
      case 1: __builtin_amdgcn_s_setprio(1); break;
      default: break;
    }
  }
  // SPEC != 0: the model has exactly the table sizes of Sizes<SPEC> (checked by myo_model_load): loop bounds become compile-time
  // constants (+3 % measured on MyoHand); SPEC = 0 reads them from the model
  typedef Sizes<SPEC> Z;
  const int nv = SPEC ? Z::nv : M.nv, nu = SPEC ? Z::nu : M.nu, nq = SPEC ? Z::nq : W.nq;
  const int nl_ = SPEC ? Z::nl : M.nl, nlevel_ = SPEC ? Z::nlevel : M.nlevel, maxnnz_ = SPEC ? Z::maxnnz : M.maxnnz, ngt_ = SPEC ? Z::nu : M.ngt,
            nseg_ = SPEC ? Z::nseg : M.nseg, ncg_ = SPEC ? Z::ncg : M.ncg, npair_ = SPEC ? Z::npair : M.npair;
  typedef WaveCfg<NVT, KC, NC, NTR, WPE, SCHED, SPEC, HF, TRK, RK4> C;
  constexpr int CDW = C::CDW, NJ = C::NJ, NR = C::NR, NCXK = C::NCXK, RND = C::RND;
  constexpr bool FULL = C::FULL, MROW = C::MROW, MHL_A = C::MHL_A, MHL_B = C::MHL_B, MHL_E = C::MHL_E, OVR = C::OVR, LDL_MFMA = C::LDL_MFMA;
  const bool has_free = FULL && W.has_free;
  const int neq = FULL ? W.neq : 0;
  // tendon limits: never in the size-specialised and TRK instantiations (myo_model_load checks it), so their tendon lengths / velocities
  // do not stay live in registers from the tendon stage to the row stage
  const bool has_tl = (SPEC != 0 || TRK) ? false : (W.has_tl != 0);
  const bool walk = FULL && wk != nullptr;   // fused observation / reward pass of the walk task after the last substep
  if (!SCHED && FULL && (kflags & KF_RESET_ONLY) && Bt.elapsed[env] != 0) return;   // wave-uniform: refresh only the envs an auto-reset just touched
#if MYO_STAMPS
  long long st_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  long long st_t0 = clock64();
#endif
  SubStamps st_;
  const int nsubtot = nsub + (walk ? 1 : 0);
  const float h = M.timestep;
  // scheduler state of this wave: the queue of the XCD it runs on
  const int sq_q = SCHED ? (int)(__builtin_amdgcn_s_getreg((31 << 11) | 20) & 7) % S.nqueue : 0;
  int* const sq_ctl = SCHED ? S.ctl + 4 * sq_q : nullptr;
  int* const sq_ring = SCHED ? S.ring + (size_t)sq_q * S.stride : nullptr;
  const int sq_n = SCHED ? sq_ctl[2] : 0;
  int last_cost = 0;
  for (;;) {   // task loop: one (env, substep) per pass when SCHED, a single pass over all substeps of this workgroup's env otherwise
  int s0 = 0, s1 = nsubtot;
  if (SCHED) {
    int t = 0;
    if (lane_id == 0) t = atomicAdd(&sq_ctl[0], 1);
    t = __builtin_amdgcn_readfirstlane(t);
    if (t >= sq_n * nsubtot) break;                       // every ticket of this queue is taken: this wave is done
    const int gen = t / sq_n, slot = t - gen * sq_n;
    int v = 0, spins = 0;
    for (;;) {                                            // wait until the slot of this ticket has been published
      v = __hip_atomic_load(&sq_ring[slot], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((v >> 24) == gen || ++spins > (1 << 21)) break;
      __builtin_amdgcn_s_sleep(8);
    }
    v = __builtin_amdgcn_readfirstlane(v);
    if ((v >> 24) != gen) { if (lane_id == 0) { atomicOr(&Bt.flags[0], MYO_FLAG_SCHED_TIMEOUT); sq_ctl[3] = 1; } break; }
    env = v & SCHED_ENV_MASK;
    s0 = (v >> 20) & 15; s1 = s0 + 1;
  }
  // ---- state: LDS copies of what other lanes gather; per-dof / per-actuator scalars stay in registers.  Under the scheduler the
  // rows were written by another CU of this XCD: agent-scope loads read them from L2 instead of a possibly stale L1 line
  float actdot[NTR];   // (RK4 only)
  // the solver's warm start (= the previous substep's qacc) stays in the batch row Bt.warm between substeps: one coalesced store after the
  // solve, one load before the next (issued ahead of the row stage); a register for it would be live across every stage of the substep and
  // the 16-envs-per-CU LDS slice has no 24 floats to spare
  float* const warm_row = Bt.warm + (size_t)env * nv;
#pragma unroll
  for (int r = 0; r < NTR; r++) actdot[r] = 0.f;
#ifndef MYO_POISON_BITS
#define MYO_POISON_BITS 0x7fc00000
#endif
#if MYO_POISON   // diagnostic build: LDS words start as NaN, so a read of a word this launch never wrote shows up in the results
  // MYO_POISON = 1: everything; 2: state + frames (qpos .. anchor); 3: xv, qfc; 4: sq; 5: mprw / tJp; 6: region X
  { const int lo_ = MYO_POISON == 1 ? 0 : MYO_POISON == 2 ? 0 : MYO_POISON == 3 ? Y.xv : MYO_POISON == 4 ? Y.sq : MYO_POISON == 5 ? Y.mprw : Y.X;
    const int hi_ = MYO_POISON == 1 ? Y.total : MYO_POISON == 2 ? Y.xv : MYO_POISON == 3 ? Y.sq : MYO_POISON == 4 ? Y.mprw : MYO_POISON == 5 ? Y.X : Y.total;
    for (int i = lo_ + lane_id; i < hi_; i += 64) E[i] = __int_as_float(MYO_POISON_BITS); }
  SYNC();
#endif
  if (lane_id < nq) E[Y.qpos + lane_id] = ldstate<SCHED>(Bt.qpos + (size_t)env * nq + lane_id);
  if (lane_id < nv) {
    E[Y.qvel + lane_id] = ldstate<SCHED>(Bt.qvel + (size_t)env * nv + lane_id);
  }
  for (int i = lane_id; i < nu; i += 64) {
    E[Y.act + i] = ldstate<SCHED>(Bt.act + (size_t)env * nu + i);
    float c;
    if (action && s0 == 0) c = action_map(Bt, M.act, action, env, i, nu, actmap);   // the action map runs once per env step
    else c = ldstate<SCHED>(Bt.ctrl + (size_t)env * nu + i);
    E[Y.ctrl + i] = c;
  }
  float time = uniformf(ldstate<SCHED>(Bt.time + env));
  // MYO_TASK_TRACK (TRK models): this launch is a whole TrackEnv.step -- reference row of the pre-step time now, reward / done / reset at the end
  const bool track_on = TRK && Bt.track != nullptr && action != nullptr && actmap == MYO_ACTMAP_CTRLRANGE && nsub > 0;
  if constexpr (TRK) { if (track_on) track_lookup(*Bt.track, env, env + Bt.env_offset, time, Bt.elapsed[env], lane_id); }
  int flags = 0, d_nefc = 0, d_ncon = 0, d_iter = 0, d_cost = 0;
  int f_cand = 0, f_mpr = 0, f_ncon = 0, f_iter = 0, f_itcon = 0, f_ls = 0, f_fact = 0;   // work features of this env step (placement cost model)
  if (SCHED && s0 > 0) {   // accumulators of the earlier substeps of this env step
    const int* D = Bt.diag + (size_t)env * 8;
    int a2 = ldstatei<SCHED>(D + 2), a4 = ldstatei<SCHED>(D + 4), a5 = ldstatei<SCHED>(D + 5), a6 = ldstatei<SCHED>(D + 6), a7 = ldstatei<SCHED>(D + 7);
    d_nefc = ldstatei<SCHED>(D); d_ncon = ldstatei<SCHED>(D + 1);   // the observation pass has no rows of its own: keep the last substep's
    d_iter = a2; f_cand = a4 & 0xFFFF; f_ncon = a4 >> 16; f_mpr = a5; f_itcon = a6 & 0xFFFF; f_iter = a6 >> 16; f_ls = a7 & 0xFFFF; f_fact = a7 >> 16;
  }
  // contacts beyond the NC of LDS live in this env's HBM overflow rows (WaveCfg: NCXK of them, fields O_*)
  float* const ovf_env = Bt.ovf ? Bt.ovf + (size_t)env * Bt.ovf_rows * Bt.ovf_row : nullptr;
  const int ovf_row = Bt.ovf_row;
  const int nct = ovf_env ? NC + NCXK : NC;
  int* const ovf_cand = (!HF && Bt.ovf_cand) ? Bt.ovf_cand + (size_t)env * NCANDX : nullptr;
  typedef std::remove_cv_t<std::remove_reference_t<decltype(Y)>> LY;
  const WaveCtx<LY> X{M, W, Y, Bt, wk, env, nv, nu, nq, nl_, nlevel_, maxnnz_, ngt_, nseg_, ncg_, npair_, has_free, neq, has_tl, h, nsub, kflags, ovf_env, ovf_row, nct, ovf_cand};
  bool alive = true;
  int n_mprw = 0;   // MPR warm-start table (pair id + last contact normal in geom 1's frame): entries of the previous substep
  bool gone = false;   // scheduler: a wave of an earlier substep of this launch found the env bad and reset it (word 62 of the table row, which
                       // the first substep's wave clears): the env's remaining substeps are no-ops, as in the one-wave-per-env launch
  if (SCHED && s0 > 0) {   // ... which another wave ran: the table travels through the batch like the state rows, so that a scheduled
    // launch computes exactly what the one-wave-per-env launch does
    const int* Wt = Bt.mprw + (size_t)env * 64;
    n_mprw = __builtin_amdgcn_readfirstlane(ldstatei<SCHED>(Wt + 63));
    gone = __builtin_amdgcn_readfirstlane(ldstatei<SCHED>(Wt + 62)) != 0;
    if (lane_id < 4 * n_mprw) ((int*)(E + Y.mprw))[lane_id] = ldstatei<SCHED>(Wt + lane_id);
  }
  SYNC();
  // How a bad env leaves this loop (`leave_substeps` below): step = nsub - 1; continue.  The increment makes step = nsub, which is the walk
  // task's observation pass where this wave runs one (no scheduler: s1 = nsub + 1) and the end of the loop everywhere else (no walk task:
  // s1 = nsub; scheduler: s1 = s0 + 1 <= nsub, the observation pass is a task of its own and finds the reset rows).  A `gone` env's physics
  // tasks (s0 < nsub) start at s1, i.e. run nothing; its observation task (s0 == nsub) runs as usual
#define leave_substeps() { step = nsub - 1; continue; }
  for (int step = (gone && s0 < nsub) ? s1 : s0; step < s1; step++) {
    const bool op = walk && step == nsub;   // observation pass: position / velocity stages at the post-step state, then out
    // RK4 state of this substep (dead code otherwise): X0 and the weighted sums of the stage derivatives
    RkAcc<NTR> rk{0.f, 0.f, 0.f, 0.f, 0.f, {1.f, 0.f, 0.f, 0.f}, {}, {}};
    int rk_stage = 0;
  rk_next_stage:
    // compiler-only barrier: keeps the (substep-invariant) model-table loads inside the loop body instead of hoisting
    // ~60 values per lane out of it and spilling them to scratch
    asm volatile("" ::: "memory");
    int lane;   // opaque per-iteration copy of the lane id: address arithmetic derived from it cannot be hoisted (and spilled)
    lane = wave_lane();
    w_check_state<C>(X, lane, op, flags, alive);
    // a bad env (wave-uniform) is reset like mj_resetData on the spot and leaves the substep loop: no stage ever runs on a non-finite state.
    // The walk task's observation pass, if there is one, then runs on the reset state
    if (__builtin_expect(!alive && !op, 0)) { w_reset_bad<C>(X, warm_row, time); leave_substeps(); }
    STAMP(0);
    w_kinematics<C>(X, lane, step);
    STAMP(1);
    SUB0();
    const float qfa = w_tendons<C>(X, lane, step, op, actdot, st_);
    STAMP(2);
    float smooth;
    if (w_dynamics<C>(X, lane, op, qfa, smooth, st_)) break;   // the walk task's observation pass ends here
    STAMP(3);
    int ncon = 0;
    if (!M.disable_contact) {
      const int ncand = w_broad_phase<C>(X, lane, flags, f_cand);
      STAMP(6);
      ncon = w_narrow_phase<C>(X, lane, ncand, n_mprw, flags, f_mpr);
    } else n_mprw = 0;
    STAMP(4);
    // constraint rows (registers: lane = dof / lane = contact)
    const float warm_r = lane < nv ? ldstate<SCHED>(warm_row + lane) : 0.f;   // (its latency hides behind the row stage)
    const LimRow lim = w_limit_rows<C>(X, lane);
    ConConst<NR> con;
    FricLoss fl;
    bool bank1, b1lane;   // TRK, more than 64 contacts: the second bank is in use / this lane also owns one of its contacts
    int nefc = w_contact_rows<C>(X, lane, ncon, lim, con, fl, bank1, b1lane);
    const int ncon_real = ncon;
    if (has_tl) w_tendon_limit_rows<C>(X, lane, con, ncon, nefc, flags);
    const EqRow eq = w_equality_rows<C>(X, lane);
    nefc += neq;
    float mrow[MROW ? NVT : 1];
    w_pack_mass<C>(X, lane, mrow);
    STAMP(5);
    SUB0();
    float qacc, qaccE, cjar[NR];
    int iters;
    // Solver, inline: Newton iterations, then the Euler solve, sharing ONE instance of the unrolled register Cholesky.  phase 0 = Newton,
    // 1 = unconstrained (nefc == 0), 2 = Euler (implicit damping).  (As a stage function with these values as parameters it compiled to slower
    // code, measured against the parent: TrackEnv kernel +0.7 % kernel time, headline +0.1 %, also with the row structs passed by value.)
    // In: nefc, ncon, warm_r, smooth, lim, con, fl, eq, bank1, b1lane, mrow.  Out: qacc (the constrained acceleration: next substep's warm start),
    // qaccE (what the integrator advances the velocity with), cjar (J qacc - aref of the lane's contact rows at the final iterate: the sensor
    // readout takes the forces from it), iters; adds to f_itcon, f_ls, f_fact.
    // LDS: reads Mp, cJ, cdofs (overflow rows / state blocks for contacts >= NC), and sq = M at the first refactor of a substep (MHL_A); writes
    // sq (Hessian, then its factor L with 1 / D in the padding column), xv (warm start / search vector) and qfc (J^T f).  All three are dead
    // afterwards; Mp, cJ, cdofs, cpos, cnrm, cpair stay valid for the sensor readout.
    {
      const float* Mp = E + Y.Mp;
      auto symv_reg = [&](float x, int lane) -> float {      // (lane by value: inside the Newton loop it is that loop's opaque copy, see there)
        if constexpr (MROW) {
          float s0 = 0.f, s1 = 0.f;      // two partial sums: half the dependent chain
#pragma unroll
          for (int k = 0; k < NVT; k += 2) { s0 = fmaf(mrow[k], rdlane(x, k), s0); if (k + 1 < NVT) s1 = fmaf(mrow[k + 1], rdlane(x, k + 1), s1); }
          return s0 + s1;
        } else return symv_lds<NVT>(Mp, x, lane, nv);
      };
      float Ma = 0.f, grad = 0.f, qfc = 0.f, ljar = 0.f, ljv = 0.f, cost = 0.f, fljar = 0.f, fljv = 0.f, ejar = 0.f, ejv = 0.f;
      qaccE = 0.f; qacc = 0.f;
      float cjv[NR];
#pragma unroll
      for (int k = 0; k < NR; k++) { cjar[k] = 0.f; cjv[k] = 0.f; }
      int phase = nefc > 0 ? 0 : 1;
      iters = 0;
      if (phase == 0) {  // start from the warm start (MuJoCo also tries qacc_smooth; the minimiser is the same)
        qacc = warm_r;
        Ma = symv_reg(qacc, lane);
        ljar = lim.sign * qacc - lim.aref;
        if constexpr (TRK) fljar = qacc - fl.aref;
        if (lane < nv) E[Y.xv + lane] = qacc;
        SYNC();
        auto row_jar = [&](const ConRow& R) {
          const float* const cJ = R.cJ;
          const unsigned int* const cdw = R.cdw;
          float an = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
          for (int k = 0; k < KC; k++) {
            float xv = E[Y.xv + CDOFP(cdw, k)]; an += cJ[k] * xv; a1 += cJ[KC + k] * xv; a2 += cJ[2 * KC + k] * xv;
            if constexpr (TRK) a3 += cJ[3 * KC + k] * xv;
          }
          cjar[0] = an + con.mu * a1 - con.aref[0]; cjar[1] = an - con.mu * a1 - con.aref[1]; cjar[2] = an + con.mu * a2 - con.aref[2]; cjar[3] = an - con.mu * a2 - con.aref[3];
          if constexpr (TRK) { cjar[4] = an + con.mut * a3 - con.aref[4]; cjar[5] = an - con.mut * a3 - con.aref[5]; }
        };
        if (lane < ncon) con_row<C>(Y, E, ovf_env, ovf_row, lane, row_jar);
        if constexpr (TRK) {
          if (b1lane) {   // J * warm - aref of the lane's bank-1 contact, into its state block
            const float* g = ovf_env + (lane + 64 - NC) * ovf_row;
            const unsigned int* cdw = (const unsigned int*)(g + C::O_CDW);
            float* S = bank1_state<C>(ovf_env, ovf_row, lane + 64);
            float an = 0, a1 = 0, a2 = 0, a3 = 0;
            for (int k = 0; k < KC; k++) { const float xv = E[Y.xv + CDOFP(cdw, k)]; an += g[C::O_CJ + k] * xv; a1 += g[C::O_CJ + KC + k] * xv; a2 += g[C::O_CJ + 2 * KC + k] * xv; a3 += g[C::O_CJ + 3 * KC + k] * xv; }
            const float mu = S[C::S_MU], mut = S[C::S_MUT];
            S[C::S_JAR] = an + mu * a1 - S[C::S_AREF]; S[C::S_JAR + 1] = an - mu * a1 - S[C::S_AREF + 1]; S[C::S_JAR + 2] = an + mu * a2 - S[C::S_AREF + 2]; S[C::S_JAR + 3] = an - mu * a2 - S[C::S_AREF + 3];
            S[C::S_JAR + 4] = an + mut * a3 - S[C::S_AREF + 4]; S[C::S_JAR + 5] = an - mut * a3 - S[C::S_AREF + 5];
          }
        }
        if (eq.act) ejar = E[Y.xv + eq.d1] + eq.J2 * E[Y.xv + eq.d2] - eq.aref;
      }
      SUB(6);
      bool first = true;
      int sig_prev = -1;
      while (true) {
        const int lane = wave_lane();   // opaque copy again: keeps the 24 per-lane symv addresses from being hoisted out of the loop and spilled
        float r[NVT], rhs, invd;
        bool refactor = true;
        if (phase == 0) {
          // forces of the active rows, J^T f (LDS atomics), cost, gradient; convergence test; then, only if the iteration goes on and
          // the active set differs from the one whose Hessian was factorised last, the Hessian blocks (LDS atomics)
          bool lact = lim.sign != 0.f && ljar < 0;
          float w0 = cjar[0] < 0 ? con.D : 0.f, w1 = cjar[1] < 0 ? con.D : 0.f, w2 = cjar[2] < 0 ? con.D : 0.f, w3 = cjar[3] < 0 ? con.D : 0.f;
          float f0 = -w0 * cjar[0], f1 = -w1 * cjar[1], f2 = -w2 * cjar[2], f3 = -w3 * cjar[3];
          float w4 = 0.f, w5 = 0.f, f4 = 0.f, f5 = 0.f, flforce = 0.f, flcost = 0.f;
          bool flquad = false;
          if constexpr (TRK) {
            w4 = cjar[4] < 0 ? con.D2 : 0.f; w5 = cjar[5] < 0 ? con.D2 : 0.f;
            f4 = -w4 * cjar[4]; f5 = -w5 * cjar[5];
            if (fl.f > 0.f) {
              if (fljar <= -fl.rf) { flforce = fl.f; flcost = fl.f * (-0.5f * fl.rf - fljar); }
              else if (fljar >= fl.rf) { flforce = -fl.f; flcost = fl.f * (-0.5f * fl.rf + fljar); }
              else { flforce = -fl.D * fljar; flcost = 0.5f * fl.D * fljar * fljar; flquad = true; }
            }
          }
          float cst_b1 = 0.f;      // TRK second bank: cost of the lane's bank-1 contact; its force / Hessian coefficients go to its state block
          bool sig_b1_changed = false;
          if constexpr (TRK) {
            if (b1lane) {
              float* S = bank1_state<C>(ovf_env, ovf_row, lane + 64);
              const float D = S[C::S_D], D2 = S[C::S_D2], mu = S[C::S_MU], mut = S[C::S_MUT];
              float w[NR], f[NR];
              int sg = 0;
#pragma unroll
              for (int k = 0; k < NR; k++) {
                const float jr = S[C::S_JAR + k];
                w[k] = jr < 0 ? (k < 4 ? D : D2) : 0.f;
                f[k] = -w[k] * jr;
                cst_b1 += 0.5f * w[k] * jr * jr;
                sg |= (w[k] != 0.f ? 2 : 0) << k;
              }
              S[C::S_FC] = f[0] + f[1] + f[2] + f[3] + f[4] + f[5]; S[C::S_FC + 1] = mu * (f[0] - f[1]); S[C::S_FC + 2] = mu * (f[2] - f[3]); S[C::S_FC + 3] = mut * (f[4] - f[5]);
              S[C::S_HC] = w[0] + w[1] + w[2] + w[3] + w[4] + w[5]; S[C::S_HC + 1] = mu * (w[0] - w[1]); S[C::S_HC + 2] = mu * (w[2] - w[3]);
              S[C::S_HC + 3] = mu * mu * (w[0] + w[1]); S[C::S_HC + 4] = mu * mu * (w[2] + w[3]); S[C::S_HC + 5] = mut * (w[4] - w[5]); S[C::S_HC + 6] = mut * mut * (w[4] + w[5]);
              sig_b1_changed = ((const int*)S)[C::S_SIG] != sg;
              ((int*)S)[C::S_SIG] = sg;
            }
          }
          if (lane < nv) E[Y.qfc + lane] = (lact ? -lim.sign * lim.D * ljar : 0.f) + flforce;
          SYNC();
          if constexpr (KC == 8 || TRK) {
            // J^T f with lane = (contact of the pass, dof slot), 64 / KC contacts per pass: the contact's three (four) force components come from
            // its own lane by shuffle, every lane adds one entry (one lane per contact walking its dofs was the longer chain)
            const float Fn = f0 + f1 + f2 + f3 + f4 + f5, Ft1 = con.mu * (f0 - f1), Ft2 = con.mu * (f2 - f3), Ft3 = con.mut * (f4 - f5);
            constexpr int FG = 64 / KC;
            const int fg = lane / KC, fk = lane - fg * KC;
            for (int c0 = 0; c0 < ncon; c0 += FG) {
              const int c = c0 + fg;
              const bool on = fg < FG && c < ncon;
              const int cs = on ? c : 0;
              float sFn = __shfl(Fn, cs & 63), sF1 = __shfl(Ft1, cs & 63), sF2 = __shfl(Ft2, cs & 63), sF3 = TRK ? __shfl(Ft3, cs & 63) : 0.f;
              int kc = __shfl(con.kc, cs & 63);
              if constexpr (TRK) {
                if (on && c >= 64) { const float* S = bank1_state<C>(ovf_env, ovf_row, c); sFn = S[C::S_FC]; sF1 = S[C::S_FC + 1]; sF2 = S[C::S_FC + 2]; sF3 = S[C::S_FC + 3]; kc = ((const int*)S)[C::S_KC]; }
              }
              if (on && fk < kc) con_row<C>(Y, E, ovf_env, ovf_row, c, [&](const ConRow& R) {
                const float* const cJ = R.cJ;
                atomicAdd(&E[Y.qfc + CDOFP(R.cdw, fk)], sFn * cJ[fk] + sF1 * cJ[KC + fk] + sF2 * cJ[2 * KC + fk] + (TRK ? sF3 * cJ[(NJ - 1) * KC + fk] : 0.f));
              });
            }
          } else if (lane < ncon) {   // MyoLeg (<= 10 contacts of 20 dofs): one lane per contact measured 1 % faster than three contacts per pass
            float Fn = f0 + f1 + f2 + f3 + f4 + f5, Ft1 = con.mu * (f0 - f1), Ft2 = con.mu * (f2 - f3);
            con_row<C>(Y, E, ovf_env, ovf_row, lane, [&](const ConRow& R) {
              const float* const cJ = R.cJ;
              for (int k = 0; k < con.kc; k++) atomicAdd(&E[Y.qfc + CDOFP(R.cdw, k)], Fn * cJ[k] + Ft1 * cJ[KC + k] + Ft2 * cJ[2 * KC + k]);
            });
          }
          if (eq.act) { float f = -eq.D * ejar; atomicAdd(&E[Y.qfc + eq.d1], f); atomicAdd(&E[Y.qfc + eq.d2], eq.J2 * f); }
          SYNC();
          qfc = lane < nv ? E[Y.qfc + lane] : 0.f;
          float cst = lact ? 0.5f * lim.D * ljar * ljar : 0.f;
          cst += 0.5f * eq.D * ejar * ejar;
          cst += 0.5f * (w0 * cjar[0] * cjar[0] + w1 * cjar[1] * cjar[1] + w2 * cjar[2] * cjar[2] + w3 * cjar[3] * cjar[3]);
          if constexpr (TRK) cst += 0.5f * (w4 * cjar[4] * cjar[4] + w5 * cjar[5] * cjar[5]) + flcost + cst_b1;
          cst += 0.5f * qacc * Ma - qacc * smooth;          // Gauss term up to a constant
          float newcost = wave_sum(cst);
          grad = Ma - smooth - qfc;
          if (!first) {
            const float scale = M.newton_scale;   // 1 / (meaninertia * nv), computed at load: a scalar load here instead of a VGPR live across every stage
            float improvement = scale * (cost - newcost);
            float gn = scale * sqrtf(wave_sum(grad * grad));
            // float32 round-off of the gradient's own terms: below it the iteration only chases noise (float32 oracle build: 2.7 -> 1.9
            // Newton iterations per substep with this test, the float64 build needs 1.9; solution unchanged)
            const float gterm = fabsf(Ma) + fabsf(smooth) + fabsf(qfc);
            float gnoise = GRAD_NOISE * scale * sqrtf(wave_sum(gterm * gterm));
            iters++;
            f_itcon += ncon;
            if (improvement < fmaxf(M.tolerance, NEWTON_NOISE * scale * fabsf(newcost)) || gn < fmaxf(M.tolerance, gnoise) || iters >= M.iterations) phase = 2;
          }
          cost = newcost;
          SUB(0);
          if (phase == 0) {
            // H = M + J^T D J depends on the state only through the set of active rows: same set as last time -> same factor
            const int sig = (lact ? 1 : 0) | (w0 != 0.f ? 2 : 0) | (w1 != 0.f ? 4 : 0) | (w2 != 0.f ? 8 : 0) | (w3 != 0.f ? 16 : 0) |
                            (TRK ? ((w4 != 0.f ? 32 : 0) | (w5 != 0.f ? 64 : 0) | (flquad ? 128 : 0)) : 0);
            refactor = first || __any(sig != sig_prev || sig_b1_changed);
            sig_prev = sig;
            if (refactor) {
              f_fact++;
              // the Hessian buffer starts as M (lower rows; identity rows for the padding lanes) plus the limit / friction-loss diagonal, and the contact
              // blocks are added on top: the factorisation then reads finished rows instead of combining two LDS reads and three selects per entry
              // (MHL_A: at the first refactor of a substep the buffer still holds this substep's M -- lower rows, zeros above the diagonal and in
              // the rows of the padding lanes; nothing has written it since the dynamics stage -- so only the diagonal term goes in)
              if (MHL_A && first) {
                if (lane < NVT) {
                  const float dg_ = (lane < nv) ? ((lact ? lim.D : 0.f) + (flquad ? fl.D : 0.f)) : 1.f;
                  const float mv_ = lane < nv ? E[Y.sq + lane * (NVT + 1) + lane] : 0.f;
                  E[Y.sq + lane * (NVT + 1) + lane] = mv_ + dg_;
                }
              } else if (MHL_E && !first) {      // (MYO_MHL_A=0: the first refactor takes the full refill below)
                // a later refactor of the substep: the buffer holds L, i.e. exact zeros from the diagonal on, so only what lies below the diagonal
                // comes back from the packed copy, and the whole wave moves it (tri_pair): 2 x 5 LDS instructions for 24 dofs where lane = row takes 2 x 24.
                // The diagonal goes in as before, from the lane that owns the row's diagonal term.
#pragma unroll
                for (int i0 = 0; i0 < TRI_N<NVT>; i0 += 64) {
                  int d, k;
                  tri_pair<NVT>(i0 + lane, d, k);
                  if (i0 + lane < TRI_N<NVT> && k < d) E[Y.sq + d * (NVT + 1) + k] = d < nv ? Mp[(d * (d + 1)) / 2 + k] + 0.f : 0.f;
                }
                if (lane < NVT) {
                  const float dg_ = (lane < nv) ? ((lact ? lim.D : 0.f) + (flquad ? fl.D : 0.f)) : 1.f;
                  const float mv_ = lane < nv ? Mp[(lane * (lane + 1)) / 2 + lane] : 0.f;
                  E[Y.sq + lane * (NVT + 1) + lane] = mv_ + dg_;
                }
              } else if (lane < NVT) {
                const int dd_ = lane < nv ? lane : 0;
                const int based_ = (dd_ * (dd_ + 1)) / 2;
                const float dg_ = (lane < nv) ? ((lact ? lim.D : 0.f) + (flquad ? fl.D : 0.f)) : 1.f;
#pragma unroll
                for (int k = 0; k < NVT; k++) {
                  float mv_;
                  if constexpr (MROW) mv_ = (k <= lane) ? mrow[k] : 0.f;
                  else mv_ = (lane < nv && k <= lane) ? Mp[based_ + (k <= dd_ ? k : 0)] : 0.f;
                  E[Y.sq + lane * (NVT + 1) + k] = mv_ + (k == lane ? dg_ : 0.f);
                }
              }
              float Wn = w0 + w1 + w2 + w3 + w4 + w5, A1 = con.mu * (w0 - w1), A2 = con.mu * (w2 - w3), B1 = con.mu * con.mu * (w0 + w1), B2 = con.mu * con.mu * (w2 + w3);
              const float A3 = con.mut * (w4 - w5), B3 = con.mut * con.mut * (w4 + w5);
              SYNC();
              // 64 / KC contacts per pass, lane = (contact of the pass, row a of its kc x kc block): the lane folds the contact's weights into
              // its row (hv = n_b p_n + t1_b p_t + t2_b p_u [+ s_b p_s]) and walks the columns b; the entries of different contacts meet in
              // the LDS atomics.  (One contact per pass with lane = block entry spent 7 passes per contact on a 20-dof block, half of the
              // lanes above the diagonal: 25 % of the TrackEnv kernel.)
              {
                constexpr int HG = 64 / KC;
                const int hg = lane / KC, ha = lane - hg * KC;
                for (int c0 = 0; c0 < ncon; c0 += HG) {
                  const int c = c0 + hg;
                  const bool on = hg < HG && c < ncon;
                  const int cs = on ? c : 0;
                  float sW = __shfl(Wn, cs & 63), sA1 = __shfl(A1, cs & 63), sA2 = __shfl(A2, cs & 63), sB1 = __shfl(B1, cs & 63), sB2 = __shfl(B2, cs & 63);
                  float sA3 = TRK ? __shfl(A3, cs & 63) : 0.f, sB3 = TRK ? __shfl(B3, cs & 63) : 0.f;
                  int kc = __shfl(con.kc, cs & 63);
                  if constexpr (TRK) {
                    if (on && c >= 64) {
                      const float* S = bank1_state<C>(ovf_env, ovf_row, c);
                      sW = S[C::S_HC]; sA1 = S[C::S_HC + 1]; sA2 = S[C::S_HC + 2]; sB1 = S[C::S_HC + 3]; sB2 = S[C::S_HC + 4]; sA3 = S[C::S_HC + 5]; sB3 = S[C::S_HC + 6]; kc = ((const int*)S)[C::S_KC];
                    }
                  }
                  if (on && sW != 0.f && ha < kc) {
                    auto hrow = [&](const ConRow& R) {
                      const float* const cJ = R.cJ;
                      const unsigned int* const cdw = R.cdw;
                      const int da = CDOFP(cdw, ha);
                      const float na = cJ[ha], ta = cJ[KC + ha], ua = cJ[2 * KC + ha];
                      float pn = sW * na + sA1 * ta + sA2 * ua, ps = 0.f;
                      const float pt = sA1 * na + sB1 * ta, pu = sA2 * na + sB2 * ua;
                      if constexpr (TRK) { const float sa = cJ[3 * KC + ha]; pn += sA3 * sa; ps = sA3 * na + sB3 * sa; }
                      for (int hb0 = 0; hb0 < kc; hb0 += 4) {   // four columns at a time: all reads first, then the atomics back to back
                        float hv[4];
                        int db[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                          const int hb = min(hb0 + u, KC - 1);      // (measured: without the clamp the reads merge into wide LDS loads and the TRK assembly gets 20 % slower)
                          db[u] = (hb0 + u < kc) ? CDOFP(cdw, hb) : 0x7fffffff;
                          hv[u] = pn * cJ[hb] + pt * cJ[KC + hb] + pu * cJ[2 * KC + hb];
                          if constexpr (TRK) hv[u] += ps * cJ[3 * KC + hb];
                        }
#pragma unroll
                        for (int u = 0; u < 4; u++) if (da >= db[u]) atomicAdd(&E[Y.sq + da * (NVT + 1) + db[u]], hv[u]);
                      }
                    };
                    con_row<C>(Y, E, ovf_env, ovf_row, c, hrow);
                  }
                }
              }
              if (eq.act) {
                atomicAdd(&E[Y.sq + eq.d1 * (NVT + 1) + eq.d1], eq.D);
                atomicAdd(&E[Y.sq + eq.d2 * (NVT + 1) + eq.d2], eq.D * eq.J2 * eq.J2);
                atomicAdd(&E[Y.sq + max(eq.d1, eq.d2) * (NVT + 1) + min(eq.d1, eq.d2)], eq.D * eq.J2);
              }
              SYNC();
            }
          }
          first = false;
          SUB(1);
        }
        rhs = phase == 0 ? -grad : (phase == 1 ? smooth : smooth + qfc);
        float x;
        if (SPEC != 0 && !RK4 && phase != 0) {
          // unconstrained and Euler solves of the size-specialised instantiations: M (+ h D) factorised leaves first, tree-sparse
          constexpr int NVS = SpecTree<SPEC>::nv > 0 ? SpecTree<SPEC>::nv : 1;
          const bool act = lane < NVS;
          const int q = act ? NVS - 1 - lane : 0;                   // this lane's dof in leaves-first order
          const float dadd = phase == 2 ? h * M.dof_damping[q] : 0.f;
          const float rhs_p = act ? __shfl(rhs, q) : 0.f;
#pragma unroll
          for (int k = 0; k < NVT; k++) {
            const int qk = k < NVS ? NVS - 1 - k : 0;               // compile-time after unrolling; qk >= q where k <= lane
            const float mv = (act && k <= lane) ? Mp[(qk * (qk + 1)) / 2 + q] : 0.f;
            r[k] = act ? mv + (k == lane ? dadd : 0.f) : (k == lane ? 1.f : 0.f);
          }
          SYNC();
          invd = chol_rows_tree<NVT, SPEC>(r, lane);
          if (lane < NVT) {
#pragma unroll
            for (int k = 0; k < NVT; k++) E[Y.sq + lane * (NVT + 1) + k] = r[k];
            E[Y.sq + lane * (NVT + 1) + NVT] = invd;
          }
          SYNC();
          SUBX(1);
          const float xp = chol_solve_rows<NVT>(r, invd, rhs_p, E + Y.sq, lane);
          x = __shfl(xp, act ? NVS - 1 - lane : lane);
        } else {
        // Newton refactor on the matrix cores: L and 1 / D replace the Hessian in the buffer, the rows are then reloaded like a reused factor
        if constexpr (LDL_MFMA) {
          if (refactor && phase == 0) {
            ldl_mfma<NVT>(E + Y.sq, lane);
            SYNC();
          }
        }
        if (refactor && !(LDL_MFMA && phase == 0)) {
          if (phase == 0) {          // Newton: the buffer already holds M + the diagonal terms + J^T D J (see the assembly above)
            const int ll_ = lane < NVT ? lane : 0;
#pragma unroll
            for (int k = 0; k < NVT; k++) r[k] = lane < NVT ? E[Y.sq + ll_ * (NVT + 1) + k] : 0.f;
          } else {                   // unconstrained / Euler solves of the instantiations without a tree-sparse path: M (+ h D)
            const int dd = lane < nv ? lane : 0;
            const int based = (dd * (dd + 1)) / 2;
            const float diag_add = (phase == 2 && !RK4) ? h * M.dof_damping[dd] : 0.f;
#pragma unroll
            for (int k = 0; k < NVT; k++) {
              float mv;
              if constexpr (MROW) mv = (k <= lane) ? mrow[k] : 0.f;                                      // lower row of M (zero for lanes >= nv)
              else mv = (lane < nv && k <= lane) ? Mp[based + (k <= dd ? k : 0)] : 0.f;
              r[k] = (lane < nv) ? mv + (k == lane ? diag_add : 0.f) : (k == lane ? 1.f : 0.f);
            }
          }
          SYNC();
          invd = chol_rows<NVT>(r, lane);
          if (lane < NVT) {
#pragma unroll
            for (int k = 0; k < NVT; k++) E[Y.sq + lane * (NVT + 1) + k] = r[k];
            E[Y.sq + lane * (NVT + 1) + NVT] = invd;      // 1 / D in the padding column, for the iterations that reuse the factor
          }
          SYNC();
        } else {
          // the factor of the previous iteration (or the one ldl_mfma just wrote) is in LDS (row-major L): reload this lane's row
          const int ll = lane < NVT ? lane : 0;
#pragma unroll
          for (int k = 0; k < NVT; k++) r[k] = E[Y.sq + ll * (NVT + 1) + k];
          invd = E[Y.sq + ll * (NVT + 1) + NVT];
        }
        if (refactor && phase == 0) { SUBX(0); CNTX(2); } else SUB(2);
        x = chol_solve_rows<NVT>(r, invd, rhs, E + Y.sq, lane);
        }
        SUB(3);
        if (phase == 1) { qacc = x; qfc = 0.f; phase = 2; continue; }
        if (phase == 2) { qaccE = x; break; }
        // ---- Newton: exact line search along x
        float search = lane < nv ? x : 0.f;
        float Mv = symv_reg(search, lane);
        ljv = lim.sign * search;
        if constexpr (TRK) fljv = search;
        if (lane < nv) E[Y.xv + lane] = search;
        SYNC();
        auto row_jv = [&](const ConRow& R) {
          const float* const cJ = R.cJ;
          const unsigned int* const cdw = R.cdw;
          float an = 0, a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
          for (int k = 0; k < KC; k++) {
            float xv = E[Y.xv + CDOFP(cdw, k)]; an += cJ[k] * xv; a1 += cJ[KC + k] * xv; a2 += cJ[2 * KC + k] * xv;
            if constexpr (TRK) a3 += cJ[3 * KC + k] * xv;
          }
          cjv[0] = an + con.mu * a1; cjv[1] = an - con.mu * a1; cjv[2] = an + con.mu * a2; cjv[3] = an - con.mu * a2;
          if constexpr (TRK) { cjv[4] = an + con.mut * a3; cjv[5] = an - con.mut * a3; }
        };
        if (lane < ncon) con_row<C>(Y, E, ovf_env, ovf_row, lane, row_jv);
        if constexpr (TRK) {
          if (b1lane) {   // J * search of the lane's bank-1 contact, into its state block
            const float* g = ovf_env + (lane + 64 - NC) * ovf_row;
            const unsigned int* cdw = (const unsigned int*)(g + C::O_CDW);
            float* S = bank1_state<C>(ovf_env, ovf_row, lane + 64);
            float an = 0, a1 = 0, a2 = 0, a3 = 0;
            for (int k = 0; k < KC; k++) { const float xv = E[Y.xv + CDOFP(cdw, k)]; an += g[C::O_CJ + k] * xv; a1 += g[C::O_CJ + KC + k] * xv; a2 += g[C::O_CJ + 2 * KC + k] * xv; a3 += g[C::O_CJ + 3 * KC + k] * xv; }
            const float mu = S[C::S_MU], mut = S[C::S_MUT];
            S[C::S_JV] = an + mu * a1; S[C::S_JV + 1] = an - mu * a1; S[C::S_JV + 2] = an + mu * a2; S[C::S_JV + 3] = an - mu * a2; S[C::S_JV + 4] = an + mut * a3; S[C::S_JV + 5] = an - mut * a3;
          }
        }
        if (eq.act) ejv = E[Y.xv + eq.d1] + eq.J2 * E[Y.xv + eq.d2];
        float g1 = wave_sum(search * (Ma - smooth)), g2 = wave_sum(0.5f * search * Mv), sn = sqrtf(wave_sum(search * search));
        SUB(4);
        float alpha = 0, lo = 0, hi = -1, dlo = 0, d2lo = 0, dhi = 0, d2hi = 0, d1init = 0;
        bool ls_on = sn >= MINVALF;
        for (int lsit = -1; lsit < M.ls_iterations && ls_on; lsit++) {
          float a = (lsit < 0) ? 0.f : alpha;
          float p1 = 0, p2 = 0;
          if (lim.sign != 0.f) { float xx = ljar + a * ljv; if (xx < 0) { p1 += lim.D * xx * ljv; p2 += lim.D * ljv * ljv; } }
          p1 += eq.D * (ejar + a * ejv) * ejv; p2 += eq.D * ejv * ejv;
#pragma unroll
          for (int k = 0; k < 4; k++) { float xx = cjar[k] + a * cjv[k]; if (xx < 0) { p1 += con.D * xx * cjv[k]; p2 += con.D * cjv[k] * cjv[k]; } }
          if constexpr (TRK) {
#pragma unroll
            for (int k = 4; k < 6; k++) { float xx = cjar[k] + a * cjv[k]; if (xx < 0) { p1 += con.D2 * xx * cjv[k]; p2 += con.D2 * cjv[k] * cjv[k]; } }
            if (fl.f > 0.f) {
              const float xx = fljar + a * fljv;
              if (xx <= -fl.rf) p1 -= fl.f * fljv;
              else if (xx >= fl.rf) p1 += fl.f * fljv;
              else { p1 += fl.D * xx * fljv; p2 += fl.D * fljv * fljv; }
            }
            if (b1lane) {   // (state block re-read per evaluation: a handful of L2 hits on a path that exists for > 64 contacts only)
              const float* S = bank1_state<C>(ovf_env, ovf_row, lane + 64);
              const float D = S[C::S_D], D2 = S[C::S_D2];
#pragma unroll
              for (int k = 0; k < NR; k++) { const float jv = S[C::S_JV + k], xx = S[C::S_JAR + k] + a * jv, Dk = k < 4 ? D : D2; if (xx < 0) { p1 += Dk * xx * jv; p2 += Dk * jv * jv; } }
            }
          }
          const float sp1 = wave_sum(p1);
          float d1 = sp1 + g1 + 2 * a * g2;
          float d2 = wave_sum(p2) + 2 * g2;
          if (lsit < 0) {
            if (d1 >= 0 || d2 <= 0) { ls_on = false; alpha = 0; break; }
            dlo = d1; d2lo = d2; d1init = fabsf(d1);
            alpha = -d1 / d2;
            continue;
          }
          f_ls++;
          // stop when the slope is below MuJoCo's tolerance -- or below the float32 round-off of the terms that cancel in it: without
          // the second test the search chases noise (measured on the float32 oracle build: 4.6 -> 1.45 evaluations per search, the float64
          // build needs 1.6; solution unchanged)
          float gtol = fmaxf(fmaxf(M.tolerance * M.ls_tolerance * sn / M.newton_scale, LS_FLOOR * d1init), LS_NOISE * (fabsf(g1) + fabsf(2 * a * g2) + fabsf(sp1)));
          if (fabsf(d1) < gtol) break;
          if (d1 < 0) { lo = alpha; dlo = d1; d2lo = d2; } else { hi = alpha; dhi = d1; d2hi = d2; }
          float cand = alpha - d1 / d2;
          if (hi < 0) {
            if (!(cand > lo)) break;
            alpha = cand;
          } else {
            if (!(cand > lo && cand < hi)) {
              float c2 = d1 < 0 ? hi - dhi / d2hi : lo - dlo / d2lo;
              cand = (c2 > lo && c2 < hi) ? c2 : 0.5f * (lo + hi);
            }
            if (cand == alpha || hi - lo <= 1e-7f * hi) break;
            alpha = cand;
          }
        }
        SUB(5);
        if (!(alpha > 0)) { phase = 2; continue; }   // no descent left: keep qacc / qfc of this iterate
        qacc += alpha * search; Ma += alpha * Mv; ljar += alpha * ljv; ejar += alpha * ejv;
        if constexpr (TRK) fljar += alpha * fljv;
#pragma unroll
        for (int k = 0; k < NR; k++) cjar[k] += alpha * cjv[k];
        if constexpr (TRK) {
          if (b1lane) {
            float* S = bank1_state<C>(ovf_env, ovf_row, lane + 64);
#pragma unroll
            for (int k = 0; k < NR; k++) S[C::S_JAR + k] += alpha * S[C::S_JV + k];
          }
        }
      }
    }
    STAMP(7);
    d_nefc = nefc; d_ncon = ncon_real; d_iter = max(d_iter, iters);
    f_ncon += ncon; f_iter += iters;
    {  // mj_checkAcc.  Both accelerations: a line search that finds no descent on non-finite data keeps the (finite) warm start as qacc,
       // while the Euler solve carries the non-finite forces into qaccE -- the env is bad in this substep, not by its velocities in the next
      bool bad = lane < nv && !(fabsf(qacc) <= MAXVALF && fabsf(qaccE) <= MAXVALF);   // (a NaN fails the comparison)
      if (__builtin_expect(__any(bad), 0)) { flags |= MYO_FLAG_BAD_QACC; alive = false; w_reset_bad<C>(X, warm_row, time); leave_substeps(); }   // (as above)
    }
    if (lane < nv) warm_row[lane] = qacc;
    if constexpr (FULL && !TRK && !RK4) {   // on the last substep of the launch only (under the scheduler: by the wave that runs it)
      if (Bt.sens && step == nsub - 1) w_touch_sensors<C>(X, lane, ncon_real, con, cjar);
    }
    if constexpr (RK4) {
      w_integrate_rk4<C>(X, lane, rk_stage, rk, actdot, qaccE, time);
      SYNC();
      if (++rk_stage < 4) goto rk_next_stage;
    } else {
      w_integrate_euler<C>(X, lane, qaccE, time);
    }
    SYNC();
    STAMP(8);
  }
#undef leave_substeps
  if (!SCHED && FULL && (kflags & KF_AUX)) return;   // observation-only launch: the state arrays are not touched
  bool track_reset = false;
  if constexpr (TRK) { if (track_on) track_reset = w_track_epilogue<C>(X, warm_row, time, !alive); }
  if (lane_id < nq) Bt.qpos[(size_t)env * nq + lane_id] = E[Y.qpos + lane_id];
  if (lane_id < nv) {
    Bt.qvel[(size_t)env * nv + lane_id] = E[Y.qvel + lane_id];
    Bt.qacc[(size_t)env * nv + lane_id] = warm_row[lane_id];   // (= the last substep's qacc; zero for an env that was just reset, like mj_resetData)
  }
  for (int i = lane_id; i < nu; i += 64) {
    Bt.act[(size_t)env * nu + i] = E[Y.act + i];
    Bt.ctrl[(size_t)env * nu + i] = E[Y.ctrl + i];
  }
  if (SCHED && s1 < nsubtot) {
    int* Wt = Bt.mprw + (size_t)env * 64;
    if (lane_id < 4 * n_mprw) Wt[lane_id] = ((const int*)(E + Y.mprw))[lane_id];
    if (lane_id == 63) Wt[63] = n_mprw;
    if (lane_id == 62 && (s0 == 0 || !alive)) Wt[62] = alive ? 0 : 1;
  }
  if (lane_id == 0) {
    Bt.time[env] = time;
    if (s1 == nsubtot) Bt.elapsed[env] = track_reset ? 0 : Bt.elapsed[env] + 1;
    if (SCHED) { if (flags) atomicOr(&Bt.flags[env], flags); } else Bt.flags[env] |= flags;
    Bt.diag[(size_t)env * 8 + 0] = d_nefc; Bt.diag[(size_t)env * 8 + 1] = d_ncon; Bt.diag[(size_t)env * 8 + 2] = d_iter;
    // predicted work of this env's NEXT step for the placement hint, in units of 1024 single-wave cycles: linear model of this
    // step's work features and the last substep's contact / row counts, fitted on one-wave-per-SIMD runs where a wave's duration is
    // its own work (tools/gpu_cost_fit2.py; correlation with the next step's measured duration 0.92 hand / 0.90 legs)
    d_cost = FULL ? 1909 + ((7436 * f_cand - 28892 * f_ncon + 1362 * f_mpr + 25014 * f_iter + 2046 * f_itcon - 1413 * f_ls + 13292 * d_nefc + 343707 * d_ncon) >> 10)
                  : 2236 + ((-141 * f_cand - 3413 * f_ncon + 2188 * f_mpr + 8971 * f_iter - 107 * f_itcon - 122 * f_ls - 518 * d_nefc + 74475 * d_ncon) >> 10);
    d_cost = max(d_cost, 1);
    Bt.diag[(size_t)env * 8 + 3] = d_cost;
    Bt.diag[(size_t)env * 8 + 4] = f_cand | (f_ncon << 16); Bt.diag[(size_t)env * 8 + 5] = f_mpr;
    Bt.diag[(size_t)env * 8 + 6] = f_itcon | (f_iter << 16); Bt.diag[(size_t)env * 8 + 7] = f_ls | (f_fact << 16);
  }
  last_cost = d_cost;
  STAMP(9);
  if (!SCHED) break;
  // publish this env's next substep: the state rows written above must have reached L2 before the ring entry becomes visible
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
  if (s1 < nsubtot && lane_id == 0) {
    const int tt = atomicAdd(&sq_ctl[1], 1);
    const int g2 = tt / sq_n, sl = tt - g2 * sq_n;
    __hip_atomic_store(&sq_ring[sl], (g2 << 24) | (s1 << 20) | env, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  SYNC();   // the next task reuses this wave's LDS slice
  }  // task loop
#if MYO_STAMPS
  st_acc[10] = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID: wave/simd/cu/sh/se ids (placement census)
  st_acc[11] = (__builtin_amdgcn_s_getreg((31 << 11) | 20) & 0xFF) | ((long long)(oe >> 28) << 8) | ((long long)last_cost << 16);   // HW_REG_XCC_ID, issue priority, cost estimate
  if (stamps && lane_id == 0) for (int k = 0; k < 12; k++) { stamps[(size_t)blockIdx.x * 12 + k] = st_acc[k]; stamps[((size_t)gridDim.x + blockIdx.x) * 12 + k] = st_.sub[k];
                                                stamps[((size_t)2 * gridDim.x + blockIdx.x) * 12 + k] = st_.x[k]; }
#endif
}

#undef lane_id
#endif  // MYO_KERNEL_WAVE_H