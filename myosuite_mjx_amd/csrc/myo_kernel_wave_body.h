// myo_kernel_wave_body.h -- the body of the wave-per-env step kernel: prologue, substep loop (stages of myo_wave_*.h, the inline Newton solver),
// epilogue.  Not a header in the usual sense: myo_kernel_wave.h includes this text inside the braces of step_kernel_w and of step_kernel_obj,
// with the ten template parameters, the kernel arguments and `constexpr bool OBJ` in scope.  No include guard (it is included twice).
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
  typedef WaveCfg<NVT, KC, NC, NTR, WPE, SCHED, SPEC, HF, TRK, RK4, OBJ> C;
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
