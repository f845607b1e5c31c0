// myo_host_step.h -- the step launch: the table of step_kernel_w instantiations and the choice among them, launch_step in
// its pieces (lane choice and refusals, the substep scheduler's plan, the wave launch, the lanes launch), and the entry points that exist
// to time it: myo_bench_rollout, myo_bench_last_kernel_ms / _name, myo_probe_valu (include/myo_hip.h).
#ifndef MYO_HOST_STEP_H
#define MYO_HOST_STEP_H

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
  WK_TRK_OBJ
};
static const WaveKernel wave_kernels[] = {
#define X(id, name, ...) {name, step_kernel_w<__VA_ARGS__>},
  MYO_WAVE_KERNELS(X)
#undef X
  {"step_kernel_obj<36,20,32,2,2,false,0,false,true,false>", step_kernel_obj<36, 20, 32, 2, 2, false, 0, false, true, false>},   // WK_TRK_OBJ: the TRK kernel with the per-env object parameters (myo_host_objects.h)
};

// the instantiation a launch of model m runs: bm = the per-env body-mass override is on (only the run-time-sized instantiations read its
// link tables), sched = the substep scheduler is on (large-kernel models without RK4; terrain models only with their specialised sizes)
static WaveKernelId select_wave_kernel(const myo_model* m, bool bm, bool sched, bool obj = false) {
  const bool hand_sizes = m->hand_sizes && !bm, leg_sizes = m->leg_sizes && !bm;
  if (sched) return m->dw.hf.on ? WK_TERRAIN_SPEC_SCHED : (leg_sizes ? WK_LEG_SPEC_SCHED : WK_LEG_SCHED);
  if (m->rk4) return m->wave_cfg == 0 ? WK_HAND_RK4 : WK_LEG_RK4;
  if (m->wave_cfg == 2) return obj ? WK_TRK_OBJ : WK_TRK;   // TrackEnv model class (obj: the batch carries per-env object parameters)
  if (m->wave_cfg == 0) return hand_sizes ? WK_HAND_SPEC : WK_HAND;
  if (m->dw.hf.on) return m->terrain_sizes ? WK_TERRAIN_SPEC : WK_TERRAIN;   // terrain models: the instantiations with the height-field narrow phase
  return leg_sizes ? WK_LEG_SPEC : WK_LEG;
}

// Substep scheduler: MYO_SCHED=1 forces it, 0 disables it; default (auto) uses it where it was measured to pay: when the launch holds at
// least twice as many envs as the chip holds waves of this kernel (MyoLeg: 8 waves per CU; +6 % at 4096 envs).  With as many waves as envs
// every wave just re-takes its own env and only the overhead is left (MyoHand at 4096 envs: -15 %).  The plan of one launch: whether the
// scheduler runs, the grid, and the queue record every wave launch passes to its kernel
struct SchedPlan { bool on; int grid; SchedDev S; };
static SchedPlan sched_plan(const myo_batch* b, int nsub, bool walk, int kflags) {
  const myo_model* m = b->model;
  const int Bn = b->db.B, nsubtot = nsub + (walk ? 1 : 0);
  static const int sched_mode = [] { const char* e = getenv("MYO_SCHED"); return e ? atoi(e) : -1; }();   // process-wide configuration (environment)
  const int n_cu = m->n_cu > 0 ? m->n_cu : 256;                                                        // per model = per device
  const int resident = n_cu * (m->wave_cfg == 0 ? 16 : (m->wave_cfg == 1 ? 8 : std::max(1, (160 * 1024) / std::max(1, m->env_lds_bytes_w))));
  const bool sched_ok = !kflags && Bn >= 64 && Bn <= SCHED_ENV_MASK && nsubtot <= 15 && nsub > 0;
  const bool on = sched_ok && !b->bm_on && m->wave_cfg == 1 && !m->rk4 && !(m->dw.hf.on && !m->terrain_sizes) && (sched_mode == 1 || (sched_mode == -1 && Bn >= 2 * resident));
  // one queue per XCD the device (or its partition) shows: MI355X has 32 CUs per XCD, 8 XCDs in SPX mode (a queue keyed on
  // XCC_ID & 7 would never be drained on a DPX / QPX / CPX partition)
  const int nqueue = std::max(1, std::min(8, n_cu / 32));
  SchedPlan P{on, Bn, SchedDev{b->d_sched, b->d_sched + 32, nqueue == 8 ? b->sched_stride : (Bn + nqueue - 1) / nqueue + 1, nsubtot, nqueue}};
  if (on) {
    P.grid = Bn < resident ? Bn : resident;    // persistent waves: no more workgroups than the chip holds at once
    static const int grid_override = [] { const char* e = getenv("MYO_SCHED_GRID"); return e ? atoi(e) : 0; }();
    if (grid_override > 0 && grid_override < P.grid) P.grid = grid_override;
  }
  return P;
}

// one env per wavefront: step_kernel_w.  wk and kflags are null / 0 for every model outside the large-kernel class (the walk task needs
// wave_cfg == 1); the placement order is set only without the scheduler
static int launch_wave(myo_batch* b, const float* action, int actmap, int nsub, hipStream_t s, int kflags, const DevWalk* wk) {
  const myo_model* m = b->model;
  static OncePerDevice attr;
  int rc = set_lds_limit(attr, wave_kernels, 64 * 1024, m->device);
  if (rc) return rc;
  const int Bn = b->db.B;
  const SchedPlan P = sched_plan(b, nsub, wk != nullptr, kflags);
  const int* order = nullptr;
  if (b->balance && Bn >= 1024 && Bn % 4 == 0 && !kflags && !P.on) {
    static const int prio_mode = [] { const char* e = getenv("MYO_PRIO"); return e ? atoi(e) : 2; }();
    hipLaunchKernelGGL(balance_kernel, dim3(1), dim3(1024), 0, s, (const int*)b->db.diag, Bn, b->d_order, Bn / 4, prio_mode);
    order = b->d_order;
  }
  const WaveKernel& k = wave_kernels[select_wave_kernel(m, b->bm_on, P.on, b->obj_on)];
  if (!kflags) b->last_kernel = k.name;
  if (P.on) hipLaunchKernelGGL(sched_init_kernel, dim3(1), dim3(1024), 0, s, (const int*)b->db.diag, Bn, P.S);
  hipLaunchKernelGGL(k.fn, dim3(P.grid), dim3(64), (size_t)m->env_lds_bytes_w, s, (const DevModel*)m->d_dm, (const DevModelW*)m->d_dw, b->db, action, actmap,
                     nsub, b->d_stamps, order, wk, kflags, P.S);
  HIPCHK(hipGetLastError());
  // walk task with the term row on: the row and MYO_F_REWARD of every launch whose fused pass wrote the reward
  if (wk && b->db.rwd && !(kflags & KF_OBS_ONLY)) { if ((rc = walk_terms_launch(b, s))) return rc; }
  // ... and with the observation-term rows on, those rows of every launch: each of them wrote MYO_F_OBS
  if (wk && b->obs_terms.terms) return obs_terms_launch(b, s);
  return MYO_OK;
}

// G = 16 / 32 / 64 lanes per env, 64 / G envs per wavefront: step_kernel<G>
static int launch_lanes(myo_batch* b, int G, const float* action, int actmap, int nsub, hipStream_t s) {
  const myo_model* m = b->model;
  const int EPW = 64 / G, grid = (b->db.B + EPW - 1) / EPW;
  const size_t lds = (size_t)EPW * m->env_lds_bytes;
  if (G == 16) hipLaunchKernelGGL(step_kernel<16>, dim3(grid), dim3(64), lds, s, m->dm, b->db, action, actmap, nsub, b->d_stamps);
  else if (G == 32) hipLaunchKernelGGL(step_kernel<32>, dim3(grid), dim3(64), lds, s, m->dm, b->db, action, actmap, nsub, b->d_stamps);
  else hipLaunchKernelGGL(step_kernel<64>, dim3(grid), dim3(64), lds, s, m->dm, b->db, action, actmap, nsub, b->d_stamps);
  HIPCHK(hipGetLastError());
  return MYO_OK;
}

// (prototype with the default argument: myo_host.h)
static int launch_step(myo_batch* b, const float* action, int actmap, int nsub, hipStream_t s, int kflags) {
  const myo_model* m = b->model;
  const DevWalk* wk = b->task.task == MYO_TASK_WALK ? b->d_walk : nullptr;
  if (kflags && !(wk && g_lanes == 64)) return fail(MYO_E_ARG, "observation pass: walk task on the wave kernel only");
  // models the wave kernel cannot take fall back to 16 lanes; models only the wave kernel can take always use it
  const int G = (g_lanes == 64 && !m->wave_ok) ? 16 : ((g_lanes != 64 && !m->generic_ok) ? 64 : g_lanes);
  const bool wave = G == 64 && m->wave_ok;
  // the lanes kernels and the reach observation kernel (which a reach batch launches on its own) get their limit whichever kernel steps
  static OncePerDevice attr;
  static const struct { const void* fn; } lanes_kernels[] = {{(const void*)step_kernel<16>}, {(const void*)step_kernel<32>}, {(const void*)step_kernel<64>}, {(const void*)reach_obs_kernel<16>}};
  int rc = set_lds_limit(attr, lanes_kernels, 160 * 1024, m->device);
  if (rc) return rc;
#if MYO_POISON
  {  // MYO_POISON_MODE (diagnostic build only): bit 0 scratch memory, bit 1 vector registers, bit 2 scalar registers; default all
    static const int pmode = [] { const char* e = getenv("MYO_POISON_MODE"); return e ? atoi(e) : 7; }();
    if (pmode & 1) hipLaunchKernelGGL(scratch_poison_kernel, dim3(16384), dim3(64), 0, s, (float*)b->d_stamps, 0);
    if (pmode & 2) hipLaunchKernelGGL(vgpr_poison_kernel, dim3(8192), dim3(64), 0, s, 0x7fc0dead);
    if (pmode & 4) hipLaunchKernelGGL(sgpr_poison_kernel, dim3(32768), dim3(64), 0, s);
  }
#endif
  if (!wave && !m->generic_ok)
    return fail(MYO_E_UNSUPPORTED, "this model (tendon limits / free joint / equalities / plane contacts) needs the wave-per-env kernel (lanes = 64)");
  if (b->sens_on && (rc = sens_check(b))) return rc;   // (lanes may have changed since the sensors were enabled)
  // per-env body masses: link tables of every env recomposed once per launch; the step runs on the run-time-sizes instantiation of the
  // model's class (the only ones that read them)
  if (b->bm_on) {
    if ((rc = bm_check(b))) return rc;
    const int n = b->db.B * m->dm.nl;
    hipLaunchKernelGGL(link_compose_kernel, dim3((n + 255) / 256), dim3(256), 0, s, b->db, m->dm.nl, m->d_lm_adr, m->d_lm_body, m->d_lm_tab);
  }
  // per-env object parameters: the rows the TRK kernel reads, composed from the batch's tables once per launch
  if ((rc = obj_compose(b, s))) return rc;
  return wave ? launch_wave(b, action, actmap, nsub, s, kflags, wk) : launch_lanes(b, G, action, actmap, nsub, s);
}

// HIP-event milliseconds of the first n step-kernel event pairs, into last_kernel_ms
static int sum_kernel_ms(myo_batch* b, int n) {
  float tot = 0.f;
  for (int i = 0; i < n; i++) { float t; HIPCHK(hipEventElapsedTime(&t, b->kev[2 * i], b->kev[2 * i + 1])); tot += t; }
  b->last_kernel_ms = tot;
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
  return sum_kernel_ms(b, steps);
}

const char* myo_bench_last_kernel_name(const myo_batch* b) { return b ? b->last_kernel : ""; }

/* total HIP-event milliseconds spent in the step kernel launches of the last synchronous myo_bench_rollout call, or -- after
 * asynchronous calls (ms_out == NULL) -- of all launches enqueued since the last collection (waits for them) */
int myo_bench_last_kernel_ms(myo_batch* b, float* ms_out) {
  if (!b || !ms_out) return fail(MYO_E_ARG, "null");
  if (b->kev_pending > 0) {
    HIPCHK(hipSetDevice(b->model->device));
    HIPCHK(hipEventSynchronize(b->kev[2 * b->kev_pending - 1]));
    if (const int rc = sum_kernel_ms(b, b->kev_pending)) return rc;
    b->kev_pending = 0;
  }
  *ms_out = b->last_kernel_ms;
  return MYO_OK;
}

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

#endif  // MYO_HOST_STEP_H
