"""Developer probe (diagnostic build, -DMYO_STAMPS=1): where a substep spends its cycles, per lanes-per-env setting."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
# MYO_STAMPS_LIB: another stamps build of the same sources (A/B: e.g. one compiled with MYO_HIPCC_EXTRA=-DMYO_LDL_MFMA=0)
os.environ["MYO_HIP_LIB"] = os.environ.get("MYO_STAMPS_LIB") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "myosuite_mjx_amd", "libmyo_hip_stamps.so")
from myosuite_mjx_amd import capi
from myosuite_mjx_amd.envs import BatchedMyoEnv

B = int(os.environ.get("B", 4096))
NAMES = ["load/check", "kinematics", "tendon+muscle", "dynamics(CRB/RNE)", "collision (wave kernel: narrow phase)", "constraint rows", "wave kernel: geom frames + broad phase", "newton", "euler", "store"]
ENV = os.environ.get("ENV", "myoHandPoseRandom-v0")
env = BatchedMyoEnv(ENV, num_envs=B, as_torch=False)
mode = capi.BENCH_OBS | capi.BENCH_FRESH_ACTIONS | capi.BENCH_AUTORESET
for lanes, bal in ((64, 0), (64, 1)):
    capi.set_lanes(lanes)
    env.batch.set_balance(bal)
    env.reset(seed=1)
    env.batch.bench_rollout(30, 10, 0, mode, env.max_episode_steps, None)
    ms = env.batch.bench_rollout(10, 10, 0, 0, 0, None) / 10
    nwg = B // (64 // lanes)
    st3, ok = capi.read_stamps(env.batch, 3 * nwg)      # second third: finer split of tendon / dynamics / Newton; last third: factorisations (wave kernel only)
    st, sub, xs = st3[:nwg], st3[nwg:2 * nwg], st3[2 * nwg:]
    tot = st[:, :10].sum(1)          # columns 10, 11 hold hardware ids, not cycles
    print(f"== lanes/env {lanes} balance {bal}: step kernel {ms:.3f} ms per env-step ({B/ms*1e3:,.0f} env-steps/s); per-WG total cycles mean {tot.mean():,.0f} max {tot.max():,.0f} (10 substeps)")
    for k, n in enumerate(NAMES):
        print(f"   {n:26s} {st[:,k].mean()/10:12,.0f} cycles/substep  {100*st[:,k].mean()/tot.mean():5.1f}%")
    SUBN = ["newton: forces, cost, gradient, convergence test", "newton: Hessian assembly", "newton+euler: other factorisations / reload L", "newton+euler: triangular solves",
            "newton: M*search, J*search", "newton: line search", "newton: start (M*warm, J*warm)", "tendons: site / geom frames + wrap geometry", "tendons: moment arms of the straight pieces", "tendons: gather + muscle",
            "dynamics: cinert, cdof", "dynamics: RNE forward / backward, M assembly"]
    for k, n in enumerate(SUBN):
        if n != "-":
            print(f"      {n:52s} {sub[:,k].mean()/10:12,.0f} cycles/substep  {100*sub[:,k].mean()/tot.mean():5.1f}%")
    # split out of "build rows, Cholesky, store L": the dense Newton refactor (phase 0) and the tree-sparse M / M + h D factorisations
    for k, n in ((0, "newton: dense refactor (ldl, store L, reload)"), (1, "unconstr.+euler: tree-sparse M / M + hD factor.")):
        print(f"      {n:52s} {xs[:,k].mean()/10:12,.0f} cycles/substep  {100*xs[:,k].mean()/tot.mean():5.1f}%")
    nf = xs[:, 2] / 10.0
    heavy = int(np.argmax(tot))
    print(f"      dense Newton refactors per substep: mean {nf.mean():.2f}, max {nf.max():.2f}, heaviest WG {nf[heavy]:.2f}; cycles per refactor {xs[:,0].sum()/max(1,xs[:,2].sum()):,.0f}")
