"""Golden fixture of the classic gym TrackEnv (envs/myo/myodm/myodm_v0.py), generated FROM THE REFERENCE in the build container only.

The reference module is imported *by file path*, as tools/make_ref_fixtures.py does.  MuJoCo and gym are absent here, so small stand-in
modules take the place of `myosuite.envs.myo.base_v0` (BaseV0: only what TrackEnv._setup and the reward read) and `myosuite.utils.gym`;
`myosuite.logger.reference_motion`, `myosuite.utils.quat_math` and `myosuite.envs.obs_vec_dict` are the reference's own modules.  The
reference's TrackEnv._setup, get_obs_dict, get_reward_dict and check_termination then run on a stand-in `self` / `sim` that holds recorded
states: qpos, qvel, act, time and the object / wrist (lunate) body frames xipos / ximat, computed by this repository's float64 oracle
(oracle/) at those qpos -- the post-step kinematics the reference reads after update_reference_insim's sim.forward().

    python tools/make_myodm_classic_fixture.py      # writes tests/golden/myodm_classic.npz

Three references: the airplane Fixed and Random ids' registered references and the airplane fly1 motion (tests/golden/ref_motion.npz).
Recorded per case: the inputs, the reference row get_reference returned (RANDOM draws come from the reference's generator), the obs
vector (obsdict2obsvec), the reward dict and check_termination, plus _setup's init_qpos and _lift_z."""
import importlib.util
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MYO_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden", "myodm_classic.npz")
sys.path.insert(0, ROOT)


def _load(rel, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _reference_trackenv():
    """myodm_v0.TrackEnv with the stand-ins in place of the modules that need MuJoCo / gym."""
    for name in ("myosuite", "myosuite.envs", "myosuite.envs.myo", "myosuite.logger", "myosuite.utils"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["myosuite.utils.quat_math"] = _load("myosuite/utils/quat_math.py", "myosuite.utils.quat_math")
    sys.modules["myosuite.logger.reference_motion"] = _load("myosuite/logger/reference_motion.py", "myosuite.logger.reference_motion")
    ov = _load("myosuite/envs/obs_vec_dict.py", "myosuite.envs.obs_vec_dict")

    class BaseV0(ov.ObsVecDict):
        """Stand-in for BaseV0 / MujocoEnv: _setup keeps what get_obs_dict / get_reward_dict read.  The observation keys get `act` appended
        as base_v0.py:34-38 does; init_qpos starts as the sim's qpos (env_base.py:115-139; TrackEnv._setup then overwrites every entry)."""

        def _setup(self, obs_keys, weighted_reward_keys, frame_skip=10, **kwargs):
            if self.sim.model.na > 0 and "act" not in obs_keys:
                obs_keys = obs_keys.copy()
                obs_keys.append("act")
            self.obs_keys, self.rwd_keys_wt, self.frame_skip = obs_keys, weighted_reward_keys, frame_skip
            self.init_qpos = self.sim.data.qpos.ravel().copy()
            self.init_qvel = self.sim.data.qvel.ravel().copy()

    base = types.ModuleType("myosuite.envs.myo.base_v0")
    base.BaseV0 = BaseV0
    sys.modules["myosuite.envs.myo.base_v0"] = base
    gym = types.ModuleType("myosuite.utils.gym")
    sys.modules["myosuite.utils"].gym = gym
    sys.modules["myosuite.utils.gym"] = gym
    return _load("myosuite/envs/myo/myodm/myodm_v0.py", "ref_myodm_v0").TrackEnv, ov


class _Sim:
    """Stand-in MjSim: names from the compiled model, data rows set per recorded state; forward() is a no-op (the frames are recorded)."""

    def __init__(self, m):
        self.model = types.SimpleNamespace(
            na=m.n_muscle, site_pos=np.zeros((8, 3)), geom_rgba=np.ones((len(m.names["geom"]), 4)),
            site_name2id=lambda n: 0, body_name2id=lambda n: m.name2id("body", n), geom_name2id=lambda n: 0)
        self.data = types.SimpleNamespace(qpos=np.zeros(m.nq), qvel=np.zeros(m.nv), act=np.zeros(m.n_muscle), time=0.0,
                                          xipos=np.zeros((m.nbody, 3)), ximat=np.zeros((m.nbody, 9)))

    def forward(self):
        pass


def _states(m, ref_robot, ref_object, n, seed):
    """n post-step-like states around a reference pose: hand + arm near the reference (with noise), the object near its target, random
    velocities and muscle activations; the body frames from the oracle at that qpos."""
    from myosuite_mjx_amd import track as T
    from oracle.oracle import Oracle
    rng = np.random.default_rng(seed)
    o = Oracle(m.blob())
    out = dict(qpos=np.zeros((n, m.nq)), qvel=rng.normal(0, 0.3, (n, m.nv)), act=rng.uniform(0, 1, (n, m.n_muscle)),
               xipos=np.zeros((n, m.nbody, 3)), ximat=np.zeros((n, m.nbody, 9)))
    for i in range(n):
        r, ob = ref_robot[i % len(ref_robot)], ref_object[i % len(ref_object)]
        q = np.zeros(m.nq)
        q[:29] = r + rng.normal(0, 0.05 if i % 3 else 0.4, 29)
        far = 0.3 if i % 5 == 4 else 0.02                      # every fifth state: object far from its target (terminates)
        q[29:32] = ob[:3] + rng.normal(0, far, 3)
        q[32:35] = T.quat2euler(ob[3:]) + rng.normal(0, 0.3, 3)
        o.reset()
        o.set_state(qpos=q, qvel=np.zeros(m.nv))
        o.forward()
        out["qpos"][i] = q
        out["xipos"][i] = o.field("xipos").reshape(-1, 3)
        out["ximat"][i] = o.field("ximat").reshape(-1, 9)
    return out


def main():
    from myosuite_mjx_amd import envs, model as M
    TrackEnv, ov = _reference_trackenv()
    m = M.load_asset("myohand_object_airplane")
    f = np.load(os.path.join(ROOT, "tests", "golden", "ref_motion.npz"))
    motion = {k.split("__in__")[1]: f[k] for k in f.files if k.startswith("track_MyoHand_airplane_fly1__in__")}
    cases = [("fixed", envs.REGISTRY["MyoHandAirplaneFixed-v0"]["reference"], 0.0, [0.0, 0.02, 0.5, 1.0]),
             ("random", envs.REGISTRY["MyoHandAirplaneRandom-v0"]["reference"], 0.0, [0.0, 0.02, 0.04, 0.6]),
             ("track", motion, 0.0, [0.0, 0.02, 0.04, 0.1, 0.5, 0.98, 1.5, 1.98, 2.5]),
             ("trackmid", motion, 0.01, [0.0, 0.02, 0.3, 1.0])]       # motion_start_time 0.01: between-frame lookups
    out = {}
    ob_id, wr_id = m.name2id("body", "airplane"), m.name2id("body", "lunate")
    from oracle.oracle import Oracle
    o = Oracle(m.blob())
    o.reset()
    o.forward()
    xipos0 = o.field("xipos").reshape(-1, 3).copy()                      # _setup reads the object's xipos at qpos0 (:154)
    for name, reference, t0, times in cases:
        for term_pose in (False, True):
            sim = _Sim(m)
            sim.data.qpos[:] = np.asarray(m.qpos0, float)
            sim.data.xipos[:] = xipos0
            env = TrackEnv.__new__(TrackEnv)
            ov.ObsVecDict.__init__(env)
            env.sim = env.sim_obsd = sim
            env.object_name = "airplane"
            env.np_random = np.random.default_rng(11)
            env.initialized_pos = False
            env._setup(reference=reference, motion_start_time=t0, Termimate_pose_fail=term_pose)
            key = f"{name}_{'pose' if term_pose else 'obj'}"
            R = env.ref.reference
            st = _states(m, np.atleast_2d(R["robot"]), np.atleast_2d(R["object"]), len(times) * 2, seed=len(out))
            drawn = dict(robot=[], robot_vel=[], object=[])
            get = env.ref.get_reference

            def record(t, get=get, drawn=drawn):
                r = get(t)
                for k in drawn:
                    v = getattr(r, k)
                    drawn[k].append(np.zeros(0) if v is None else np.asarray(v, float).copy())
                return r
            env.ref.get_reference = record
            obs, rwd, term = [], {k: [] for k in ("pose", "object", "bonus", "penalty", "sparse", "solved", "done", "dense")}, []
            tt = np.repeat(np.asarray(times, float), 2)
            for i, t in enumerate(tt):
                sim.data.qpos[:], sim.data.qvel[:], sim.data.act[:], sim.data.time = st["qpos"][i], st["qvel"][i], st["act"][i], float(t)
                sim.data.xipos[:], sim.data.ximat[:] = st["xipos"][i], st["ximat"][i]
                od = env.get_obs_dict(sim)
                _, vec = env.obsdict2obsvec(od, env.obs_keys)
                env.expand_dims(od)                                  # as MujocoEnv._forward does before get_reward_dict
                rd = env.get_reward_dict(od)
                obs.append(vec)
                term.append(bool(env.check_termination(od)))
                for k in rwd:
                    rwd[k].append(float(np.asarray(rd[k]).ravel()[0]))
            out.update({f"{key}__time": tt, f"{key}__motion_start_time": np.float64(t0), f"{key}__init_qpos": env.init_qpos.copy(),
                        f"{key}__lift_z": np.float64(env._lift_z), f"{key}__obs": np.stack(obs), f"{key}__terminate": np.array(term),
                        f"{key}__obs_keys": np.array(env.obs_keys)})
            for k in ("qpos", "qvel", "act"):
                out[f"{key}__{k}"] = st[k]
            out[f"{key}__obj_xipos"], out[f"{key}__obj_ximat"] = st["xipos"][:, ob_id], st["ximat"][:, ob_id]
            out[f"{key}__wrist_xipos"] = st["xipos"][:, wr_id]
            for k, v in drawn.items():
                out[f"{key}__ref_{k}"] = np.stack(v)
            for k, v in rwd.items():
                out[f"{key}__rwd_{k}"] = np.array(v)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes, {len(out)} arrays)")


if __name__ == "__main__":
    main()
