"""Touch sensors and ground reaction forces of the MyoLeg step kernels against the float64 oracle (tests/touch_ref.py), N = 32 envs.

Tolerance: not invented.  The oracle's own float32 build, run on the same states, deviates from its float64 build by at most 4.8e-5
(nsub = 1) and 5.8e-5 (nsub = 5) on the MyoLeg model and 1.7e-2 on the terrain model (height-field prisms), relative to max(fn, 1 N);
the kernel reorders sums and uses rcp, so it is allowed 4 x that floor: 1.9e-4, 2.3e-4 and 6.8e-2.  The floor is measured again by each
run (touch_ref.f32_floor) and the figures are printed before they are asserted.  Envs whose contact count differs from the oracle's are
left out; at most 10 % of the envs may be.  Parity against MuJoCo itself stays unpinned, like all contact dynamics of this project.

More than 32 contacts: the flat-terrain test states themselves reach 45 contacts per env (a foot on the height field touches several
prisms), so the terrain routing test reads contacts 32.. from the env's overflow rows; no separate step-edge state was constructed.

The whole file runs once more against libmyo_hip_poison.so (last test): the epilogue reads the solver's row registers on lanes beyond
the contact count, and its result must not depend on what they held."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import touch_ref as T  # noqa: E402
from myosuite_mjx_amd import capi  # noqa: E402
from myosuite_mjx_amd import model as M  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEG, LEG_SPEC = "step_kernel_w<36,20,32,2,2,false,0,false>", "step_kernel_w<36,20,32,2,2,false,2,false>"
LEG_SPEC_SCHED = "step_kernel_w<36,20,32,2,2,true,2,false>"
TERRAIN_SPEC = "step_kernel_w<36,20,32,2,2,false,3,true>"


def run_hip(m, q, nsub, no_spec=False, sensors=True):
    """Step the test states `nsub` substeps from rest through the raw ABI; returns the batch (kept alive) and its read-outs."""
    old = os.environ.pop("MYO_NO_SPEC", None)
    try:
        if no_spec:
            os.environ["MYO_NO_SPEC"] = "1"      # read at model load: the run-time-sized instantiation
        hm = capi.HipModel(m.blob(), 0)
    finally:
        os.environ.pop("MYO_NO_SPEC", None)
        if old is not None:
            os.environ["MYO_NO_SPEC"] = old
    b = capi.HipBatch(hm, len(q))
    if sensors:
        b.enable_sensors()
    b.write(capi.F_QPOS, q.astype(np.float32))
    b.step(None, capi.ACTMAP_NONE, nsub)
    out = dict(ncon=b.read(capi.F_DIAG)[:, 1], kernel=b.last_kernel_name(), flags=b.status())
    if sensors:
        out["sens"] = b.read(capi.F_SENSORDATA).astype(np.float64)
        out["cfrc"] = b.read(capi.F_CFRC).astype(np.float64).reshape(len(q), -1, 3)
    return b, out


def compare(m, got, nsub, name="myolegs"):
    ref = T.oracle_outputs(m, nsub, name=name)
    floor = T.f32_floor(m, nsub, name)
    bound = 4 * floor
    same = got["ncon"] == ref["ncon"]
    worst = dict(sens=0.0, cfrc=0.0, total=0.0, total_qfc=0.0)
    for e in np.nonzero(same)[0]:
        scale = np.maximum(ref["sens"][e], 1.0)
        tscale = max(ref["sens"][e].sum(), np.linalg.norm(ref["cfrc"][e, -1]), 1.0)
        worst["sens"] = max(worst["sens"], (np.abs(got["sens"][e] - ref["sens"][e]) / scale).max())
        worst["cfrc"] = max(worst["cfrc"], (np.abs(got["cfrc"][e, :-1] - ref["cfrc"][e, :-1]) / scale[:, None]).max())
        worst["total"] = max(worst["total"], np.abs(got["cfrc"][e, -1] - ref["cfrc"][e, -1]).max() / tscale)
        worst["total_qfc"] = max(worst["total_qfc"], np.abs(got["cfrc"][e, -1] - ref["qfc"][e]).max() / tscale)
    print(f"\n{name} nsub={nsub} kernel={got['kernel']}: float32 floor {floor:.3e}, bound {bound:.3e}, envs left out {int((~same).sum())}, "
          f"max ncon {int(got['ncon'].max())}, worst " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert (got["flags"] & (capi.FLAG_BAD_STATE | capi.FLAG_BAD_QACC | capi.FLAG_CONTACT_OVERFLOW)).max() == 0
    assert (~same).sum() <= 0.1 * len(same)
    assert (ref["sens"][same] > 0).any(0).all()      # every sensor is exercised by the compared envs
    for k, v in worst.items():
        assert v <= bound, (k, v, bound)
    # a sensor the oracle reads as zero reads as zero here too (up to the bound, in newtons), and the other way round
    assert (np.abs(got["sens"][same][ref["sens"][same] == 0]) <= bound).all()


@pytest.mark.parametrize("nsub", [1, 5])
def test_raw_abi_matches_the_oracle(legs, nsub):
    """sensordata, the per-sensor forces and the total row, env by env; nsub = 5 catches reading a substep other than the last.  The total
    row also equals the oracle's qfrc_constraint[0:3] under the same bound."""
    _, got = run_hip(legs, T.states(legs), nsub)
    assert got["kernel"] == LEG_SPEC
    compare(legs, got, nsub)


def test_generic_routing(legs):
    _, got = run_hip(legs, T.states(legs), 1, no_spec=True)
    assert got["kernel"] == LEG
    compare(legs, got, 1)


def test_terrain_routing_and_the_overflow_rows(terrain):
    q = T.states(terrain, "myolegs_terrain")
    _, got = run_hip(terrain, q, 1)
    assert got["kernel"] == TERRAIN_SPEC
    assert got["ncon"].max() > 32      # contacts beyond the LDS table: point, normal and pair come from the env's overflow rows
    compare(terrain, got, 1, "myolegs_terrain")


SCHED_CHILD = """
import os, sys
sys.path.insert(0, {root!r}); sys.path.insert(0, os.path.join({root!r}, "tests"))
import numpy as np
import touch_ref as T
from test_gpu_touch import run_hip
from myosuite_mjx_amd import model as M
m = M.load_asset("myolegs")
q = np.concatenate([T.states(m), T.states(m)])      # the scheduler takes launches of 64 envs and more
_, got = run_hip(m, q, 5)
np.savez({out!r}, sens=got["sens"], cfrc=got["cfrc"], kernel=np.array(got["kernel"]))
"""


def test_scheduler_routing_gives_the_same_bits(legs, tmp_path):
    """The substep scheduler (one wave per (env, substep); only the wave of the last substep writes) against one wave per env.  The scheduler
    switch is read once per process, so the scheduled run is a child process."""
    out = str(tmp_path / "sched.npz")
    r = subprocess.run([sys.executable, "-c", SCHED_CHILD.format(root=ROOT, out=out)], cwd=ROOT, env=dict(os.environ, MYO_SCHED="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    s = np.load(out)
    assert str(s["kernel"]) == LEG_SPEC_SCHED
    q = np.concatenate([T.states(legs), T.states(legs)])
    _, got = run_hip(legs, q, 5)
    if not os.environ.get("MYO_SCHED"):
        assert got["kernel"] == LEG_SPEC
    assert s["sens"].tobytes() == got["sens"].tobytes() and s["cfrc"].tobytes() == got["cfrc"].tobytes()
    assert (got["sens"] > 0).any()


def test_sensors_off_changes_nothing():
    """State, obs and reward of a 10-step myoLegWalk-v0 rollout are bit-identical with sensors=True and sensors=False."""
    import myosuite_mjx_amd as myo
    import torch
    res = []
    for sensors in (False, True):
        env = myo.make("myoLegWalk-v0", num_envs=32, seed=7, sensors=sensors)
        env.reset(seed=7)
        g = torch.Generator().manual_seed(1)
        tr = []
        for _ in range(10):
            a = torch.rand((32, env.act_dim), generator=g) * 2 - 1
            obs, rew, done, trunc, _ = env.step(a)
            tr.append((obs.cpu().numpy().copy(), rew.cpu().numpy().copy(), env.batch.read(capi.F_QPOS), env.batch.read(capi.F_QVEL), env.batch.read(capi.F_ACT)))
        res.append(tr)
        if sensors:
            assert float(env.sensordata.max()) > 0
    for a, b in zip(*res):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()


def test_env_api():
    import myosuite_mjx_amd as myo
    import torch
    env = myo.make("myoLegWalk-v0", num_envs=32, sensors=True)
    assert env.sensor_names == ["r_foot", "r_toes", "l_foot", "l_toes"]
    env.reset(seed=3)
    sd, cf = env.sensordata, env.contact_force
    assert tuple(sd.shape) == (32, 4) and tuple(cf.shape) == (32, 5, 3)
    assert sd.data_ptr() == env.batch.field_ptr(capi.F_SENSORDATA)[0] and cf.data_ptr() == env.batch.field_ptr(capi.F_CFRC)[0]      # views, no copy
    assert float(sd.abs().max()) == 0 and float(cf.abs().max()) == 0      # nothing stepped yet
    a = torch.zeros((32, env.act_dim))
    for _ in range(3):
        env.step(a)
    assert float(env.sensordata.max()) > 0 and env.sensordata is sd
    np.testing.assert_array_equal(env.batch.read(capi.F_SENSORDATA), sd.cpu().numpy())
    # an env reset by autoreset reads zeros: force env 5 to the end of its episode
    el = env.view(capi.F_ELAPSED)
    el[5] = env.max_episode_steps
    env.step(a)
    assert int(el[5, 0]) == 0
    assert float(sd[5].abs().max()) == 0 and float(cf[5].abs().max()) == 0 and float(sd.max()) > 0
    # read-only fields, and no sensors without the kwarg
    with pytest.raises(capi.MyoError):
        env.batch.write(capi.F_SENSORDATA, np.zeros((32, 4), np.float32))
    plain = myo.make("myoLegWalk-v0", num_envs=4)
    with pytest.raises(AttributeError):
        plain.sensordata
    with pytest.raises(capi.MyoError):
        plain.batch.read(capi.F_SENSORDATA)
    for env_id in ("myoHandPoseRandom-v0", "MyoHandAirplaneFixed-v0"):
        with pytest.raises(NotImplementedError, match="sensors"):
            myo.make(env_id, num_envs=4, sensors=True)


def test_refusals_are_host_side(legs, hand):
    rk = capi.HipBatch(capi.HipModel(legs.with_integrator("RK4").blob(), 0), 4)
    with pytest.raises(capi.MyoError, match="-4.*RK4"):
        rk.enable_sensors()
    hb = capi.HipBatch(capi.HipModel(hand.blob(), 0), 4)
    with pytest.raises(capi.MyoError, match="-4.*hip_touch"):
        hb.enable_sensors()
    hm = capi.HipModel(legs.blob(), 0)
    assert hm.nsensor == 4 and capi.HipModel(hand.blob(), 0).nsensor == 0
    b = capi.HipBatch(hm, 4)
    with pytest.raises(capi.MyoError, match="-1"):
        b.read(capi.F_SENSORDATA)
    capi.set_lanes(32)
    try:
        with pytest.raises(capi.MyoError, match="-4.*lanes"):
            b.enable_sensors()
    finally:
        capi.set_lanes(64)
    b.enable_sensors()
    b.enable_sensors()
    assert b.read(capi.F_SENSORDATA).shape == (4, 4) and b.read(capi.F_CFRC).shape == (4, 15)


def test_sim_scene_sensor_access(legs):
    from myosuite_mjx_amd.sim import HipSimScene
    sim = HipSimScene("myolegs", num_envs=32, sensors=True)
    sim.data.qpos[:] = T.states(legs).astype(np.float32)
    sim.advance(substeps=1)
    ref = T.oracle_outputs(legs, 1)
    sd = sim.data.sensordata.cpu().numpy()
    assert sd.shape == (32, 4)
    r = sim.data.sensor("l_foot").data[0].cpu().numpy()      # the reference's sim.data.sensor(name).data[0], one value per env
    np.testing.assert_array_equal(r, sd[:, 2])
    assert np.abs(sd - ref["sens"]).max() <= 4 * T.f32_floor(legs, 1) * max(ref["sens"].max(), 1.0)


def test_the_file_passes_on_the_poisoned_build():
    if os.environ.get("MYO_HIP_LIB", "").endswith("libmyo_hip_poison.so"):
        return      # this IS the poisoned run
    lib = os.path.join(ROOT, "myosuite_mjx_amd", "libmyo_hip_poison.so")
    assert os.path.exists(lib), "libmyo_hip_poison.so is missing: run __graft_entry__.build()"
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_touch.py"], cwd=ROOT,
                       env=dict(os.environ, MYO_HIP_LIB=lib), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout
