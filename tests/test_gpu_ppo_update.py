"""GPU tests (pytest -m gpu) of the device learner (myo_ppo_learner_*, include/myo_hip_ppo.h; ppo.Learner; ppo.train(update="hip")): its
gradients against float64 autograd of tests/ppo_update_ref.py, its Adam against a float64 Adam fed with the learner's own gradients, bit
determinism, refusals, the wiring into ppo.train, and the first three once more on the LDS-poisoned build.

The gradient bound is not picked by hand: the same step stated in float32 torch on the CPU is compared with float64 on the very inputs of the
test, and the learner may be off by 4x that (the MFMA sums a k-ordered fmaf chain where torch sums in blocks, and dW sums over up to 2 368
rows).  Both figures are max |g - g64| / max |g64| per tensor, then the worst over all tensors; per case they are the worst of the case's
three steps.  Measured figures: profiles/ppo_update.md."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ppo_update_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DEFAULT_P, DEFAULT_V = (32, 32, 32, 32), (256,) * 5
# (T, mb, obs_dim, act_dim, policy_hidden, value_hidden), seed.  The seed of each case is the smallest one at which each of its three
# minibatches, in float64 at the initial parameters, keeps rho more than 1e-3 away from the clip edges and has 2 % to 50 % of its samples
# outside the clip range (the last case, one sample, is exempt: its normalised advantage is 0 and only the entropy term drives the policy).
CASES = {
    "tiny": ((3, 5, 7, 1, (32,), (256,)), 1),
    "hand": ((2, 33, 70, 6, DEFAULT_P, DEFAULT_V), 4),
    "wide": ((8, 37, 108, 39, DEFAULT_P, DEFAULT_V), 7),
    "ragged": ((5, 64, 33, 3, (17, 40), (100, 9)), 0),
    "one": ((1, 1, 7, 1, (32,), (256,)), 0),
}


def _flat(groups):
    return [a for group in groups for a in group]


def _read(learner, which):
    return tuple([a.cpu().numpy().copy() for a in group] for group in learner.tensors(which))


def _run(name):
    """Three steps of two learners on one case; everything the tests below look at, computed once."""
    import torch
    from myosuite_mjx_amd import ppo
    shape, seed = CASES[name]
    case = R.make_case(*shape, seed=seed)
    T, mb = case["T"], case["mb"]
    dev = {k: torch.as_tensor(case[k], device="cuda") for k in ("obs", "u", "logp", "rewards", "termination", "truncation", "mean", "std")}
    make = lambda: ppo.Learner(case["obs_dim"], case["act_dim"], *case["params"], T, mb, learning_rate=R.LR, **R.HYPER)
    a, b = make(), make()
    adam = R.Adam64(_flat(case["params"]))
    steps = []
    for k in range(3):
        idx, noise = torch.as_tensor(case["idx"][k], device="cuda"), torch.as_tensor(case["noise"][k], device="cuda")
        before = _read(a, "param")
        sums = [torch.zeros(3, device="cuda") for _ in range(2)]
        for learner, s in zip((a, b), sums):
            learner.step(dev["obs"], dev["u"], dev["logp"], dev["rewards"], dev["termination"], dev["truncation"], idx, dev["mean"], dev["std"],
                         noise, s)
        torch.cuda.synchronize()
        grads = _read(a, "grad")
        g64, l64, rho, adv = R.gradients(before, case, case["idx"][k], case["noise"][k])
        g32, _, _, _ = R.gradients(before, case, case["idx"][k], case["noise"][k], dtype=torch.float32)
        adam.step(_flat(grads))
        steps.append(dict(grads=grads, g64=g64, l64=l64, clip=R.clip_figures(rho, adv), e32=R.gradient_error(g32, g64),
                          err=R.gradient_error(grads, g64), sums=[s.cpu().numpy() for s in sums],
                          after=[{w: _read(l, w) for w in ("param", "m", "v")} for l in (a, b)],
                          adam=dict(p=[p.copy() for p in adam.p], m=[m.copy() for m in adam.m], v=[v.copy() for v in adam.v])))
    return steps


_RUNS = {}


@pytest.fixture
def run(request):
    name = request.param
    if name not in _RUNS:
        _RUNS[name] = _run(name)
    return name, _RUNS[name]


by_case = pytest.mark.parametrize("run", list(CASES), indirect=True)


@by_case
def test_gradients_match_float64(run):
    """Every entry of every gradient tensor, three steps in a row at the learner's own parameters.  Bound: 4 x the float32 CPU torch
    statement's error on the same inputs (module docstring).  The loss terms agree with float64 to 1e-5 max(1, |term|)."""
    name, steps = run
    for k, s in enumerate(steps):
        print(f"{name} step {k}: rho to clip edge {s['clip'][0]:.2e}, clipped share {s['clip'][1]:.3f}, float32 torch {s['e32']:.3e}, "
              f"learner {s['err']:.3e}, ratio {s['err'] / s['e32']:.2f}, losses {s['sums'][0]} float64 {s['l64']}")
    if name != "one":
        for s in steps:
            assert s["clip"][0] > 1e-4 and 0.02 <= s["clip"][1] <= 0.5, s["clip"]
    for s in steps:
        assert all(np.isfinite(g).all() for g in _flat(s["grads"]))
        for got, want in zip(s["sums"][0], s["l64"]):
            assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (s["sums"][0], s["l64"])
    e32, err = max(s["e32"] for s in steps), max(s["err"] for s in steps)
    print(f"{name}: float32 torch {e32:.3e}, learner {err:.3e}, ratio {err / e32:.2f}")
    assert err <= 4 * e32


@by_case
def test_adam_matches_float64_on_the_learners_gradients(run):
    """A float64 Adam fed with the gradients read back from the learner: after step k every parameter is within k float32 ulps of itself
    plus 1e-5 lr of the float64 one, and the moments agree to 1e-6 of their tensor's largest entry."""
    name, steps = run
    for k, s in enumerate(steps, start=1):
        got = s["after"][0]
        for p, m, v, p64, m64, v64 in zip(_flat(got["param"]), _flat(got["m"]), _flat(got["v"]), s["adam"]["p"], s["adam"]["m"], s["adam"]["v"]):
            assert (np.abs(p - p64) <= k * np.spacing(np.abs(p)) + 1e-5 * R.LR).all(), (name, k, float(np.abs(p - p64).max()))
            assert np.abs(m - m64).max() <= 1e-6 * np.abs(m64).max(), (name, k)
            assert np.abs(v - v64).max() <= 1e-6 * np.abs(v64).max(), (name, k)


@by_case
def test_two_learners_end_bit_identical(run):
    name, steps = run
    for s in steps:
        a, b = s["after"]
        for w in ("param", "m", "v"):
            for x, y in zip(_flat(a[w]), _flat(b[w])):
                assert np.array_equal(x, y), (name, w)
        assert np.array_equal(s["sums"][0], s["sums"][1]), name
    assert not np.array_equal(_flat(steps[0]["after"][0]["param"])[0], _flat(steps[2]["after"][0]["param"])[0])


def test_refusals_launch_nothing():
    """MYO_E_ARG (-1): T > max_unroll, mb > max_minibatch, a NULL tensor.  MYO_E_UNSUPPORTED (-4): a layer 513 wide, nine layers.  The
    learner's parameters are the same bits afterwards."""
    import torch
    from myosuite_mjx_amd import capi, ppo
    case = R.make_case(*CASES["tiny"][0], seed=1)
    T, mb, B = case["T"], case["mb"], case["B"]
    learner = ppo.Learner(case["obs_dim"], case["act_dim"], *case["params"], T, mb, **R.HYPER)
    before = _read(learner, "param")
    d = {k: torch.as_tensor(case[k], device="cuda") for k in ("obs", "u", "logp", "rewards", "termination", "truncation", "mean", "std")}
    idx, noise = torch.as_tensor(case["idx"][0], device="cuda"), torch.as_tensor(case["noise"][0], device="cuda")
    args = [d["obs"], d["u"], d["logp"], d["rewards"], d["termination"], d["truncation"], idx, d["mean"], d["std"], noise]
    assert learner.step_rc(*args, T=T + 1, mb=mb) == -1
    assert learner.step_rc(*args, T=T, mb=mb + 1) == -1
    for hole in (0, 6, 9):                                      # obs, idx, the entropy noise
        assert learner.step_rc(*[None if i == hole else a for i, a in enumerate(args)], T=T, mb=mb) == -1
    pw, pb, vw, vb = ppo.init_networks(7, 1, (513,), (16,), 0)
    with pytest.raises(capi.MyoError, match="error -4"):
        ppo.Learner(7, 1, pw, pb, vw, vb, T, mb)
    pw, pb, vw, vb = ppo.init_networks(7, 1, (8,) * 8, (16,), 0)
    with pytest.raises(capi.MyoError, match="error -4"):
        ppo.Learner(7, 1, pw, pb, vw, vb, T, mb)
    torch.cuda.synchronize()
    for x, y in zip(_flat(before), _flat(_read(learner, "param"))):
        assert np.array_equal(x, y)
    assert B == 2 * mb + 1


ENV_ID, NUM_ENVS = "myoElbowPose1D6MFixed-v0", 64


def test_train_first_iteration_agrees_with_the_torch_update():
    """One iteration of one SGD step in each update mode from one seed: the rollouts are bit-equal, the reported losses are those of the
    shared initial parameters, and Adam's first step moves no parameter by more than lr."""
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import ppo
    lr, out = 3e-4, {}
    for update in ("torch", "hip"):
        env = myo.make(ENV_ID, num_envs=NUM_ENVS)
        out[update] = ppo.train(env, NUM_ENVS * 8, unroll_length=8, num_minibatches=1, num_updates_per_batch=1, seed=5, learning_rate=lr,
                                keep_first_rollout=True, update=update)
    (_, pt, mt), (_, ph, mh) = out["torch"], out["hip"]
    for k in ("obs", "u", "logp", "reward"):
        assert np.array_equal(mt[0]["first_rollout"][k], mh[0]["first_rollout"][k]), k
    for k in ("policy_loss", "value_loss", "entropy_loss"):
        print(k, mt[0][k], mh[0][k])
        assert abs(mt[0][k] - mh[0][k]) <= 1e-5 * max(1.0, abs(mt[0][k])), k
    init = ppo.init_networks(env.obs_dim, env.act_dim, (32, 32, 32, 32), (256,) * 5, 5)
    moved = 0.0
    for prefix, group in zip(("w", "b", "vw", "vb"), init):
        for i, p0 in enumerate(group):
            moved = max(moved, float(np.abs(ph[f"{prefix}{i}"] - p0.detach().numpy()).max()))
    assert 0.0 < moved <= lr * (1 + 1e-3), moved


TRAIN_KW = dict(unroll_length=8, num_minibatches=4, num_updates_per_batch=2, seed=5, keep_first_rollout=True)


def test_train_two_iterations_with_the_hip_update(tmp_path):
    import torch
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import ppo
    from myosuite_mjx_amd.policy import BraxPolicy
    env_id, num_envs = ENV_ID, NUM_ENVS
    env = myo.make(env_id, num_envs=num_envs)
    seen = []
    pol, params, metrics = ppo.train(env, 2 * num_envs * 8, progress_fn=lambda n, m: seen.append(n), update="hip", **TRAIN_KW)
    assert seen == [num_envs * 8, 2 * num_envs * 8] and len(metrics) == 2
    assert (env.status() == 0).all()
    assert float(params["obs_count"]) == 2 * num_envs * 8
    # all parameters are finite and have changed
    init = ppo.init_networks(env.obs_dim, env.act_dim, (32, 32, 32, 32), (256,) * 5, TRAIN_KW["seed"])
    n = 5
    for prefix, group in zip(("w", "b", "vw", "vb"), init):
        for i, p0 in enumerate(group):
            p = params[f"{prefix}{i}"]
            assert p.shape == tuple(p0.shape) and np.isfinite(p).all() and not np.array_equal(p, p0.detach().numpy()), (prefix, i)
    assert np.isfinite(params["obs_mean"]).all() and np.isfinite(params["obs_std"]).all() and (params["obs_std"] > 0).all()
    assert all(np.isfinite(m[k]) for m in metrics for k in ("policy_loss", "value_loss", "entropy_loss", "steps_per_s"))
    # the saved .npz loads with BraxPolicy.from_npz and acts like the torch network; so does the policy train() kept up to date on the device
    path = tmp_path / "policy.npz"
    ppo.save(path, params)
    loaded = BraxPolicy.from_npz(str(path))
    assert (loaded.obs_dim, loaded.act_dim) == (env.obs_dim, env.act_dim)
    obs = torch.as_tensor(metrics[0]["first_rollout"]["obs"][3], device="cuda").contiguous()
    a1, a2 = torch.empty((num_envs, env.act_dim), device="cuda"), torch.empty((num_envs, env.act_dim), device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    loaded.act(obs.data_ptr(), num_envs, a1.data_ptr(), deterministic=True, stream=st)
    pol.act(obs.data_ptr(), num_envs, a2.data_ptr(), deterministic=True, stream=st)
    t = {k: torch.as_tensor(v, device="cuda") for k, v in params.items()}
    loc, _ = ppo.policy_forward(obs, t["obs_mean"], t["obs_std"], [t[f"w{i}"] for i in range(n)], [t[f"b{i}"] for i in range(n)])
    torch.cuda.synchronize()
    assert float((a1 - torch.tanh(loc)).abs().max()) < 2e-5
    assert torch.equal(a1, a2)


def test_gradients_adam_and_determinism_on_the_poisoned_build():
    """Tests 1-3 of this file against the -DMYO_POISON=1 build, where every new kernel first fills the LDS it declares with NaN bits: a read
    of a word the launch never wrote shows up in the gradients.  A child process, because the library is chosen when it is first loaded."""
    lib = os.path.join(ROOT, "myosuite_mjx_amd", "libmyo_hip_poison.so")
    assert os.path.exists(lib), "libmyo_hip_poison.so is missing: run __graft_entry__.build()"
    env = dict(os.environ, MYO_HIP_LIB=lib)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "tests/test_gpu_ppo_update.py", "-k",
                        "test_gradients_match_float64 or test_adam_matches or test_two_learners"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "15 passed" in r.stdout, r.stdout[-500:]
