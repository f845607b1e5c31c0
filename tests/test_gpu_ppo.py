"""GPU tests (pytest -m gpu) of the device side of PPO training (include/myo_hip_ppo.h, myosuite_mjx_amd/ppo.py): myo_policy_sample and
myo_ppo_gae against the float64 statements of tests/ppo_ref.py, myo_policy_update, and two iterations of ppo.train on a pose id and on a
MyoDM id.  No claim about learning is made here: tests/test_ppo_host.py holds the learning check, on the torch path.

Tolerances are not picked by hand: the same formula evaluated in float32 by numpy (sampling) or by the torch loop on the CPU (GAE) is compared
with float64 on the very inputs of the test, and the kernel is allowed 4x the largest error found over the test's cases, because its FMA
contraction and reduction order differ from numpy's."""
import numpy as np
import pytest

import ppo_ref
from ppo_ref import gae_inputs

pytestmark = pytest.mark.gpu

SAMPLE_CASES = [(2, 6, 1), (2, 6, 1000), (108, 39, 257), (403, 80, 65)]       # act_dim below, near and above 64 lanes; B not a multiple of 8
GAE_CASES = [(1, 1), (2, 63), (50, 64), (50, 65), (7, 1000)]


def random_policy(rng, obs_dim, act_dim, hidden=(32, 32, 32, 32)):
    sizes = [obs_dim, *hidden, 2 * act_dim]
    ks = [rng.normal(0, 1.0 / np.sqrt(sizes[i]), (sizes[i], sizes[i + 1])).astype(np.float32) for i in range(len(sizes) - 1)]
    bs = [rng.normal(0, 0.1, sizes[i + 1]).astype(np.float32) for i in range(len(sizes) - 1)]
    return rng.normal(0, 1, obs_dim).astype(np.float32), rng.uniform(0.5, 2.0, obs_dim).astype(np.float32), ks, bs


@pytest.fixture(scope="module")
def sample_runs():
    """Every case once: the kernel's outputs, the float64 log-probability at the kernel's own u, and the float32 numpy statement's error."""
    import torch
    from myosuite_mjx_amd.policy import BraxPolicy
    st = torch.cuda.current_stream().cuda_stream
    runs = {}
    for obs_dim, act_dim, B in SAMPLE_CASES:
        rng = np.random.default_rng(1000 * obs_dim + B)
        mean, std, ks, bs = random_policy(rng, obs_dim, act_dim)
        pol = BraxPolicy(mean, std, ks, bs)
        obs_np = rng.normal(0, 2, (B, obs_dim)).astype(np.float32)
        obs = torch.as_tensor(obs_np, device="cuda")
        ref_act = torch.empty((B, act_dim), dtype=torch.float32, device="cuda")
        act, raw, logp = torch.full_like(ref_act, np.nan), torch.full_like(ref_act, np.nan), torch.full((B,), np.nan, device="cuda")
        pol.act(obs.data_ptr(), B, ref_act.data_ptr(), deterministic=False, seed=11, step=5, stream=st)
        pol.sample(obs.data_ptr(), B, act.data_ptr(), raw.data_ptr(), logp.data_ptr(), seed=11, step=5, stream=st)
        tanh_raw = torch.tanh(raw)
        torch.cuda.synchronize()
        u = raw.cpu().numpy()
        lp64 = ppo_ref.log_prob(*ppo_ref.forward(obs_np, mean, std, ks, bs), u)
        lp32 = ppo_ref.log_prob(*ppo_ref.forward(obs_np, mean, std, ks, bs, dtype=np.float32), u, dtype=np.float32)
        runs[(obs_dim, act_dim, B)] = dict(ref_act=ref_act.cpu().numpy(), act=act.cpu().numpy(), raw=u, tanh_raw=tanh_raw.cpu().numpy(),
                                           logp=logp.cpu().numpy(), lp64=lp64, err32=float(np.abs(lp32 - lp64).max()))
    return runs


@pytest.mark.parametrize("case", SAMPLE_CASES)
def test_policy_sample(sample_runs, case):
    """action bit-equal to myo_policy_act's, tanh(u) bit-equal to action, log-probability against float64 at the kernel's own u.
    Measured on the MI355X: the float32 numpy statement (forward pass and formula) is off by at most 1.21e-5 over the four cases (the
    widest one, act_dim 80), so the kernel is allowed 4.83e-5; it is off by at most 9.7e-6.  (One tolerance for the four cases, not one each:
    the single sample of the B = 1 case happens to round well in numpy, 2.7e-8, which says nothing about what float32 may do there.)"""
    r = sample_runs[case]
    tol = 4 * max(v["err32"] for v in sample_runs.values())
    err = float(np.abs(r["logp"] - r["lp64"]).max())
    print(f"sample {case}: float32 numpy error {r['err32']:.3e}, tolerance {tol:.3e}, kernel error {err:.3e}, "
          f"tanh(u) != action at {int((r['tanh_raw'] != r['act']).sum())} of {r['act'].size}")
    assert np.isfinite(r["raw"]).all() and np.isfinite(r["logp"]).all()
    assert np.array_equal(r["act"], r["ref_act"])
    assert np.array_equal(r["tanh_raw"], r["act"])
    assert err <= tol


@pytest.fixture(scope="module")
def gae_runs():
    import torch
    from myosuite_mjx_amd import ppo
    runs = {}
    for T, B in GAE_CASES:
        args = gae_inputs(T, B)
        vs, adv = ppo.compute_gae(*(torch.as_tensor(a, device="cuda") for a in args), 0.95, 0.9)
        cvs, cadv = ppo.compute_gae(*(torch.as_tensor(a) for a in args), 0.95, 0.9)
        rvs, radv = ppo_ref.gae(*args, 0.95, 0.9)
        runs[(T, B)] = dict(vs=vs.cpu().numpy(), adv=adv.cpu().numpy(), cvs=cvs.numpy(), cadv=cadv.numpy(), rvs=rvs, radv=radv,
                            err32=float(max(np.abs(cvs.numpy() - rvs).max(), np.abs(cadv.numpy() - radv).max())))
    return runs


@pytest.mark.parametrize("case", GAE_CASES)
def test_ppo_gae(gae_runs, case):
    """myo_ppo_gae against float64 and against the torch fallback.  The float32 torch loop on the CPU is off from float64 by at most
    2.21e-6 over the five cases (values of size ~2, up to 50 steps), so the kernel is allowed 8.83e-6; measured on the MI355X it is off by at
    most 1.76e-6 from float64 and 1.55e-6 from the torch loop."""
    r = gae_runs[case]
    tol = 4 * max(v["err32"] for v in gae_runs.values())
    e64 = float(max(np.abs(r["vs"] - r["rvs"]).max(), np.abs(r["adv"] - r["radv"]).max()))
    eto = float(max(np.abs(r["vs"] - r["cvs"]).max(), np.abs(r["adv"] - r["cadv"]).max()))
    print(f"gae {case}: float32 torch error {r['err32']:.3e}, tolerance {tol:.3e}, kernel vs float64 {e64:.3e}, kernel vs torch {eto:.3e}")
    assert r["vs"].shape == case and r["adv"].shape == case
    assert e64 <= tol and eto <= tol


def test_ppo_gae_refuses_bad_arguments():
    import torch
    from myosuite_mjx_amd import capi
    L = capi.lib()
    x = torch.zeros((2, 3), device="cuda")
    p = x.data_ptr()
    assert L.myo_ppo_gae(p, p, p, p, p, 0, 3, 0.9, 0.9, p, p, None) == L.myo_ppo_gae(p, p, p, p, p, 2, 0, 0.9, 0.9, p, p, None) != 0
    assert L.myo_ppo_gae(p, None, p, p, p, 2, 3, 0.9, 0.9, p, p, None) != 0 and L.myo_ppo_gae(p, p, p, p, p, 2, 3, 0.9, 0.9, p, None, None) != 0
    with pytest.raises(capi.MyoError):
        capi._chk(L.myo_ppo_gae(None, p, p, p, p, 2, 3, 0.9, 0.9, p, p, None))
    torch.cuda.synchronize()
    assert float(x.abs().sum()) == 0.0


@pytest.mark.parametrize("on_device", [False, True])
def test_policy_update(on_device):
    import torch
    from myosuite_mjx_amd.policy import BraxPolicy, reference_forward
    rng = np.random.default_rng(3)
    obs_dim, act_dim, B = 108, 39, 257
    mean, std, ks, bs = random_policy(rng, obs_dim, act_dim)
    mean2, std2, ks2, bs2 = random_policy(rng, obs_dim, act_dim)
    pol = BraxPolicy(mean, std, ks, bs)
    obs_np = rng.normal(0, 2, (B, obs_dim)).astype(np.float32)
    obs = torch.as_tensor(obs_np, device="cuda")
    act = torch.empty((B, act_dim), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    give = (lambda a: None if a is None else torch.as_tensor(a, device="cuda")) if on_device else (lambda a: a)

    def err(mean, std, ks, bs):
        pol.act(obs.data_ptr(), B, act.data_ptr(), deterministic=True, stream=st)
        torch.cuda.synchronize()
        return np.abs(act.cpu().numpy() - reference_forward(obs_np, mean, std, ks, bs)[0]).max()
    assert err(mean, std, ks, bs) < 2e-5
    # None keeps: only the observation mean, then only the second kernel and the last bias, change
    pol.update(obs_mean=give(mean2))
    assert err(mean2, std, ks, bs) < 2e-5 and err(mean, std, ks, bs) > 1e-2
    pol.update(kernels=[None, give(ks2[1]), None, None, None], biases=[None] * 4 + [give(bs2[4])])
    assert err(mean2, std, [ks[0], ks2[1], *ks[2:]], [*bs[:4], bs2[4]]) < 2e-5
    pol.update(give(mean2), give(std2), [give(k) for k in ks2], [give(b) for b in bs2])
    assert err(mean2, std2, ks2, bs2) < 2e-5 and err(mean2, std, ks2, bs2) > 1e-2
    with pytest.raises(ValueError):
        pol.update(obs_mean=give(mean2[:-1]))
    with pytest.raises(ValueError):
        pol.update(kernels=[give(ks2[0])])


TRAIN_KW = dict(unroll_length=8, num_minibatches=4, num_updates_per_batch=2, seed=5, keep_first_rollout=True)


def _two_iterations(env_id, num_envs, tmp_path, **make_kw):
    import torch
    import myosuite_mjx_amd as myo
    from myosuite_mjx_amd import ppo
    from myosuite_mjx_amd.policy import BraxPolicy
    env = myo.make(env_id, num_envs=num_envs, **make_kw)
    seen = []
    pol, params, metrics = ppo.train(env, 2 * num_envs * 8, progress_fn=lambda n, m: seen.append(n), **TRAIN_KW)
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
    return metrics[0]["first_rollout"]


def test_train_two_iterations_pose(tmp_path):
    a = _two_iterations("myoElbowPose1D6MFixed-v0", 64, tmp_path)
    b = _two_iterations("myoElbowPose1D6MFixed-v0", 64, tmp_path)
    for k in ("obs", "u", "logp", "reward"):     # the first unroll is a function of the seed alone
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
    assert a["obs"].shape == (9, 64, a["obs"].shape[2]) and a["u"].shape == (8, 64, 6) and np.ptp(a["u"]) > 1.0


def test_train_two_iterations_myodm(tmp_path):
    """A MyoDM id hands out float views for terminated / truncated; the trainer casts them."""
    r = _two_iterations("MyoHandAirplaneRandom-v0", 32, tmp_path, seed=0, autoreset=True)
    assert r["obs"].shape == (9, 32, 70) and all(np.isfinite(r[k]).all() for k in r)
