"""CPU tests of myosuite_mjx_amd.ppo: the torch statements of GAE, the tanh-normal log-probability and entropy, the running observation
statistics and the loss against the float64 numpy statements of tests/ppo_ref.py; the trainer's argument checks; a whole training run on
the torch backend; save -> BraxPolicy's .npz.  The HIP kernels are compared with the same statements in tests/test_gpu_ppo.py."""
import numpy as np
import pytest
import torch

import ppo_ref
from ppo_ref import gae_inputs
from myosuite_mjx_amd import ppo
from myosuite_mjx_amd.policy import reference_forward

EPS32 = float(np.finfo(np.float32).eps)


def gae_bound(T, args, discount, lam):
    """What a float32 evaluation of the recurrence may be off by: each of the T trips adds a few roundings of numbers no larger than the
    largest |vs|, |adv| or input, and the errors of later trips are carried down with a factor <= discount * lambda < 1 -- so a dozen
    roundings of the largest magnitude per trip, summed over the trips as a geometric series."""
    vs, adv = ppo_ref.gae(*args, discount, lam)
    mag = max(np.abs(vs).max(), np.abs(adv).max(), *(np.abs(a).max() for a in args[:3]))
    return 12 * EPS32 * mag / (1 - discount * lam)


@pytest.mark.parametrize("T,B", [(1, 1), (2, 3), (50, 65)])
def test_gae_torch_matches_float64(T, B):
    args = gae_inputs(T, B)
    vs, adv = ppo.compute_gae(*(torch.as_tensor(a) for a in args), 0.95, 0.9)
    rvs, radv = ppo_ref.gae(*args, 0.95, 0.9)
    bound = gae_bound(T, args, 0.95, 0.9)
    assert vs.dtype == torch.float32 and vs.shape == (T, B) and adv.shape == (T, B)
    assert np.abs(vs.numpy() - rvs).max() <= bound and np.abs(adv.numpy() - radv).max() <= bound
    if T == 50:     # the flags matter: without them the result differs
        assert args[3].sum() > 0 and args[4].sum() > 0 and (args[3] * args[4]).sum() == 0
        plain, _ = ppo_ref.gae(args[0], args[1], args[2], 0 * args[3], 0 * args[4], 0.95, 0.9)
        assert np.abs(plain - rvs).max() > 0.1


def test_gae_by_hand():
    """T = 3, B = 1, discount = lambda = 1/2, rewards 1, 2, 3, values 1/2, 1, 2, bootstrap 4.  Every number is exact in float32.
    t = 2 (both cases): delta = 3 + 4/2 - 2 = 3, acc = 3, vs = 5, adv = 3 + 4/2 - 2 = 3.
    Termination at t = 1: nothing of t = 2 reaches back.  delta = 2 - 1 = 1, acc = 1, vs = 2, adv = 1;
                          t = 0: delta = 1 + 1/2 - 1/2 = 1, acc = 1 + 1/4 * 1 = 5/4, vs = 7/4, adv = 1 + 2/2 - 1/2 = 3/2.
    Truncation at t = 1:  the step is masked out.  delta = 0, acc = 0, vs = 1 (= its value), adv = 0;
                          t = 0: delta = 1, acc = 1 + 1/4 * 0 = 1, vs = 3/2, adv = 1 + 1/2 - 1/2 = 1."""
    r, v, boot = torch.tensor([[1.0], [2.0], [3.0]]), torch.tensor([[0.5], [1.0], [2.0]]), torch.tensor([4.0])
    flag, zero = torch.tensor([[0.0], [1.0], [0.0]]), torch.zeros(3, 1)
    vs, adv = ppo.compute_gae(r, v, boot, flag, zero, 0.5, 0.5)
    assert vs[:, 0].tolist() == [1.75, 2.0, 5.0] and adv[:, 0].tolist() == [1.5, 1.0, 3.0]
    vs, adv = ppo.compute_gae(r, v, boot, zero, flag, 0.5, 0.5)
    assert vs[:, 0].tolist() == [1.5, 1.0, 5.0] and adv[:, 0].tolist() == [1.0, 0.0, 3.0]
    for a, b in ((flag, zero), (zero, flag)):     # the float64 statement says the same
        rvs, radv = ppo_ref.gae(r.numpy(), v.numpy(), boot.numpy(), a.numpy(), b.numpy(), 0.5, 0.5)
        vs, adv = ppo.compute_gae(r, v, boot, a, b, 0.5, 0.5)
        assert np.array_equal(vs.numpy(), rvs) and np.array_equal(adv.numpy(), radv)


def test_gae_refuses_bad_shapes():
    z = torch.zeros(2, 3)
    with pytest.raises(ValueError):
        ppo.compute_gae(z, z, torch.zeros(2), z, z, 0.9, 0.9)
    with pytest.raises(ValueError):
        ppo.compute_gae(torch.zeros(0, 3), torch.zeros(0, 3), torch.zeros(3), torch.zeros(0, 3), torch.zeros(0, 3), 0.9, 0.9)


@pytest.mark.parametrize("act_dim", [1, 6, 80])
def test_log_prob_and_entropy_match_float64(act_dim):
    """u runs up to |u| = 12, where tanh(u) == +-1 in float32 and log(1 - tanh(u)^2) is -inf: the softplus form stays finite.
    Bound: each of the act_dim terms is a short sum of z^2 / 2, log scale, a constant and 2 (log 2 - u - softplus(-2u)), every piece
    rounded a few times, so 8 eps32 times the sum of the pieces' magnitudes."""
    rng = np.random.default_rng(act_dim)
    N = 40
    u = np.concatenate([rng.uniform(-12, 12, (N - 2, act_dim)), np.full((1, act_dim), 12.0), np.full((1, act_dim), -12.0)]).astype(np.float32)
    loc = (u + rng.normal(0, 1, u.shape)).astype(np.float32)
    scale = rng.uniform(0.05, 2.0, u.shape).astype(np.float32)
    assert np.all(np.abs(np.tanh(u[-2:])) == 1.0)
    lp = ppo.tanh_normal_log_prob(torch.as_tensor(loc), torch.as_tensor(scale), torch.as_tensor(u)).numpy()
    en = ppo.tanh_normal_entropy(torch.as_tensor(loc), torch.as_tensor(scale), torch.as_tensor(u)).numpy()
    z = (u.astype(np.float64) - loc) / scale
    pieces = 0.5 * z * z + np.abs(np.log(scale.astype(np.float64))) + 1.5 + 2 * (np.log(2) + np.abs(u) + np.logaddexp(0, -2.0 * u))
    bound = 8 * EPS32 * pieces.sum(-1)
    assert lp.shape == (N,) and np.isfinite(lp).all() and np.isfinite(en).all()
    assert np.all(np.abs(lp - ppo_ref.log_prob(loc, scale, u)) <= bound)
    assert np.all(np.abs(en - ppo_ref.entropy(loc, scale, u)) <= bound)
    # the density integrates to one over the action: for act_dim = 1, sum of exp(log_prob) da over a grid of a = tanh(u)
    if act_dim == 1:
        g = np.linspace(-8, 8, 20001)[:, None]
        p = np.exp(ppo_ref.log_prob(np.full_like(g, 0.3), np.full_like(g, 0.7), g))
        a = np.tanh(g[:, 0])
        assert abs(np.sum(0.5 * (p[1:] + p[:-1]) * np.diff(a)) - 1.0) < 1e-6


def test_running_stats_one_batch_and_three():
    rng = np.random.default_rng(5)
    x = (rng.normal(0, 1, (300, 5)) * [0.1, 1, 3, 10, 1] + [5, -2, 0, 40, 0]).astype(np.float32)
    x[:, 4] = 2.5                                                   # a constant column: std is clipped at 1e-6, not zero
    one, three, ref = ppo.RunningStats(5), ppo.RunningStats(5), ppo_ref.RunningStats(5)
    assert one.count == 0 and one.mean.tolist() == [0.0] * 5 and one.std.tolist() == [1.0] * 5
    one.update(torch.as_tensor(x))
    for part in (x[:7], x[7:150], x[150:]):
        three.update(torch.as_tensor(part))
        ref.update(part)
    assert one.count == three.count == ref.count == 300
    x64 = x.astype(np.float64)
    # float32 sums of 300 numbers of size <= |x|max: relative error of a few sqrt(300) eps
    tol = 64 * EPS32 * np.abs(x64).max(0)
    for s in (one, three):
        assert np.all(np.abs(s.mean.numpy() - x64.mean(0)) <= tol)
        assert np.all(np.abs(s.std.numpy()[:4] - x64.std(0)[:4]) <= 30 * tol[:4])     # the variance is a difference of sums: less exact
        assert abs(float(s.std[4]) - 1e-6) < 1e-9
    assert np.allclose(ref.mean, x64.mean(0), atol=1e-12) and np.allclose(ref.std[:4], x64.std(0)[:4], atol=1e-12)


def _minibatch(T=5, B=8, A=3, seed=2):
    rng = np.random.default_rng(seed)
    f = np.float32
    d = dict(loc=rng.normal(0, 0.5, (T, B, A)), scale=rng.uniform(0.3, 1.2, (T, B, A)), values=rng.normal(0, 1, (T, B)),
             bootstrap=rng.normal(0, 1, B), u=rng.normal(0, 1, (T, B, A)), rewards=rng.normal(0, 0.3, (T, B)),
             termination=(rng.random((T, B)) < 0.1), entropy_noise=rng.normal(0, 1, (T, B, A)))
    d["truncation"] = (rng.random((T, B)) < 0.1) & ~d["termination"]
    d = {k: v.astype(f) for k, v in d.items()}
    # behaviour log-probabilities: the current ones, shifted so that rho = exp(-shift) spreads over (0.5, 2): some clipped at both ends
    d["logp_behaviour"] = (ppo_ref.log_prob(d["loc"], d["scale"], d["u"]) + rng.uniform(-0.7, 0.7, (T, B))).astype(f)
    return d


HYPER = dict(discounting=0.95, gae_lambda=0.9, clipping_epsilon=0.3, entropy_cost=1e-2, reward_scaling=5.0, normalize_advantage=True)
ORDER = ("loc", "scale", "values", "bootstrap", "u", "logp_behaviour", "rewards", "termination", "truncation", "entropy_noise")


@pytest.mark.parametrize("normalize", [True, False])
def test_loss_matches_float64(normalize):
    d = _minibatch()
    hyper = dict(HYPER, normalize_advantage=normalize)
    total, terms = ppo.loss(*(torch.as_tensor(d[k]) for k in ORDER), **hyper)
    pol, val, ent, rho, adv = ppo_ref.loss(*(d[k] for k in ORDER), **hyper)
    assert ((rho > 1.3) & (adv > 0)).any() and ((rho < 0.7) & (adv < 0)).any() and ((rho > 0.7) & (rho < 1.3)).any()
    # float32 against float64 on 40 samples of size O(1..10): a few hundred roundings at the most
    assert abs(float(terms["policy_loss"]) - pol) < 2e-5 * max(1.0, abs(pol))
    assert abs(float(terms["value_loss"]) - val) < 2e-5 * max(1.0, abs(val))
    assert abs(float(terms["entropy_loss"]) - ent) < 2e-5 * max(1.0, abs(ent))
    assert abs(float(total) - (pol + val + ent)) < 6e-5 * max(1.0, abs(pol + val + ent))


def test_policy_gradient_is_zero_where_rho_is_clipped():
    d = _minibatch()
    t = {k: torch.as_tensor(d[k]) for k in ORDER}
    t["loc"].requires_grad_()
    t["scale"].requires_grad_()
    hyper = dict(HYPER, entropy_cost=0.0)                            # the policy loss alone reaches loc and scale
    total, _ = ppo.loss(*(t[k] for k in ORDER), **hyper)
    total.backward()
    _, _, _, rho, adv = ppo_ref.loss(*(d[k] for k in ORDER), **hyper)
    clipped = ((rho > 1.3) & (adv > 0)) | ((rho < 0.7) & (adv < 0))
    margin = (np.abs(rho - 1.3) > 1e-4) & (np.abs(rho - 0.7) > 1e-4)  # (no sample sits on a clip boundary in float32 but not in float64)
    assert margin.all() and clipped.any() and (~clipped).any()
    g = t["loc"].grad.numpy()
    assert np.all(g[clipped] == 0) and np.all(t["scale"].grad.numpy()[clipped] == 0)
    assert np.all(np.abs(g[~clipped]).max(-1) > 0)
    assert t["values"].grad is None                                   # (values did not ask for one; vs and A are detached)
    v = t["values"].clone().requires_grad_()
    total, _ = ppo.loss(t["loc"].detach(), t["scale"].detach(), v, *(t[k] for k in ORDER[3:]), **hyper)
    total.backward()
    vs, _ = ppo_ref.gae(d["rewards"].astype(np.float64) * 5.0, d["values"], d["bootstrap"], d["termination"], d["truncation"], 0.95, 0.9)
    assert np.abs(v.grad.numpy() - 0.5 * (d["values"] - vs) / vs.size).max() < 1e-6      # d/dV of 1/4 mean((vs - V)^2), vs held fixed


class _Shape:
    """An env that must not be touched: the argument checks come before anything is allocated."""

    def __init__(self, num_envs=64, obs_dim=3, act_dim=2, max_episode_steps=None):
        self.num_envs, self.obs_dim, self.act_dim = num_envs, obs_dim, act_dim
        if max_episode_steps is not None:
            self.max_episode_steps = max_episode_steps

    def reset(self, seed=None):
        raise AssertionError("reset() was called before the arguments were checked")

    step = reset


@pytest.mark.parametrize("env_kw,kw", [
    ({}, dict(num_minibatches=5)),                                   # 64 % 5 != 0
    ({}, dict(unroll_length=0)),
    ({}, dict(action_repeat=0)),
    ({}, dict(policy_hidden=(32, 513))),                             # wider than the kernel's 512
    ({}, dict(policy_hidden=(32,) * 8)),                             # 8 hidden layers + the head = 9 > 8
    ({"act_dim": 257}, {}),                                          # the head, 2 * act_dim, is a layer too
    ({"obs_dim": 1025}, {}),                                         # wider than the LDS tile
    ({"max_episode_steps": 100}, dict(episode_length=50)),
])
def test_train_refuses(env_kw, kw):
    args = dict(num_minibatches=4)
    args.update(kw)
    with pytest.raises(ValueError):
        ppo.train(_Shape(**env_kw), 1000, **args)


class BanditEnv:
    """One-step episodes: a constant observation, reward = -|a - a*|^2, every step ends the episode."""
    num_envs, obs_dim, act_dim = 64, 3, 2

    def __init__(self):
        self.obs = torch.tensor([0.5, -1.0, 2.0]).repeat(self.num_envs, 1)
        self.target = torch.tensor([0.6, -0.4])
        self.done, self.never = torch.ones(self.num_envs, dtype=torch.bool), torch.zeros(self.num_envs, dtype=torch.bool)

    def reset(self, seed=None):
        return self.obs

    def step(self, action):
        return self.obs, -((action - self.target) ** 2).sum(-1), self.done, self.never, {}


TRAIN_KW = dict(unroll_length=4, num_minibatches=4, num_updates_per_batch=4, learning_rate=3e-3, reward_scaling=1.0, policy_hidden=(32, 32),
                value_hidden=(64, 64), seed=3)


@pytest.fixture(scope="module")
def bandit_run():
    seen = []
    out = ppo.train(BanditEnv(), 30 * 64 * 4, progress_fn=lambda n, m: seen.append(n), keep_first_rollout=True, **TRAIN_KW)
    return out + (seen,)


def test_training_run_on_the_torch_path_learns(bandit_run):
    """30 iterations of 64 envs x 4 steps, seed 3.  Measured: mean episode reward -1.53 in the first iteration, -0.02 in the last, an
    improvement of 1.51; the margin asked for is 0.75, half of it."""
    pol, params, metrics, seen = bandit_run
    assert pol is None and len(metrics) == 30 and seen == [256 * (i + 1) for i in range(30)]
    first, last = metrics[0], metrics[-1]
    print("bandit: first", first["eval/episode_reward"], "last", last["eval/episode_reward"])
    assert first["episodes"] == 256 and first["eval/episode_length"] == 1.0
    assert last["eval/episode_reward"] > first["eval/episode_reward"] + 0.75
    assert all(np.isfinite(m[k]) for m in metrics for k in ("policy_loss", "value_loss", "entropy_loss", "steps_per_s"))
    assert float(params["obs_count"]) == 30 * 256
    # a constant observation: mean = the observation, std at its floor
    assert np.allclose(params["obs_mean"], [0.5, -1.0, 2.0], atol=1e-5) and np.all(params["obs_std"] < 1e-3)


def test_training_run_is_reproducible():
    a = ppo.train(BanditEnv(), 2 * 256, keep_first_rollout=True, **TRAIN_KW)
    b = ppo.train(BanditEnv(), 2 * 256, keep_first_rollout=True, **TRAIN_KW)
    for k in ("obs", "u", "logp", "reward"):
        assert np.array_equal(a[2][0]["first_rollout"][k], b[2][0]["first_rollout"][k])
    assert all(np.array_equal(a[1][k], b[1][k]) for k in a[1])
    r = a[2][0]["first_rollout"]
    assert np.abs(r["reward"] + ((np.tanh(r["u"].astype(np.float64)) - [0.6, -0.4]) ** 2).sum(-1)).max() < 1e-5      # the action taken is tanh(u)


def test_action_repeat_sums_rewards_up_to_the_first_end():
    """Episodes of three steps with reward 1 each and action_repeat = 2: the repeats cover steps (1, 2), (3, then 1 of the next episode,
    which is not counted), (2, 3), (1, 2): rewards 2, 1, 2, 2, and two episodes end per env, of 3 and 2 counted steps."""
    class Count:
        num_envs, obs_dim, act_dim = 4, 1, 1

        def __init__(self):
            self.k = 0

        def reset(self, seed=None):
            self.k = 0
            return torch.zeros(4, 1)

        def step(self, action):
            self.k += 1
            end = torch.full((4,), self.k % 3 == 0)
            return torch.zeros(4, 1), torch.ones(4), end & False, end, {}
    _, _, metrics = ppo.train(Count(), 1, unroll_length=4, num_minibatches=1, num_updates_per_batch=1, action_repeat=2, policy_hidden=(8,),
                              value_hidden=(8,), keep_first_rollout=True)
    assert metrics[0]["first_rollout"]["reward"][:, 0].tolist() == [2.0, 1.0, 2.0, 2.0]
    assert metrics[0]["episodes"] == 2 * 4 and metrics[0]["eval/episode_length"] == 2.5 and metrics[0]["eval/episode_reward"] == 2.5


def test_save_round_trip(tmp_path, bandit_run):
    _, params, _, _ = bandit_run
    path = tmp_path / "policy.npz"
    ppo.save(path, params)
    z = np.load(path, allow_pickle=False)
    n = len(TRAIN_KW["policy_hidden"]) + 1
    assert sorted(z.files) == sorted(["obs_mean", "obs_std", "obs_count"] + [f"{p}{i}" for p in ("w", "b") for i in range(n)]
                                     + [f"{p}{i}" for p in ("vw", "vb") for i in range(len(TRAIN_KW["value_hidden"]) + 1)])
    assert sum(1 for k in z.files if k.startswith("w")) == n         # what BraxPolicy.from_npz counts as the policy's layers
    assert z["w0"].shape == (3, 32) and z[f"w{n - 1}"].shape == (32, 4) and z["vw2"].shape == (64, 1)
    obs = np.random.default_rng(0).normal(0, 1, (16, 3)) * 1e-4 + [0.5, -1.0, 2.0]
    ref, _, _ = reference_forward(obs, z["obs_mean"], z["obs_std"], [z[f"w{i}"] for i in range(n)], [z[f"b{i}"] for i in range(n)])
    t = {k: torch.as_tensor(np.asarray(v, np.float64)) for k, v in params.items()}
    loc, _ = ppo.policy_forward(torch.as_tensor(obs), t["obs_mean"], t["obs_std"], [t[f"w{i}"] for i in range(n)], [t[f"b{i}"] for i in range(n)])
    assert np.abs(torch.tanh(loc).numpy() - ref).max() < 1e-6
