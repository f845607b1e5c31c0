"""One PPO minibatch SGD step stated in torch double (or, with dtype=torch.float32, in float32: the rounding error a float32 statement
may be expected to make), written from the formulas of include/myo_hip_ppo.h and tests/ppo_ref.py, not from myosuite_mjx_amd/ppo.py: the
second statement that myo_ppo_learner_step (tests/test_gpu_ppo_update.py) is compared with.  The GAE recurrence is ppo_ref.gae
(`ppo.compute_gae` casts to float32).  tests/test_ppo_update_host.py pins this file's gradient against finite differences of its loss."""
import math

import numpy as np
import torch

import ppo_ref

HYPER = dict(discounting=0.95, gae_lambda=0.95, clipping_epsilon=0.3, entropy_cost=1e-3, reward_scaling=5.0, normalize_advantage=True)
LR, BETA1, BETA2, ADAM_EPS = 3e-4, 0.9, 0.999, 1e-8
LOG2, HALF_LOG_2PI = math.log(2.0), 0.5 * math.log(2.0 * math.pi)


def mlp(x, ws, bs):
    for l, (w, b) in enumerate(zip(ws, bs)):
        x = x @ w + b
        if l + 1 < len(ws):
            x = x * torch.sigmoid(x)
    return x


def log_det_tanh(u):
    return 2.0 * (LOG2 - u - torch.nn.functional.softplus(-2.0 * u))


def gae_targets(values, case, idx, np_dtype=np.float64, hyper=HYPER):
    """(vs, normalised advantage) of the minibatch for the value rows `values` [T + 1, mb] (numpy): constants for the gradient."""
    h, T = hyper, case["u"].shape[0]
    vs, adv = ppo_ref.gae(case["rewards"][:, idx].astype(np_dtype) * np_dtype(h["reward_scaling"]), values[:T], values[T], case["termination"][:, idx],
                          case["truncation"][:, idx], h["discounting"], h["gae_lambda"], dtype=np_dtype)
    if h["normalize_advantage"]:
        adv = (adv - adv.mean()) / (adv.std() + np_dtype(1e-8))
    return vs, adv


def losses(params, case, idx, noise, dtype=torch.float64, hyper=HYPER, targets=None):
    """(policy loss, value loss, entropy loss, rho, normalised advantage) of the minibatch `idx` (env columns) of `case` at `params` =
    (pw, pb, vw, vb), lists of tensors of `dtype`.  targets: (vs, advantage) to use in place of those of `params`' own values (a finite
    difference of this loss has to hold them fixed, as the gradient does)."""
    h, T = hyper, case["u"].shape[0]
    np_dtype = np.float64 if dtype == torch.float64 else np.float32
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=dtype)
    pw, pb, vw, vb = params
    x = (t(case["obs"][:, idx]) - t(case["mean"])) / t(case["std"])
    loc, raw = torch.chunk(mlp(x[:T], pw, pb), 2, dim=-1)
    scale = torch.nn.functional.softplus(raw) + 0.001
    v = mlp(x, vw, vb).squeeze(-1)
    vs, adv = gae_targets(v.detach().numpy(), case, idx, np_dtype, h) if targets is None else targets
    vs, adv = t(vs), t(adv)
    u = t(case["u"][:, idx])
    z = (u - loc) / scale
    logp = (-0.5 * z * z - torch.log(scale) - HALF_LOG_2PI - log_det_tanh(u)).sum(-1)
    rho = torch.exp(logp - t(case["logp"][:, idx]))
    eps = h["clipping_epsilon"]
    policy = -torch.minimum(rho * adv, torch.clamp(rho, 1.0 - eps, 1.0 + eps) * adv).mean()
    value = 0.25 * ((vs - v[:T]) ** 2).mean()
    u_ent = loc + scale * t(noise)
    entropy = -h["entropy_cost"] * (0.5 + HALF_LOG_2PI + torch.log(scale) + log_det_tanh(u_ent)).sum(-1).mean()
    return policy, value, entropy, rho.detach(), adv


def as_params(arrays, dtype=torch.float64):
    """(pw, pb, vw, vb) numpy lists -> leaf tensors of `dtype` that ask for gradients."""
    return tuple([torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in group] for group in arrays)


def gradients(arrays, case, idx, noise, dtype=torch.float64, hyper=HYPER):
    """Autograd of policy + value + entropy loss at the numpy parameters `arrays`: ((gpw, gpb, gvw, gvb) as float64 numpy lists, the three loss
    terms, rho, normalised advantage)."""
    params = as_params(arrays, dtype)
    policy, value, entropy, rho, adv = losses(params, case, idx, noise, dtype, hyper)
    (policy + value + entropy).backward()
    grads = tuple([p.grad.numpy().astype(np.float64) for p in group] for group in params)
    return grads, (float(policy.detach()), float(value.detach()), float(entropy.detach())), rho.numpy().astype(np.float64), adv.numpy().astype(np.float64)


def gradient_error(grads, grads64):
    """max |g - g64| / max |g64| per tensor, then the worst over the tensors."""
    worst = 0.0
    for group, group64 in zip(grads, grads64):
        for g, g64 in zip(group, group64):
            top = float(np.abs(g64).max())
            assert top > 0.0, "a float64 gradient tensor is all zero: the case says nothing about it"
            worst = max(worst, float(np.abs(np.asarray(g, np.float64) - g64).max()) / top)
    return worst


def clip_figures(rho, adv, eps=HYPER["clipping_epsilon"]):
    """(smallest distance of rho to a clip edge, share of samples outside the clip range)."""
    return float(np.minimum(np.abs(rho - (1 - eps)), np.abs(rho - (1 + eps))).min()), float(((rho < 1 - eps) | (rho > 1 + eps)).mean())


def make_case(T, mb, obs_dim, act_dim, policy_hidden=(32, 32, 32, 32), value_hidden=(256,) * 5, seed=0, steps=3):
    """A rollout of B = 2 mb + 1 envs and `steps` minibatches of it: networks from ppo.init_networks with N(0, 0.1) biases, observations
    N(0.3, 2), mean N(0, 0.5), std U(0.5, 2), u and the behaviour log-probability sampled from a perturbed copy of the policy (kernels +
    0.05 mean|w| N(0, 1), which spreads rho around 1), rewards and flags from ppo_ref.gae_inputs, entropy noise N(0, 1), idx: `steps`
    shuffled subsets of the columns."""
    from myosuite_mjx_amd import ppo
    rng = np.random.default_rng(seed)
    B, f = 2 * mb + 1, np.float32
    nets = ppo.init_networks(obs_dim, act_dim, policy_hidden, value_hidden, seed)
    pw, pb, vw, vb = ([a.detach().numpy().copy() for a in group] for group in nets)
    pb = [(b + rng.normal(0, 0.1, b.shape)).astype(f) for b in pb]
    vb = [(b + rng.normal(0, 0.1, b.shape)).astype(f) for b in vb]
    obs = rng.normal(0.3, 2.0, (T + 1, B, obs_dim)).astype(f)
    mean, std = rng.normal(0, 0.5, obs_dim).astype(f), rng.uniform(0.5, 2.0, obs_dim).astype(f)
    behaviour = [w + 0.05 * np.abs(w).mean() * rng.normal(0, 1, w.shape) for w in pw]
    loc, scale = ppo_ref.forward(obs[:T], mean, std, behaviour, pb)
    u = (loc + scale * rng.normal(0, 1, loc.shape)).astype(f)
    logp = ppo_ref.log_prob(loc, scale, u).astype(f)
    rewards, _, _, termination, truncation = ppo_ref.gae_inputs(T, B, seed)
    return dict(T=T, mb=mb, B=B, obs_dim=obs_dim, act_dim=act_dim, params=(pw, pb, vw, vb), obs=obs, mean=mean, std=std, u=u, logp=logp,
                rewards=rewards, termination=termination, truncation=truncation,
                idx=[rng.permutation(B)[:mb].astype(np.int64) for _ in range(steps)],
                noise=[rng.normal(0, 1, (T, mb, act_dim)).astype(f) for _ in range(steps)])


class Adam64:
    """torch.optim.Adam(lr) without weight decay, in float64 numpy, on one flat list of arrays."""

    def __init__(self, params, lr=LR, beta1=BETA1, beta2=BETA2, eps=ADAM_EPS):
        self.p = [np.asarray(a, np.float64).copy() for a in params]
        self.m, self.v = [np.zeros_like(a) for a in self.p], [np.zeros_like(a) for a in self.p]
        self.lr, self.b1, self.b2, self.eps, self.t = lr, beta1, beta2, eps, 0

    def step(self, grads):
        self.t += 1
        for p, m, v, g in zip(self.p, self.m, self.v, grads):
            g = np.asarray(g, np.float64)
            m[...] = self.b1 * m + (1 - self.b1) * g
            v[...] = self.b2 * v + (1 - self.b2) * g * g
            p -= self.lr / (1 - self.b1 ** self.t) * m / (np.sqrt(v) / math.sqrt(1 - self.b2 ** self.t) + self.eps)
