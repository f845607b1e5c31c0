"""Float64 numpy statements of the PPO pieces (GAE, tanh-normal log-probability and entropy, running observation statistics, the loss),
written from the formulas of include/myo_hip_ppo.h and the issue that introduced them, not from myosuite_mjx_amd/ppo.py: the second,
independent statement the torch functions and the HIP kernels are compared with.  Every function takes a `dtype` so that the same
statement in float32 gives the rounding error a float32 implementation may be expected to make (the tests' tolerances come from it)."""
import numpy as np

LOG2 = np.log(2.0)
LOG_2PI = np.log(2.0 * np.pi)


def softplus(x):
    return np.logaddexp(x.dtype.type(0), x)


def gae_inputs(T, B, seed=0):
    """Rewards, values, bootstrap and termination / truncation flags drawn with probability 0.05 each and made disjoint."""
    rng = np.random.default_rng(1000 * T + B + seed)
    term = rng.random((T, B)) < 0.05
    trunc = (rng.random((T, B)) < 0.05) & ~term
    f = np.float32
    return (rng.normal(0, 1, (T, B)).astype(f), rng.normal(0, 2, (T, B)).astype(f), rng.normal(0, 2, B).astype(f), term.astype(f), trunc.astype(f))


def gae(rewards, values, bootstrap, termination, truncation, discount, lam, dtype=np.float64):
    r, v, boot, term, trunc = (np.asarray(a, dtype) for a in (rewards, values, bootstrap, termination, truncation))
    discount, lam, one = dtype(discount), dtype(lam), dtype(1)
    T = r.shape[0]
    vs, adv = np.zeros_like(v), np.zeros_like(v)
    acc = np.zeros_like(boot)
    for t in range(T - 1, -1, -1):
        mask = one - trunc[t]
        v_next = v[t + 1] if t + 1 < T else boot
        vs_next = vs[t + 1] if t + 1 < T else boot
        delta = (r[t] + discount * (one - term[t]) * v_next - v[t]) * mask
        acc = delta + discount * (one - term[t]) * mask * lam * acc
        vs[t] = acc + v[t]
        adv[t] = (r[t] + discount * (one - term[t]) * vs_next - v[t]) * mask
    return vs, adv


def log_det_tanh(u):
    t = u.dtype.type
    return t(2) * (t(LOG2) - u - softplus(t(-2) * u))


def log_prob(loc, scale, u, dtype=np.float64):
    loc, scale, u = (np.asarray(a, dtype) for a in (loc, scale, u))
    z = (u - loc) / scale
    log_normal = dtype(-0.5) * z * z - np.log(scale) - dtype(0.5 * LOG_2PI)
    return (log_normal - log_det_tanh(u)).sum(-1)


def entropy(loc, scale, u, dtype=np.float64):
    loc, scale, u = (np.asarray(a, dtype) for a in (loc, scale, u))
    return (dtype(0.5) + dtype(0.5 * LOG_2PI) + np.log(scale) + log_det_tanh(u)).sum(-1)


def forward(obs, obs_mean, obs_std, kernels, biases, dtype=np.float64):
    """(loc, scale) of the policy network: normalisation, swish MLP, scale = softplus(raw) + 0.001."""
    x = (np.asarray(obs, dtype) - np.asarray(obs_mean, dtype)) / np.asarray(obs_std, dtype)
    for i, (w, b) in enumerate(zip(kernels, biases)):
        x = x @ np.asarray(w, dtype) + np.asarray(b, dtype)
        if i + 1 < len(kernels):
            x = x / (dtype(1) + np.exp(-x))
    loc, raw = np.split(x, 2, axis=-1)
    return loc, softplus(raw) + dtype(0.001)


class RunningStats:
    def __init__(self, obs_dim):
        self.count, self.mean, self.summed_var = 0, np.zeros(obs_dim), np.zeros(obs_dim)

    def update(self, x):
        x = np.asarray(x, np.float64)
        self.count += x.shape[0]
        d = x - self.mean
        self.mean = self.mean + d.sum(0) / self.count
        self.summed_var = self.summed_var + (d * (x - self.mean)).sum(0)

    @property
    def std(self):
        if self.count == 0:
            return np.ones_like(self.mean)
        return np.clip(np.sqrt(np.maximum(self.summed_var / self.count, 0.0)), 1e-6, 1e6)


def loss(loc, scale, values, bootstrap, u, logp_behaviour, rewards, termination, truncation, entropy_noise, discounting, gae_lambda,
         clipping_epsilon, entropy_cost, reward_scaling, normalize_advantage):
    """(policy loss, value loss, entropy loss, rho, normalised advantage) in float64."""
    f = np.float64
    vs, adv = gae(np.asarray(rewards, f) * reward_scaling, values, bootstrap, termination, truncation, discounting, gae_lambda)
    if normalize_advantage:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    rho = np.exp(log_prob(loc, scale, u) - np.asarray(logp_behaviour, f))
    policy = -np.minimum(rho * adv, np.clip(rho, 1 - clipping_epsilon, 1 + clipping_epsilon) * adv).mean()
    value = 0.25 * ((vs - np.asarray(values, f)) ** 2).mean()
    u_ent = np.asarray(loc, f) + np.asarray(scale, f) * np.asarray(entropy_noise, f)
    ent = -entropy_cost * entropy(loc, scale, u_ent).mean()
    return policy, value, ent, rho, adv
