"""PPO training on the device: the native counterpart of the reference's `mjx/ppo_continuous_action.py`, which builds a `TrackEnv`
and hands it to brax's `ppo.train`.  brax and jax are absent here, so the algorithm is restated from brax's documentation
-- parity with brax itself is unpinned, as for `policy.BraxPolicy`.

What runs where.  HIP (include/myo_hip_ppo.h): the rollout's action sampling with log-probabilities (`myo_policy_sample`, one launch per
env step next to the env's own), the advantage recurrence (`myo_ppo_gae`, one launch per SGD step where a torch loop takes six or more per
time step) and the refresh of the device policy's weights (`myo_policy_update`, device to device).  torch: the two networks' forward and
backward passes, Adam, and a handful of reductions (running observation statistics, metrics).
With `train(..., update="hip")` (opt-in; the default is the torch update above) the whole SGD step is HIP as well: `Learner` wraps
`myo_ppo_learner_step`, which gathers and normalises the minibatch's observations, runs both networks forward and backward on the FP32
matrix cores, GAE, the loss and Adam in 3 (policy layers + value layers) + 2 launches, and keeps the parameters on the device.  torch then
only draws the permutation and the entropy noise and keeps the running observation statistics.

Every function below dispatches on where its tensors live: CUDA tensors go to the HIP kernel, CPU tensors to a plain torch statement of
the same formula, which is also what a CPU-only training run (`backend="torch"`, or an env whose observations are CPU tensors) uses.

Formulas (brax's, restated):
    scale = softplus(raw) + 0.001;  u = loc + scale * eps;  action = tanh(u)
    log pi(u) = sum_j [ log N(u_j; loc_j, scale_j) - 2 (log 2 - u_j - softplus(-2 u_j)) ]
    entropy   = sum_j [ 1/2 + 1/2 log(2 pi) + log scale_j + 2 (log 2 - u_j - softplus(-2 u_j)) ]      (u: a fresh sample)
    GAE: see `compute_gae`;  loss: see `loss`.
"""
from __future__ import annotations

import ctypes as C
import math
import time

import numpy as np

from . import capi

_LOG2 = math.log(2.0)
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
# limits of the policy kernel (csrc/myo_kernels_ppo.h): layer widths, layer count, and the LDS tile that holds two activation rows of 8 envs
MAX_WIDTH, MAX_LAYERS, MAX_OBS_DIM = 512, 8, 64 * 1024 // (2 * 8 * 4)


def _gae_torch(rewards, values, bootstrap, termination, truncation, discount, gae_lambda):
    import torch
    T = rewards.shape[0]
    vs, adv = torch.empty_like(values), torch.empty_like(values)
    v_next, vs_next, acc = bootstrap, bootstrap, torch.zeros_like(bootstrap)
    for t in range(T - 1, -1, -1):
        cont, mask = discount * (1.0 - termination[t]), 1.0 - truncation[t]
        delta = (rewards[t] + cont * v_next - values[t]) * mask
        acc = delta + cont * mask * gae_lambda * acc
        vs[t] = acc + values[t]
        adv[t] = (rewards[t] + cont * vs_next - values[t]) * mask
        v_next, vs_next = values[t], vs[t]
    return vs, adv


def compute_gae(rewards, values, bootstrap, termination, truncation, discount, gae_lambda):
    """Generalised advantage estimation, brax's compute_gae.  [T, B] float32 tensors (termination / truncation as 0 / 1), bootstrap [B]:
        mask_t  = 1 - truncation_t;  v_next_t = values_{t+1} (bootstrap for t = T-1)
        delta_t = (rewards_t + discount (1 - termination_t) v_next_t - values_t) mask_t
        acc_t   = delta_t + discount (1 - termination_t) mask_t lambda acc_{t+1}                    (acc_T = 0)
        vs_t    = acc_t + values_t
        adv_t   = (rewards_t + discount (1 - termination_t) vs_{t+1} - values_t) mask_t             (vs_T = bootstrap)
    Returns (vs, adv), without gradient.  CUDA tensors: one launch of myo_ppo_gae on torch's current stream."""
    import torch
    with torch.no_grad():
        args = [torch.as_tensor(a, dtype=torch.float32).detach().contiguous() for a in (rewards, values, bootstrap, termination, truncation)]
        r, v, boot = args[0], args[1], args[2]
        if r.dim() != 2 or r.shape[0] < 1 or r.shape[1] < 1 or any(a.shape != r.shape for a in (v, args[3], args[4])) or boot.shape != r.shape[1:]:
            raise ValueError("compute_gae: rewards, values, termination, truncation are [T, B] and bootstrap is [B], T, B >= 1")
        if not r.is_cuda:
            return _gae_torch(*args, float(discount), float(gae_lambda))
        if any(a.device != r.device for a in args):
            raise ValueError("compute_gae: all tensors must be on one device")
        vs, adv = torch.empty_like(v), torch.empty_like(v)
        with torch.cuda.device(r.device):
            capi._chk(capi.lib().myo_ppo_gae(*(a.data_ptr() for a in args), r.shape[0], r.shape[1], float(discount), float(gae_lambda),
                                             vs.data_ptr(), adv.data_ptr(), torch.cuda.current_stream().cuda_stream))
        return vs, adv


def _log_det_tanh(u):
    """log |d tanh(u) / du| = 2 (log 2 - u - softplus(-2 u)): finite where 1 - tanh(u)^2 underflows."""
    import torch
    return 2.0 * (_LOG2 - u - torch.nn.functional.softplus(-2.0 * u))


def tanh_normal_log_prob(loc, scale, u):
    """log-probability of the action tanh(u) under the tanh-squashed normal, summed over the last axis."""
    import torch
    z = (u - loc) / scale
    return (-0.5 * z * z - torch.log(scale) - _HALF_LOG_2PI - _log_det_tanh(u)).sum(-1)


def tanh_normal_entropy(loc, scale, u):
    """brax's entropy estimate of the tanh-squashed normal: the normal's entropy plus the log-determinant at a sample u."""
    import torch
    return (0.5 + _HALF_LOG_2PI + torch.log(scale) + _log_det_tanh(u)).sum(-1)


class RunningStats:
    """brax's running observation statistics: count, mean, summed variance; std = clip(sqrt(max(summed_var / count, 0)), 1e-6, 1e6).
    Before the first update mean = 0 and std = 1."""

    def __init__(self, obs_dim, device="cpu"):
        import torch
        self.count = 0
        self.mean = torch.zeros(obs_dim, dtype=torch.float32, device=device)
        self.summed_var = torch.zeros(obs_dim, dtype=torch.float32, device=device)
        self.std = torch.ones(obs_dim, dtype=torch.float32, device=device)

    def update(self, x):
        """x [N, obs_dim]: count' = count + N; d = x - mean; mean' = mean + sum(d) / count'; summed_var' = summed_var + sum(d (x - mean'))."""
        import torch
        with torch.no_grad():
            x = x.reshape(-1, self.mean.shape[0]).to(self.mean.dtype)
            self.count += x.shape[0]
            d = x - self.mean
            self.mean = self.mean + d.sum(0) / self.count
            self.summed_var = self.summed_var + (d * (x - self.mean)).sum(0)
            self.std = torch.clamp(torch.sqrt(torch.clamp(self.summed_var / self.count, min=0.0)), 1e-6, 1e6)


def loss(loc, scale, values, bootstrap, u, logp_behaviour, rewards, termination, truncation, entropy_noise, *, discounting=0.95,
         gae_lambda=0.95, clipping_epsilon=0.3, entropy_cost=1e-3, reward_scaling=5.0, normalize_advantage=True):
    """brax's PPO loss on one minibatch of whole unrolls.  loc, scale, u, entropy_noise: [T, B, act_dim]; values, logp_behaviour, rewards,
    termination, truncation: [T, B]; bootstrap [B] = the value of the observation after the unroll.
        vs, A  = compute_gae(rewards * reward_scaling, values, bootstrap, ...), detached; A = (A - mean) / (std + 1e-8) if normalize_advantage (std over the minibatch, 1/N)
        rho    = exp(log pi(u) - logp_behaviour)
        policy = -mean(min(rho A, clip(rho, 1 - eps, 1 + eps) A));  value = 1/4 mean((vs - V)^2)
        entropy = -entropy_cost mean(entropy at loc + scale * entropy_noise)
    Returns (total, {"policy_loss", "value_loss", "entropy_loss"})."""
    import torch
    vs, adv = compute_gae(rewards * reward_scaling, values, bootstrap, termination, truncation, discounting, gae_lambda)
    if normalize_advantage:
        adv = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
    rho = torch.exp(tanh_normal_log_prob(loc, scale, u) - logp_behaviour)
    policy_loss = -torch.minimum(rho * adv, torch.clamp(rho, 1.0 - clipping_epsilon, 1.0 + clipping_epsilon) * adv).mean()
    value_loss = 0.25 * ((vs - values) ** 2).mean()
    entropy_loss = -entropy_cost * tanh_normal_entropy(loc, scale, loc + scale * entropy_noise).mean()
    return policy_loss + value_loss + entropy_loss, {"policy_loss": policy_loss.detach(), "value_loss": value_loss.detach(),
                                                     "entropy_loss": entropy_loss.detach()}


def _mlp(sizes, gen, device):
    """A swish MLP as plain parameter lists, kernels [in, out] (the layout myo_policy_update takes), lecun-uniform kernels and zero biases
    as in brax's networks."""
    import torch
    ws, bs = [], []
    for nin, nout in zip(sizes[:-1], sizes[1:]):
        lim = math.sqrt(3.0 / nin)
        w = (torch.rand((nin, nout), generator=gen, dtype=torch.float32) * 2.0 - 1.0) * lim
        ws.append(w.to(device).requires_grad_())
        bs.append(torch.zeros(nout, dtype=torch.float32, device=device, requires_grad=True))
    return ws, bs


def init_networks(obs_dim, act_dim, policy_hidden, value_hidden, seed, device="cpu"):
    """(policy kernels, policy biases, value kernels, value biases) as `train` starts from them: drawn on the host from `seed`, so the
    same for every backend."""
    import torch
    gen = torch.Generator().manual_seed(int(seed))
    pw, pb = _mlp([obs_dim, *policy_hidden, 2 * act_dim], gen, device)
    vw, vb = _mlp([obs_dim, *value_hidden, 1], gen, device)
    return pw, pb, vw, vb


def mlp_forward(x, ws, bs):
    import torch
    for i, (w, b) in enumerate(zip(ws, bs)):
        x = x @ w + b
        if i + 1 < len(ws):
            x = x * torch.sigmoid(x)
    return x


def policy_forward(obs, mean, std, ws, bs):
    """(loc, scale) of the tanh-normal head for observations obs [..., obs_dim]: the network `BraxPolicy` runs, in torch."""
    import torch
    loc, raw = torch.chunk(mlp_forward((obs - mean) / std, ws, bs), 2, dim=-1)
    return loc, torch.nn.functional.softplus(raw) + 0.001


def _check(env, unroll_length, num_minibatches, action_repeat, policy_hidden, episode_length):
    B = int(env.num_envs)
    if num_minibatches < 1 or B % num_minibatches:
        raise ValueError(f"num_envs = {B} is not a multiple of num_minibatches = {num_minibatches}")
    if unroll_length < 1:
        raise ValueError(f"unroll_length must be at least 1, got {unroll_length}")
    if action_repeat < 1:
        raise ValueError(f"action_repeat must be at least 1, got {action_repeat}")
    if len(policy_hidden) + 1 > MAX_LAYERS:
        raise ValueError(f"the policy kernel runs at most {MAX_LAYERS} layers, policy_hidden has {len(policy_hidden)} + the head")
    if any(h < 1 or h > MAX_WIDTH for h in (*policy_hidden, 2 * int(env.act_dim))):
        raise ValueError(f"the policy kernel's layers are 1..{MAX_WIDTH} wide, got {tuple(policy_hidden)} and a head of {2 * int(env.act_dim)}")
    if int(env.obs_dim) > MAX_OBS_DIM:
        raise ValueError(f"obs_dim = {env.obs_dim} is wider than the policy kernel's LDS tile ({MAX_OBS_DIM} floats)")
    limit = getattr(env, "max_episode_steps", None)
    if episode_length is not None and limit is not None and int(episode_length) != int(limit):
        raise ValueError(f"episode_length = {episode_length}, but the env ends its episodes after {limit} steps: the time limit belongs to "
                         "the env here, give it to make(..., max_episode_steps=...)")


def params_dict(stats, pw, pb, vw, vb):
    """The trainer's parameters as numpy arrays under the names `save` writes."""
    out = {"obs_mean": stats.mean, "obs_std": stats.std}
    out.update({f"w{i}": w for i, w in enumerate(pw)})
    out.update({f"b{i}": b for i, b in enumerate(pb)})
    out.update({f"vw{i}": w for i, w in enumerate(vw)})
    out.update({f"vb{i}": b for i, b in enumerate(vb)})
    out = {k: v.detach().cpu().numpy().astype(np.float32) for k, v in out.items()}
    out["obs_count"] = np.float32(stats.count)
    return out


class Learner:
    """The device learner (include/myo_hip_ppo.h): both networks' parameters, their gradients and Adam's moments live in the library, and
    `step` is one whole minibatch SGD step -- what one pass of `train`'s inner loop does with torch autograd and `torch.optim.Adam` -- as
    HIP kernels on torch's current stream, without allocation or host synchronisation.

    pw, pb, vw, vb: the initial parameters as `init_networks` returns them (any device; kernels [in, out]).  max_unroll and max_minibatch
    size the workspace: `step` takes any T <= max_unroll and any number of unrolls <= max_minibatch.  Hyperparameters: learning_rate,
    beta1, beta2, adam_eps (torch.optim.Adam's), discounting, gae_lambda, clipping_epsilon, entropy_cost, reward_scaling,
    normalize_advantage, with `train`'s defaults.  Layer widths 1..MAX_WIDTH, at most MAX_LAYERS layers per network, any obs_dim.
    NaNs in the inputs end up in the parameters, as they do with torch."""

    WHICH = {"param": 0, "grad": 1, "m": 2, "v": 3}

    def __init__(self, obs_dim, act_dim, pw, pb, vw, vb, max_unroll, max_minibatch, *, learning_rate=3e-4, beta1=0.9, beta2=0.999,
                 adam_eps=1e-8, discounting=0.95, gae_lambda=0.95, clipping_epsilon=0.3, entropy_cost=1e-3, reward_scaling=5.0,
                 normalize_advantage=True, device=0):
        self.h = None
        host = [[capi._f32(a.detach().cpu().numpy() if hasattr(a, "detach") else a) for a in group] for group in (pw, pb, vw, vb)]
        if len(host[0]) != len(host[1]) or len(host[2]) != len(host[3]) or not host[0] or not host[2]:
            raise ValueError("Learner: one bias per kernel, at least one layer per network")
        self.obs_dim, self.act_dim, self.device = int(obs_dim), int(act_dim), int(device)
        self.max_unroll, self.max_minibatch = int(max_unroll), int(max_minibatch)
        sizes = []
        for ws, bs in ((host[0], host[1]), (host[2], host[3])):
            nin = self.obs_dim
            for w, b in zip(ws, bs):
                if w.ndim != 2 or w.shape[0] != nin or b.shape != (w.shape[1],):
                    raise ValueError(f"Learner: kernel {w.shape} / bias {b.shape} do not continue a layer input of {nin}")
                nin = w.shape[1]
            sizes.append([w.shape[1] for w in ws])
        cfg = capi.LearnerConfig(obs_dim=self.obs_dim, act_dim=self.act_dim, policy_nlayers=len(sizes[0]), value_nlayers=len(sizes[1]),
                                 max_unroll=self.max_unroll, max_minibatch=self.max_minibatch, learning_rate=learning_rate, beta1=beta1,
                                 beta2=beta2, adam_eps=adam_eps, discounting=discounting, gae_lambda=gae_lambda,
                                 clipping_epsilon=clipping_epsilon, entropy_cost=entropy_cost, reward_scaling=reward_scaling,
                                 normalize_advantage=int(bool(normalize_advantage)))
        for k in range(min(8, len(sizes[0]))):
            cfg.policy_out[k] = sizes[0][k]
        for k in range(min(8, len(sizes[1]))):
            cfg.value_out[k] = sizes[1][k]
        arrs = [(C.POINTER(C.c_float) * len(g))(*(capi._ptr(a) for a in g)) for g in host]
        h = C.c_void_p()
        capi._chk(capi.lib().myo_ppo_learner_create(self.device, C.byref(cfg), *arrs, C.byref(h)))
        self.h = h
        self.sizes = sizes
        self._views = {}

    def __del__(self):
        try:
            if self.h:
                capi.lib().myo_ppo_learner_free(self.h)
                self.h = None
        except Exception:
            pass

    def step_rc(self, obs_buf, u_buf, logp_buf, rew_buf, term_buf, trunc_buf, idx, mean, std, noise, loss_sums=None, T=None, mb=None):
        """`step` without the check of the return code and of the tensors' shapes: pointers as given (None is NULL), T and mb as given."""
        import torch
        ptr = lambda a: None if a is None else a.data_ptr()
        T = u_buf.shape[0] if T is None else T
        mb = idx.shape[0] if mb is None else mb
        B = u_buf.shape[1] if u_buf is not None else 0
        with torch.cuda.device(self.device):
            return capi.lib().myo_ppo_learner_step(self.h, ptr(obs_buf), ptr(u_buf), ptr(logp_buf), ptr(rew_buf), ptr(term_buf), ptr(trunc_buf),
                                                   int(T), int(B), ptr(idx), int(mb), ptr(mean), ptr(std), ptr(noise), ptr(loss_sums),
                                                   torch.cuda.current_stream().cuda_stream)

    def step(self, obs_buf, u_buf, logp_buf, rew_buf, term_buf, trunc_buf, idx, mean, std, noise, loss_sums=None):
        """One SGD step on the unrolls `idx` of a rollout.  Contiguous float32 CUDA tensors: obs_buf [T + 1, B, obs_dim], u_buf [T, B,
        act_dim], logp_buf / rew_buf / term_buf / trunc_buf [T, B], mean / std [obs_dim], noise [T, mb, act_dim]; idx: mb int64 env columns
        without repeats (a slice of a permutation is fine).  loss_sums: 3 floats to which the step's policy, value and entropy loss are
        added on the device, or None."""
        import torch
        T, B, mb = u_buf.shape[0], u_buf.shape[1], idx.shape[0]
        want = [(obs_buf, (T + 1, B, self.obs_dim)), (u_buf, (T, B, self.act_dim)), (logp_buf, (T, B)), (rew_buf, (T, B)), (term_buf, (T, B)),
                (trunc_buf, (T, B)), (mean, (self.obs_dim,)), (std, (self.obs_dim,)), (noise, (T, mb, self.act_dim))]
        if loss_sums is not None:
            want.append((loss_sums, (3,)))
        for a, shape in want:
            if not a.is_cuda or a.dtype != torch.float32 or not a.is_contiguous() or tuple(a.shape) != shape:
                raise ValueError(f"Learner.step: a contiguous float32 CUDA tensor of shape {shape} is needed, got {a.dtype} {tuple(a.shape)}")
        if not idx.is_cuda or idx.dtype != torch.int64 or idx.dim() != 1 or not idx.is_contiguous():
            raise ValueError("Learner.step: idx is a contiguous int64 CUDA vector")
        capi._chk(self.step_rc(obs_buf, u_buf, logp_buf, rew_buf, term_buf, trunc_buf, idx, mean, std, noise, loss_sums))

    def tensors(self, which="param"):
        """(pw, pb, vw, vb): lists of torch views (zero copy, cached) of the learner's own buffers; which = "param", "grad" (of the last
        step), "m" or "v" (Adam's moments)."""
        import torch
        if which not in self._views:
            L, out = capi.lib(), []
            for net in (0, 1):
                nin = self.obs_dim
                ws, bs = [], []
                for layer, nout in enumerate(self.sizes[net]):
                    for what, shape, dst in ((0, (nin, nout), ws), (1, (nout,), bs)):
                        p, n = C.c_void_p(), C.c_size_t()
                        capi._chk(L.myo_ppo_learner_tensor(self.h, net, layer, what, self.WHICH[which], C.byref(p), C.byref(n)))
                        assert n.value == int(np.prod(shape))
                        dst.append(capi.device_view(torch, p.value, shape, np.float32, self, self.device))
                    nin = nout
                out += [ws, bs]
            self._views[which] = tuple(out)
        return self._views[which]

    def params_dict(self, stats):
        """What `params_dict` gives, from the learner's parameters."""
        return params_dict(stats, *self.tensors("param"))


def save(path, params):
    """Writes the `.npz` that `BraxPolicy.from_npz` reads (obs_mean, obs_std, obs_count, w*, b*), the value network under vw* / vb*."""
    np.savez(path, **{k: np.asarray(v, np.float32) for k, v in params.items()})


def train(env, num_timesteps, episode_length=None, unroll_length=50, num_minibatches=32, num_updates_per_batch=8, discounting=0.95,
          gae_lambda=0.95, learning_rate=3e-4, entropy_cost=1e-3, clipping_epsilon=0.3, reward_scaling=5.0, normalize_observations=True,
          normalize_advantage=True, action_repeat=1, policy_hidden=(32, 32, 32, 32), value_hidden=(256,) * 5, seed=1, progress_fn=None,
          backend=None, keep_first_rollout=False, update=None):
    """PPO on a batched env; returns (BraxPolicy or None, params, metrics).  The argument names and defaults are those of the reference's
    `mjx/ppo_continuous_action.py`, with brax's defaults for what that script leaves unset.

    env: any object with num_envs, obs_dim, act_dim, reset(seed) -> obs [B, obs_dim] and a gym-order step(action) -> (obs, reward,
    terminated, truncated, info) that resets finished episodes in place (`BatchedMyoEnv`, `make(<MyoDM id>, autoreset=True)`; terminated
    and truncated are cast to bool).  backend: "hip" (CUDA observations: sampling, GAE and the weight refresh are HIP kernels and a
    `BraxPolicy` is returned), "torch" (everything in torch on the observations' device; returns None for the policy), None: "hip" when
    the env's observations are CUDA tensors.

    One iteration: (1) unroll_length steps, each one sample launch, one env.step and copies into preallocated [T(+1), B, ...] buffers, with
    no host synchronisation; (2) the running observation statistics take the T * B observations and go to the device policy; (3)
    num_updates_per_batch epochs, each a fresh permutation of the B unrolls into num_minibatches groups, one Adam step per group on
    `loss`; (4) the policy's parameters go to the device policy.  num_timesteps is rounded up to whole iterations of
    num_envs * unroll_length * action_repeat env steps.

    action_repeat = k: k env steps on one action; rewards are summed up to and including the first step that ends the episode,
    termination and truncation are OR-ed.  brax's wrappers reset outside the repeat; here the env has already reset in place, so the
    remaining k - 1 steps run in the new episode and are not counted.
    episode_length: the env's own time limit is what ends episodes; a different value here is refused.

    Not taken: batch_size (it is num_envs / num_minibatches here: every iteration uses all envs), num_evals (episode statistics come from
    the training rollouts, through progress_fn), max_devices_per_host (one GPU; sharding a learner is out of scope).

    progress_fn(num_steps, metrics) is called once per iteration, like the reference's callback; metrics holds "eval/episode_reward"
    and "eval/episode_length" (means over the episodes that ended in the iteration, nan when none did), "episodes", "policy_loss",
    "value_loss", "entropy_loss", "steps_per_s", "rollout_s" and "update_s".  The list of all of them is returned.
    keep_first_rollout adds host copies of the first unroll's buffers (obs, u, logp, reward) to the first metrics record.

    update: None or "torch": step (3) is torch autograd and torch.optim.Adam on `loss`.  "hip" (opt-in, needs backend "hip"): the
    parameters live in a `Learner` and each SGD step is one `Learner.step`; no torch optimiser is built.  The permutation and the entropy
    noise are drawn from the same generator in the same order either way, the loss sums stay on the device until the iteration's one
    read, and the device policy is refreshed from the learner's parameter views."""
    import torch
    if update not in (None, "torch", "hip"):
        raise ValueError(f"update {update!r}: None, 'torch' or 'hip'")
    _check(env, unroll_length, num_minibatches, action_repeat, policy_hidden, episode_length)
    B, D, A, T = int(env.num_envs), int(env.obs_dim), int(env.act_dim), int(unroll_length)
    obs = torch.as_tensor(env.reset(seed=seed))
    dev = obs.device
    if backend is None:
        backend = "hip" if obs.is_cuda else "torch"
    if backend not in ("hip", "torch") or (backend == "hip" and not obs.is_cuda):
        raise ValueError(f"backend {backend!r}: 'hip' needs an env whose observations are CUDA tensors, else 'torch'")
    hip = backend == "hip"
    if update == "hip" and not hip:
        raise ValueError("update 'hip' needs backend 'hip' (an env whose observations are CUDA tensors)")
    dgen = torch.Generator(device=dev).manual_seed(int(seed))       # permutations, entropy noise, the torch backend's action noise
    pw, pb, vw, vb = init_networks(D, A, policy_hidden, value_hidden, seed, dev)
    stats = RunningStats(D, dev)
    learner = opt = None
    if update == "hip":
        learner = Learner(D, A, pw, pb, vw, vb, T, B // num_minibatches, learning_rate=learning_rate, discounting=discounting,
                          gae_lambda=gae_lambda, clipping_epsilon=clipping_epsilon, entropy_cost=entropy_cost, reward_scaling=reward_scaling,
                          normalize_advantage=normalize_advantage, device=dev.index or 0)
    else:
        opt = torch.optim.Adam([*pw, *pb, *vw, *vb], lr=learning_rate)
    pol = None
    if hip:
        from .policy import BraxPolicy
        pol = BraxPolicy(stats.mean.cpu().numpy(), stats.std.cpu().numpy(), [w.detach().cpu().numpy() for w in pw],
                         [b.detach().cpu().numpy() for b in pb], device=dev.index or 0)
    f32 = dict(dtype=torch.float32, device=dev)
    obs_buf, u_buf, logp_buf = torch.empty((T + 1, B, D), **f32), torch.empty((T, B, A), **f32), torch.empty((T, B), **f32)
    rew_buf, term_buf, trunc_buf = torch.empty((T, B), **f32), torch.empty((T, B), **f32), torch.empty((T, B), **f32)
    act_buf = torch.empty((B, A), **f32)
    ep_ret, ep_len = torch.zeros(B, **f32), torch.zeros(B, **f32)
    mb = B // num_minibatches
    steps_per_iter = B * T * action_repeat
    iterations = max(1, -(-int(num_timesteps) // steps_per_iter))
    metrics, draws = [], 0
    sync = torch.cuda.synchronize if obs.is_cuda else (lambda: None)

    for it in range(iterations):
        sync()
        t0 = time.perf_counter()
        done_ret, done_len, done_n = torch.zeros((), **f32), torch.zeros((), **f32), torch.zeros((), **f32)
        # (1) the unroll
        for t in range(T):
            obs_buf[t].copy_(obs)
            if hip:
                pol.sample(obs_buf[t].data_ptr(), B, act_buf.data_ptr(), u_buf[t].data_ptr(), logp_buf[t].data_ptr(), int(seed), draws,
                           stream=torch.cuda.current_stream().cuda_stream)
            else:
                with torch.no_grad():
                    loc, scale = policy_forward(obs_buf[t], stats.mean, stats.std, pw, pb)
                    u_buf[t] = loc + scale * torch.randn(loc.shape, generator=dgen, **f32)
                    logp_buf[t] = tanh_normal_log_prob(loc, scale, u_buf[t])
                    act_buf.copy_(torch.tanh(u_buf[t]))
            draws += 1
            for k in range(action_repeat):
                obs, r, term, trunc, _ = env.step(act_buf)
                term, trunc = torch.as_tensor(term).to(torch.bool), torch.as_tensor(trunc).to(torch.bool)
                if k == 0:
                    rew_buf[t].copy_(r)
                    term_buf[t].copy_(term)
                    trunc_buf[t].copy_(trunc)
                    ep_len += 1
                else:
                    live = 1.0 - torch.maximum(term_buf[t], trunc_buf[t])      # envs whose episode has not ended within this repeat
                    rew_buf[t] += r * live
                    term_buf[t] = torch.maximum(term_buf[t], term * live)
                    trunc_buf[t] = torch.maximum(trunc_buf[t], trunc * live)
                    ep_len += live
            ep_ret += rew_buf[t]
            done = torch.maximum(term_buf[t], trunc_buf[t])
            done_ret += (ep_ret * done).sum()
            done_len += (ep_len * done).sum()
            done_n += done.sum()
            ep_ret *= 1.0 - done
            ep_len *= 1.0 - done
        obs = torch.as_tensor(obs)
        obs_buf[T].copy_(obs)
        sync()
        t1 = time.perf_counter()
        # (2) observation statistics
        if normalize_observations:
            stats.update(obs_buf[:T])
            if hip:
                pol.update(obs_mean=stats.mean.contiguous(), obs_std=stats.std.contiguous())
        # (3) SGD
        sums = {k: torch.zeros((), **f32) for k in ("policy_loss", "value_loss", "entropy_loss")}
        dev_sums = torch.zeros(3, **f32) if learner is not None else None
        for _ in range(num_updates_per_batch):
            perm = torch.randperm(B, generator=dgen, device=dev)
            for g in range(num_minibatches):
                idx = perm[g * mb:(g + 1) * mb]
                if learner is not None:
                    noise = torch.randn((T, mb, A), generator=dgen, **f32)
                    learner.step(obs_buf, u_buf, logp_buf, rew_buf, term_buf, trunc_buf, idx, stats.mean, stats.std, noise, dev_sums)
                    continue
                o = obs_buf[:, idx]
                loc, scale = policy_forward(o[:T], stats.mean, stats.std, pw, pb)
                v = mlp_forward((o - stats.mean) / stats.std, vw, vb).squeeze(-1)
                noise = torch.randn((T, mb, A), generator=dgen, **f32)
                total, terms = loss(loc, scale, v[:T], v[T], u_buf[:, idx], logp_buf[:, idx], rew_buf[:, idx], term_buf[:, idx],
                                    trunc_buf[:, idx], noise, discounting=discounting, gae_lambda=gae_lambda,
                                    clipping_epsilon=clipping_epsilon, entropy_cost=entropy_cost, reward_scaling=reward_scaling,
                                    normalize_advantage=normalize_advantage)
                opt.zero_grad(set_to_none=True)
                total.backward()
                opt.step()
                for k2 in sums:
                    sums[k2] += terms[k2]
        # (4) the new weights go to the device policy
        if learner is not None:
            lw, lb, _, _ = learner.tensors("param")
            pol.update(kernels=lw, biases=lb)
            sums = dict(zip(sums, dev_sums))
        elif hip:
            pol.update(kernels=[w.data for w in pw], biases=[b.data for b in pb])
        # one read of the iteration's numbers
        nsgd = num_updates_per_batch * num_minibatches
        host = torch.stack([done_ret, done_len, done_n, *(sums[k2] / nsgd for k2 in sums)]).cpu().tolist()
        t2 = time.perf_counter()
        n = host[2]
        m = {"eval/episode_reward": host[0] / n if n else float("nan"), "eval/episode_length": host[1] / n if n else float("nan"),
             "episodes": int(n), "policy_loss": host[3], "value_loss": host[4], "entropy_loss": host[5],
             "steps_per_s": steps_per_iter / (t2 - t0), "rollout_s": t1 - t0, "update_s": t2 - t1}
        if it == 0 and keep_first_rollout:     # host copies of the first unroll, for reproducibility checks
            m["first_rollout"] = {"obs": obs_buf.cpu().numpy(), "u": u_buf.cpu().numpy(), "logp": logp_buf.cpu().numpy(),
                                  "reward": rew_buf.cpu().numpy()}
        metrics.append(m)
        if progress_fn is not None:
            progress_fn((it + 1) * steps_per_iter, m)
    return pol, learner.params_dict(stats) if learner is not None else params_dict(stats, pw, pb, vw, vb), metrics
