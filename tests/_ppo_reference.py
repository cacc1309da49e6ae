"""RecurrentPPO's update written again, from the formulas and not from cantorrl_amd/train.py: the obs
normalisation (contract step 2), the two LSTMs as sb3_contrib's loop of one cell per step, the MLPs, the
Gaussian log-probability and entropy, sb3_contrib 2.6.0 RecurrentPPO.train's loss with its statistics,
the loss's closed-form gradients in NumPy f64, and ppo_update's loop over epochs, env groups and time
windows with the gradient-norm clip and SGD or Adam (contract O5) in formulas.

Everything works on a dict of the 21 tensors under the checkpoint's names, in whatever dtype they
have.  Nothing here calls train.ppo_loss, RecurrentPPOModule.heads / .normalize_obs /
.evaluate_actions, train.minibatch or a torch optimizer: the tests compare those with this."""
import math

import numpy as np
import torch

from test_lstm_seq_cpu import torch_lstm_loop

HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
STATES = ("h_pi", "c_pi", "h_vf", "c_vf")
LSTM = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
ACTION_HEAD = ("action_net.weight", "action_net.bias", "log_std")
VALUE_HEAD = ("value_net.weight", "value_net.bias")


def constants(policy):
    """What is not a tensor of the state dict, from an agent.RecurrentPolicy or a RecurrentPPOModule:
    the activation and the obs statistics (mean, var as f64 tensors or None, epsilon, clip)."""
    arrays = getattr(policy, "_arrays", None)
    mean, var = (arrays.get("obs_mean"), arrays.get("obs_var")) if arrays is not None else (policy.obs_mean, policy.obs_var)
    if mean is not None:
        mean, var = (torch.as_tensor(v, dtype=torch.float64).detach().clone() for v in (mean, var))
    return dict(activation=policy.activation, mean=mean, var=var, epsilon=float(policy.epsilon), clip=policy.clip_obs)


def parameters(module, dtype):
    """The 21 tensors of a RecurrentPPOModule as fresh leaves in `dtype`."""
    return {k: p.detach().to(dtype).clone() for k, p in module.named_parameters()}


def normalize(obs, const):
    """Contract step 2: f32(clip((f64(obs) - mean) / sqrt(var + epsilon), +-clip)); obs as they are
    where the policy carries no statistics."""
    if const["mean"] is None:
        return obs
    mean, var = const["mean"].to(obs.device), const["var"].to(obs.device)
    q = (obs.to(torch.float64) - mean) / (var + const["epsilon"]).sqrt()
    if const["clip"] is not None:
        c = float(const["clip"])
        q = torch.where(q > c, torch.full_like(q, c), torch.where(q < -c, torch.full_like(q, -c), q))
    return q.to(torch.float32)


def mlp(h, params, prefix, activation):
    act = {"tanh": torch.tanh, "relu": lambda t: torch.where(t > 0, t, torch.zeros_like(t))}[activation]
    a = act(h @ params[prefix + ".0.weight"].t() + params[prefix + ".0.bias"])
    return act(a @ params[prefix + ".2.weight"].t() + params[prefix + ".2.bias"])


def heads(params, h_pi, h_vf, actions, activation):
    """values, log_prob, entropy [...] from the LSTMs' outputs [..., 128] and the actions [..., 2]."""
    a = mlp(h_pi, params, "mlp_extractor.policy_net", activation)
    mean = a @ params["action_net.weight"].t() + params["action_net.bias"]
    a = mlp(h_vf, params, "mlp_extractor.value_net", activation)
    values = (a @ params["value_net.weight"].t() + params["value_net.bias"])[..., 0]
    log_std = params["log_std"]
    z = (actions - mean) / torch.exp(log_std)
    log_prob = (-0.5 * z * z - log_std - HALF_LOG_2PI).sum(-1)
    entropy = (0.5 + HALF_LOG_2PI + log_std).sum(-1).expand(log_prob.shape)
    return values, log_prob, entropy


def evaluate(params, const, obs, actions, episode_starts, states0):
    """evaluate_actions over obs [L,B,13], actions [L,B,2], episode_starts [L,B] from states0 = (h_pi,
    c_pi, h_vf, c_vf) [B,128] -> (values, log_prob, entropy) [L,B] in the parameters' dtype."""
    dt = params["log_std"].dtype
    x = normalize(obs, const).to(dt)
    s = [t.to(dt) for t in states0]
    h_pi = torch_lstm_loop(x, episode_starts, s[0], s[1], *(params["lstm_actor." + k] for k in LSTM))
    h_vf = torch_lstm_loop(x, episode_starts, s[2], s[3], *(params["lstm_critic." + k] for k in LSTM))
    return heads(params, h_pi, h_vf, actions.to(dt), const["activation"])


def loss(values, log_prob, entropy, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef,
         normalize_advantage=True):
    """sb3_contrib 2.6.0 RecurrentPPO.train's loss for one minibatch, mask all ones, no clip_range_vf,
    the means as sums over N -> (loss, statistics); statistics["ratio"], ["adv"]: the rows' r and A."""
    N = values.numel()
    A = advantages
    if normalize_advantage:
        mean = A.sum() / N
        std = (((A - mean) ** 2).sum() / (N - 1)).sqrt()   # unbiased
        A = (A - mean) / (std + 1e-8)
    r = torch.exp(log_prob - old_log_prob)
    lo, hi = 1.0 - clip_range, 1.0 + clip_range
    clamped = torch.where(r > hi, torch.full_like(r, hi), torch.where(r < lo, torch.full_like(r, lo), r))
    s1, s2 = A * r, A * clamped
    policy = -torch.where(s2 < s1, s2, s1).sum() / N
    value = ((returns - values) ** 2).sum() / N
    entropy_loss = -(entropy.sum() / N)
    total = policy + ent_coef * entropy_loss + vf_coef * value
    with torch.no_grad():
        stats = dict(loss=total.detach(), policy_gradient_loss=policy.detach(), value_loss=value.detach(),
                     entropy_loss=entropy_loss.detach(), approx_kl=((r - 1.0) - torch.log(r)).sum() / N,
                     clip_fraction=((r - 1.0).abs() > clip_range).sum().to(r.dtype) / N, ratio=r.detach(), adv=A.detach())
    return total, stats


def loss_numpy(values, log_prob, entropy, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef,
               normalize_advantage=True):
    """The same loss over flat f64 NumPy arrays, no autograd -> (statistics, gradients): the six
    statistics as floats plus "ratio" and "adv"; the closed-form dL/dvalues, dL/dlog_prob, dL/dentropy."""
    v, lp, ent, old, A, ret = (np.asarray(t, np.float64).reshape(-1) for t in
                               (values, log_prob, entropy, old_log_prob, advantages, returns))
    N, c = v.size, float(clip_range)
    if normalize_advantage:
        mean = A.sum() / N
        A = (A - mean) / (math.sqrt(((A - mean) ** 2).sum() / (N - 1)) + 1e-8)
    r = np.exp(lp - old)
    s1, s2 = A * r, A * np.minimum(np.maximum(r, 1.0 - c), 1.0 + c)
    policy = -np.minimum(s1, s2).sum() / N
    value = ((ret - v) ** 2).sum() / N
    entropy_loss = -(ent.sum() / N)
    stats = dict(loss=policy + ent_coef * entropy_loss + vf_coef * value, policy_gradient_loss=policy, value_loss=value,
                 entropy_loss=entropy_loss, approx_kl=((r - 1.0) - np.log(r)).sum() / N,
                 clip_fraction=float((np.abs(r - 1.0) > c).sum()) / N, ratio=r, adv=A)
    active = np.where(A >= 0.0, r < 1.0 + c, r > 1.0 - c)
    grads = dict(values=-2.0 * vf_coef * (ret - v) / N, log_prob=-A * r * active / N,
                 entropy=np.full(N, -ent_coef / N))
    return stats, grads


def window(buffer, idx, k0, W):
    """Envs idx x steps [k0, k0 + W) of a RolloutBuffer, indexed straight from its tensors, and the
    states before step k0: buffer.h_pi ... at k0 = 0, buffer.states[k0] otherwise."""
    mb = {name: getattr(buffer, name)[k0:k0 + W][:, idx]
          for name in ("observations", "actions", "episode_starts", "log_probs", "advantages", "returns")}
    if k0 == 0:
        mb["states0"] = tuple(getattr(buffer, s)[idx] for s in STATES)
    else:
        mb["states0"] = tuple(buffer.states[k0][idx][:, i] for i in range(4))
    return mb


def replay(params, buffer, dtype, optimizer, lr, n_epochs, per, W, seed, hyper, const, trace=None):
    """ppo_update's loop written again: per epoch one torch.randperm(n) from a generator seeded with
    `seed` on the buffer's device, groups of `per` envs (a short last one), windows of W steps, the
    restated loss, torch.autograd.grad, the clip c = min(1, max_norm / (norm + 1e-6)) over all the
    tensors, then optimizer "sgd" (p -= lr g) or "adam" (contract O5's formulas: betas 0.9 / 0.999,
    eps 1e-5, bias corrections from the step count), all in `dtype`.  params: {name: tensor}, const:
    constants(policy), hyper: clip_range, ent_coef, vf_coef, max_grad_norm.  trace: a list that receives
    per minibatch the rows' ratio and A and the clip fraction.  -> {name: f64 tensor}."""
    p = {k: v.detach().to(dtype).clone() for k, v in params.items()}
    names = list(p)
    K, n = buffer.k_steps, buffer.n_envs
    dev = buffer.observations.device
    gen = torch.Generator(device=dev).manual_seed(seed)
    b1, b2, eps = 0.9, 0.999, 1e-5
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v2 = {k: torch.zeros_like(v) for k, v in p.items()}
    t = 0
    for _ in range(n_epochs):
        perm = torch.randperm(n, device=dev, generator=gen)
        for lo in range(0, n, per):
            idx = perm[lo:lo + per]
            for k0 in range(0, K, W):
                mb = window(buffer, idx, k0, W)
                leaves = {k: x.clone().requires_grad_() for k, x in p.items()}
                values, log_prob, entropy = evaluate(leaves, const, mb["observations"], mb["actions"],
                                                     mb["episode_starts"], mb["states0"])
                total, stats = loss(values, log_prob, entropy, mb["log_probs"].to(dtype), mb["advantages"].to(dtype),
                                    mb["returns"].to(dtype), hyper["clip_range"], hyper["ent_coef"], hyper["vf_coef"])
                grads = dict(zip(names, torch.autograd.grad(total, [leaves[k] for k in names])))
                norm = torch.sqrt(sum((g * g).sum() for g in grads.values()))
                c = torch.clamp(hyper["max_grad_norm"] / (norm + 1e-6), max=1.0)
                t += 1
                for k in names:
                    g = grads[k] * c
                    if optimizer == "sgd":
                        p[k] = p[k] - lr * g
                    elif optimizer == "adam":
                        m[k] = b1 * m[k] + (1.0 - b1) * g
                        v2[k] = b2 * v2[k] + (1.0 - b2) * (g * g)
                        denom = v2[k].sqrt() / math.sqrt(1.0 - b2 ** t) + eps
                        p[k] = p[k] - (lr / (1.0 - b1 ** t)) * (m[k] / denom)
                    else:
                        raise ValueError(optimizer)
                if trace is not None:
                    trace.append(dict(ratio=stats["ratio"].cpu(), adv=stats["adv"].cpu(),
                                      clip_fraction=float(stats["clip_fraction"])))
    return {k: x.to(torch.float64) for k, x in p.items()}


def check_replay_inputs(trace, clip_range, need_clipping=True):
    """The conditions under which an f32 run takes the f64 replay's branches, on the f64 trace: no
    ratio within 1e-5 of 1 +- clip_range, no |A| < 1e-5, and (unless exempt) a minibatch after the
    first with a clip fraction in [0.05, 0.95].  -> (smallest edge distance, smallest |A|, fractions)."""
    edge = min(float(torch.minimum((s["ratio"] - (1 - clip_range)).abs(), (s["ratio"] - (1 + clip_range)).abs()).min())
               for s in trace)
    small = min(float(s["adv"].abs().min()) for s in trace)
    fractions = [s["clip_fraction"] for s in trace]
    assert edge >= 1e-5, f"a ratio {edge:.2e} from a clip edge: choose another seed"
    assert small >= 1e-5, f"|A| = {small:.2e}: choose another seed"
    if need_clipping:
        assert any(0.05 <= f <= 0.95 for f in fractions[1:]), fractions
    return edge, small, fractions


def replay_bound(p0, p32, p64, got, pooled=()):
    """Per tensor (name, err, d_ref, ulp): err = max |got - p64|, d_ref = max |p32 - p64|, ulp = 2^-23
    max |p0|.  `pooled`: groups of names whose d_ref is the largest of the group."""
    d = {k: float((p32[k] - p64[k]).abs().max()) for k in p64}
    for group in pooled:
        top = max(d[k] for k in group)
        d.update({k: top for k in group})
    return [(k, float((got[k].detach().to(p64[k].device, torch.float64) - p64[k]).abs().max()), d[k],
             2.0 ** -23 * float(p0[k].abs().max())) for k in p64]
