"""RecurrentPPO's update written again, from the formulas and not from cantorrl_amd/train.py: the obs
normalisation (contract step 2), the two LSTMs as sb3_contrib's loop of one cell per step, the MLPs, the
Gaussian log-probability and entropy, sb3_contrib 2.6.0 RecurrentPPO.train's loss with its statistics
and SB3 2.6.0's value clip, the loss's closed-form gradients in NumPy f64, and ppo_update's loop over
epochs, env groups and time windows with the gradient-norm clip and SGD or Adam (contract O5) in formulas,
with the preconditions under which an f32 run takes the f64 run's branches, measured on the two replays.

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


MISTAKES = ("no_vf_clip", "vf_max_of_both", "old_values_first_window", "old_values_unpermuted", "biased_std",
            "normalize_dropped", "clip_before_sum")   # what replay(mistake=...) can get wrong on purpose


def loss(values, log_prob, entropy, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef,
         normalize_advantage=True, clip_range_vf=None, old_values=None, mistake=None):
    """sb3_contrib 2.6.0 RecurrentPPO.train's loss for one minibatch, mask all ones, the means as sums
    over N -> (loss, statistics); statistics["ratio"], ["adv"]: the rows' r and A.  clip_range_vf (None:
    no value clip) is SB3 2.6.0's: values_pred = old_values + clamp(values - old_values, -c, c), then the
    mean squared error against returns; statistics["dv"]: the rows' values - old_values (with old_values),
    ["vf_clip_fraction"]: the share of rows with |dv| > c.  mistake: one of MISTAKES, for the sensitivity
    tests (the loss's: no_vf_clip, vf_max_of_both, biased_std, normalize_dropped)."""
    N = values.numel()
    A = advantages
    if normalize_advantage and mistake != "normalize_dropped":
        mean = A.sum() / N
        std = (((A - mean) ** 2).sum() / (N if mistake == "biased_std" else N - 1)).sqrt()   # unbiased
        A = (A - mean) / (std + 1e-8)
    r = torch.exp(log_prob - old_log_prob)
    lo, hi = 1.0 - clip_range, 1.0 + clip_range
    clamped = torch.where(r > hi, torch.full_like(r, hi), torch.where(r < lo, torch.full_like(r, lo), r))
    s1, s2 = A * r, A * clamped
    policy = -torch.where(s2 < s1, s2, s1).sum() / N
    dv = None if old_values is None else values - old_values
    if clip_range_vf is None or mistake == "no_vf_clip":
        value = ((returns - values) ** 2).sum() / N
    else:
        c = float(clip_range_vf)
        moved = torch.where(dv > c, torch.full_like(dv, c), torch.where(dv < -c, torch.full_like(dv, -c), dv))
        e_clipped = (returns - (old_values + moved)) ** 2
        if mistake == "vf_max_of_both":   # PPO2's, not SB3's
            e = (returns - values) ** 2
            e_clipped = torch.where(e > e_clipped, e, e_clipped)
        value = e_clipped.sum() / N
    entropy_loss = -(entropy.sum() / N)
    total = policy + ent_coef * entropy_loss + vf_coef * value
    with torch.no_grad():
        stats = dict(loss=total.detach(), policy_gradient_loss=policy.detach(), value_loss=value.detach(),
                     entropy_loss=entropy_loss.detach(), approx_kl=((r - 1.0) - torch.log(r)).sum() / N,
                     clip_fraction=((r - 1.0).abs() > clip_range).sum().to(r.dtype) / N, ratio=r.detach(), adv=A.detach())
        if dv is not None:
            stats["dv"] = dv.detach()
            if clip_range_vf is not None:
                stats["vf_clip_fraction"] = (dv.abs() > float(clip_range_vf)).sum().to(r.dtype) / N
    return total, stats


def loss_numpy(values, log_prob, entropy, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef,
               normalize_advantage=True, clip_range_vf=None, old_values=None):
    """The same loss over flat f64 NumPy arrays, no autograd -> (statistics, gradients): the six
    statistics as floats plus "ratio" and "adv" (and "dv", "vf_clip_fraction" with a value clip); the
    closed-form dL/dvalues, dL/dlog_prob, dL/dentropy."""
    v, lp, ent, old, A, ret = (np.asarray(t, np.float64).reshape(-1) for t in
                               (values, log_prob, entropy, old_log_prob, advantages, returns))
    N, c = v.size, float(clip_range)
    if normalize_advantage:
        mean = A.sum() / N
        A = (A - mean) / (math.sqrt(((A - mean) ** 2).sum() / (N - 1)) + 1e-8)
    r = np.exp(lp - old)
    s1, s2 = A * r, A * np.minimum(np.maximum(r, 1.0 - c), 1.0 + c)
    policy = -np.minimum(s1, s2).sum() / N
    extra, pred, passes = {}, v, 1.0
    if clip_range_vf is not None:
        ov, cv = np.asarray(old_values, np.float64).reshape(-1), float(clip_range_vf)
        dv = v - ov
        pred, passes = ov + np.minimum(np.maximum(dv, -cv), cv), np.abs(dv) <= cv   # clamp passes gradient on its edges
        extra = dict(dv=dv, vf_clip_fraction=float((np.abs(dv) > cv).sum()) / N)
    value = ((ret - pred) ** 2).sum() / N
    entropy_loss = -(ent.sum() / N)
    stats = dict(loss=policy + ent_coef * entropy_loss + vf_coef * value, policy_gradient_loss=policy, value_loss=value,
                 entropy_loss=entropy_loss, approx_kl=((r - 1.0) - np.log(r)).sum() / N,
                 clip_fraction=float((np.abs(r - 1.0) > c).sum()) / N, ratio=r, adv=A, **extra)
    active = np.where(A >= 0.0, r < 1.0 + c, r > 1.0 - c)
    grads = dict(values=-2.0 * vf_coef * (ret - pred) * passes / N, log_prob=-A * r * active / N,
                 entropy=np.full(N, -ent_coef / N))
    return stats, grads


def window(buffer, idx, k0, W):
    """Envs idx x steps [k0, k0 + W) of a RolloutBuffer, indexed straight from its tensors, and the
    states before step k0: buffer.h_pi ... at k0 = 0, buffer.states[k0] otherwise."""
    mb = {name: getattr(buffer, name)[k0:k0 + W][:, idx]
          for name in ("observations", "actions", "episode_starts", "log_probs", "advantages", "returns", "values")}
    if k0 == 0:
        mb["states0"] = tuple(getattr(buffer, s)[idx] for s in STATES)
    else:
        mb["states0"] = tuple(buffer.states[k0][idx][:, i] for i in range(4))
    return mb


def replay(params, buffer, dtype, optimizer, lr, n_epochs, per, W, seed, hyper, const, trace=None,
           clip_range_vf=None, normalize_advantage=True, mistake=None):
    """ppo_update's loop written again: per epoch one torch.randperm(n) from a generator seeded with
    `seed` on the buffer's device, groups of `per` envs (a short last one), windows of W steps, the
    restated loss, torch.autograd.grad, the clip c = min(1, max_norm / (norm + 1e-6)) over all the
    tensors, then optimizer "sgd" (p -= lr g) or "adam" (contract O5's formulas: betas 0.9 / 0.999,
    eps 1e-5, bias corrections from the step count), all in `dtype`.  params: {name: tensor}, const:
    constants(policy), hyper: clip_range, ent_coef, vf_coef, max_grad_norm.  clip_range_vf: SB3's value
    clip against the rollout's values of the minibatch's rows, buffer.values[k0:k0 + W][:, idx].  trace:
    a list that receives per minibatch the rows' ratio, A and dv = values - old_values, the clip fraction
    and (with a value clip) the value-clipped fraction.  mistake: one of MISTAKES.  -> {name: f64 tensor}."""
    if mistake is not None and mistake not in MISTAKES:
        raise ValueError(mistake)
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
                old_values = mb["values"]
                if mistake == "old_values_first_window":
                    old_values = buffer.values[0:W][:, idx]
                elif mistake == "old_values_unpermuted":
                    old_values = buffer.values[k0:k0 + W][:, lo:lo + len(idx)]
                leaves = {k: x.clone().requires_grad_() for k, x in p.items()}
                values, log_prob, entropy = evaluate(leaves, const, mb["observations"], mb["actions"],
                                                     mb["episode_starts"], mb["states0"])
                total, stats = loss(values, log_prob, entropy, mb["log_probs"].to(dtype), mb["advantages"].to(dtype),
                                    mb["returns"].to(dtype), hyper["clip_range"], hyper["ent_coef"], hyper["vf_coef"],
                                    normalize_advantage, clip_range_vf, old_values.to(dtype), mistake)
                grads = dict(zip(names, torch.autograd.grad(total, [leaves[k] for k in names])))
                norm = torch.sqrt(sum((g * g).sum() for g in grads.values()))
                c = torch.clamp(hyper["max_grad_norm"] / (norm + 1e-6), max=1.0)
                t += 1
                for k in names:
                    g = grads[k] * c
                    if mistake == "clip_before_sum":   # one norm per tensor
                        g = grads[k] * torch.clamp(hyper["max_grad_norm"] / (torch.sqrt((grads[k] * grads[k]).sum()) + 1e-6),
                                                   max=1.0)
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
                    trace.append(dict(ratio=stats["ratio"].cpu(), adv=stats["adv"].cpu(), dv=stats["dv"].cpu(),
                                      clip_fraction=float(stats["clip_fraction"]), grad_norm=float(norm),
                                      vf_clip_fraction=float(stats["vf_clip_fraction"]) if clip_range_vf is not None else None))
    return {k: x.to(torch.float64) for k, x in p.items()}


def replay_margins(trace, trace32, clip_range, clip_range_vf=None):
    """What the preconditions are measured on, from the all-torch replay's two traces alone (f64, and f32
    or None): d_ratio, d_dv = the largest |f32 - f64| of a row's ratio and dv over all minibatches (0
    without an f32 trace); edge, vf_edge = the f64 rows' smallest distance of the ratio from 1 +-
    clip_range and of |dv| from clip_range_vf (inf without a value clip); small = the smallest |A|;
    fractions, vf_fractions = the clipped shares per minibatch."""
    m = dict(d_ratio=0.0, d_dv=0.0, vf_edge=math.inf, vf_fractions=[])
    if trace32 is not None:
        assert len(trace32) == len(trace)
        m["d_ratio"] = max(float((a["ratio"].double() - b["ratio"]).abs().max()) for a, b in zip(trace32, trace))
        m["d_dv"] = max(float((a["dv"].double() - b["dv"]).abs().max()) for a, b in zip(trace32, trace))
    m["edge"] = min(float(torch.minimum((s["ratio"] - (1 - clip_range)).abs(), (s["ratio"] - (1 + clip_range)).abs()).min())
                    for s in trace)
    m["small"] = min(float(s["adv"].abs().min()) for s in trace)
    m["fractions"] = [s["clip_fraction"] for s in trace]
    if clip_range_vf is not None:
        m["vf_edge"] = min(float((s["dv"].abs() - clip_range_vf).abs().min()) for s in trace)
        m["vf_fractions"] = [s["vf_clip_fraction"] for s in trace]
    return m


def describe_margins(m):
    return (f"d_ratio {m['d_ratio']:.2e} closest ratio to a clip edge {m['edge']:.2e}; d_dv {m['d_dv']:.2e} closest |dv| "
            f"to clip_range_vf {m['vf_edge']:.2e}; smallest |A| {m['small']:.2e}; clip fractions "
            + " ".join(f"{f:.2f}" for f in m["fractions"]) + "; value-clipped " + " ".join(f"{f:.2f}" for f in m["vf_fractions"]))


def check_replay_inputs(trace, clip_range, need_clipping=True, trace32=None, clip_range_vf=None):
    """The conditions under which an f32 run takes the f64 replay's branches, on the replay's own traces
    (never on the code under test): every f64 ratio at least max(1e-5, 4 d_ratio) from 1 +- clip_range,
    every f64 |dv| at least max(1e-5, 4 d_dv) from clip_range_vf, no |A| < 1e-5; d_ratio and d_dv are the
    f32 replay's distance from the f64 one (trace32; without it the margins are the fixed 1e-5).  The 4
    is the bound's: a route allowed 4 d_ref on parameters needs the same room before a branch.  Coverage:
    (unless exempt) a minibatch after the first with a clip fraction in [0.05, 0.95], and with a value
    clip at least two minibatches with a value-clipped fraction in [0.05, 0.95].
    -> (smallest edge distance, smallest |A|, fractions); replay_margins has the rest."""
    m = replay_margins(trace, trace32, clip_range, clip_range_vf)
    need = max(1e-5, 4 * m["d_ratio"])
    assert m["edge"] >= need, f"a ratio {m['edge']:.2e} from a clip edge, {need:.2e} needed: choose another seed"
    assert m["small"] >= 1e-5, f"|A| = {m['small']:.2e}: choose another seed"
    if need_clipping:
        assert any(0.05 <= f <= 0.95 for f in m["fractions"][1:]), m["fractions"]
    if clip_range_vf is not None:
        need = max(1e-5, 4 * m["d_dv"])
        assert m["vf_edge"] >= need, f"a |dv| {m['vf_edge']:.2e} from clip_range_vf, {need:.2e} needed: choose another"
        assert sum(0.05 <= f <= 0.95 for f in m["vf_fractions"]) >= 2, m["vf_fractions"]
    return m["edge"], m["small"], m["fractions"]


def replay_bound(p0, p32, p64, got, pooled=()):
    """Per tensor (name, err, d_ref, ulp): err = max |got - p64|, d_ref = max |p32 - p64|, ulp = 2^-23
    max |p0|.  `pooled`: groups of names whose d_ref is the largest of the group."""
    d = {k: float((p32[k] - p64[k]).abs().max()) for k in p64}
    for group in pooled:
        top = max(d[k] for k in group)
        d.update({k: top for k in group})
    return [(k, float((got[k].detach().to(p64[k].device, torch.float64) - p64[k]).abs().max()), d[k],
             2.0 ** -23 * float(p0[k].abs().max())) for k in p64]
