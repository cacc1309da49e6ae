"""The PPO heads (include/hedge_actor.h, contract H1-H6) written again, for the tests of ha_ppo_heads_*:

* restate(): forward and backward in NumPy f64 from the formulas, closed form, with seven deliberate
  mistakes that the tests must catch;
* torch_reference(): tests/_ppo_reference.heads under torch.autograd.grad in a given dtype, the pre-activation
  gradients read off per-row copies of the biases; f64 is the reference, f32 gives d_ref;
* host_forward() / host_backward(): ha_host_ppo_heads_* over NumPy arrays through ctypes structs of their own
  (not train.py's), the outputs pre-filled so that a refusal shows them untouched;
* entropy_h3(), lsd_h6(): the two places where the contract fixes the bits without exp: H3's sum and H6's sum
  in L1's order (tests/_ppo_loss_contract.block_sum)."""
import ctypes

import numpy as np

import _ppo_loss_contract as lc
from cantorrl_amd import agent

F32, F64 = np.float32, np.float64
HALF_LOG_2PI = 0.9189385332046727
TENSORS = ("w1", "b1", "w2", "b2", "w3", "b3", "log_std", "v1", "vb1", "v2", "vb2", "v3", "vb3")
TENSOR_KEYS = ("mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias", "mlp_extractor.policy_net.2.weight",
               "mlp_extractor.policy_net.2.bias", "action_net.weight", "action_net.bias", "log_std",
               "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias", "mlp_extractor.value_net.2.weight",
               "mlp_extractor.value_net.2.bias", "value_net.weight", "value_net.bias")
FWD_IN = ("h_pi", "h_vf", "actions")
FWD_OUT = ("values", "log_prob", "entropy", "mean", "a1_pi", "a2_pi", "a1_vf", "a2_vf")
BWD_IN = ("d_values", "d_log_prob", "d_entropy", "actions", "mean", "a1_pi", "a2_pi", "a1_vf", "a2_vf")
BWD_OUT = ("d_h_pi", "d_h_vf", "d_z1_pi", "d_z2_pi", "d_z1_vf", "d_z2_vf", "d_mean", "d_log_std")
WIDTH = dict(h_pi=128, h_vf=128, actions=2, values=0, log_prob=0, entropy=0, mean=2, a1_pi=64, a2_pi=64, a1_vf=64,
             a2_vf=64, d_values=0, d_log_prob=0, d_entropy=0, d_h_pi=128, d_h_vf=128, d_z1_pi=64, d_z2_pi=64,
             d_z1_vf=64, d_z2_vf=64, d_mean=2)
MISTAKES = ("z_without_std", "lsd_missing_minus_one", "entropy_plus_one_dropped", "one_minus_a", "relu_ge",
            "w2_not_transposed", "critic_fed_h_pi")
MAX_ROWS = lc.BLOCK * lc.MAX_BLOCKS


class Weights(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in TENSORS] + [("activation", ctypes.c_int32)]


class Fwd(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in FWD_IN + FWD_OUT]


class Bwd(ctypes.Structure):
    _fields_ = [(k, ctypes.c_void_p) for k in BWD_IN + BWD_OUT]


def shape(name, R):
    if name == "d_log_std":
        return (2,)
    return (R, WIDTH[name]) if WIDTH[name] else (R,)


def policy_tensors(pol):
    """The 13 tensors of an agent.RecurrentPolicy as f32 arrays by TENSORS' names."""
    _, a = pol._host_weights()
    return {k: np.ascontiguousarray(a[k], F32).copy() for k in TENSORS}


def random_tensors(seed):
    """Uniform +-0.5 tensors, as test_policy_collect_cpu.random_policy_weights draws them."""
    rng = np.random.default_rng(seed)
    shapes = {f: s for _, f, s in agent.POLICY_KEYS}
    return {k: rng.uniform(-0.5, 0.5, shapes[k]).astype(F32) for k in TENSORS}


def rows(R, seed, scale=1.0):
    """h_pi, h_vf in +-1 (an LSTM's outputs), actions N(0, 1), and the three incoming gradients at the sizes
    ha_ppo_loss gives them for R rows."""
    rng = np.random.default_rng(seed)
    return dict(h_pi=rng.uniform(-1, 1, (R, 128)).astype(F32), h_vf=rng.uniform(-1, 1, (R, 128)).astype(F32),
                actions=(scale * rng.normal(0, 1, (R, 2))).astype(F32),
                d_values=(rng.normal(0, 1, R) / R).astype(F32), d_log_prob=(rng.normal(0, 1, R) / R).astype(F32),
                d_entropy=np.full(R, -1e-5 / R, F32))


def _call(fn, struct, w, activation, x, inputs, outputs, R, fill, n_rows, extra):
    ws = Weights()
    keep = []
    for k in TENSORS:
        if w[k] is None:
            setattr(ws, k, None)
            continue
        a = np.ascontiguousarray(w[k], F32)
        keep.append(a)
        setattr(ws, k, a.ctypes.data)
    ws.activation = {"tanh": 0, "relu": 1}.get(activation, activation)
    io = struct()
    for k in inputs:
        if x[k] is None:
            setattr(io, k, None)
            continue
        a = np.ascontiguousarray(x[k], F32)
        keep.append(a)
        setattr(io, k, a.ctypes.data)
    out = {k: np.full(shape(k, R), fill, F32) for k in outputs}
    for k, a in out.items():
        setattr(io, k, a.ctypes.data)
    for k, v in (extra or {}).items():
        setattr(io, k, v)
    st = fn(R if n_rows is None else n_rows, ctypes.byref(ws), ctypes.byref(io))
    return st, out


def host_forward(w, activation, x, fill=np.nan, n_rows=None, extra=None):
    """ha_host_ppo_heads_forward -> (status, {FWD_OUT}).  A tensor or input set to None is passed as NULL;
    extra: {field: raw pointer value} set last."""
    R = len(x["actions"]) if x.get("actions") is not None else len(x["h_pi"])
    return _call(agent.load().ha_host_ppo_heads_forward, Fwd, w, activation, x, FWD_IN, FWD_OUT, R, fill, n_rows, extra)


def host_backward(w, activation, x, fill=np.nan, n_rows=None, extra=None):
    """ha_host_ppo_heads_backward over x (BWD_IN) -> (status, {BWD_OUT})."""
    R = len(x["mean"])
    return _call(agent.load().ha_host_ppo_heads_backward, Bwd, w, activation, x, BWD_IN, BWD_OUT, R, fill, n_rows, extra)


def host_both(w, activation, x):
    """Forward, then backward on the forward's saved tensors -> one dict of every output."""
    st, f = host_forward(w, activation, x)
    assert st == 0
    st, b = host_backward(w, activation, dict(x, **f))
    assert st == 0
    return dict(f, **b)


# --------------------------------------------------------------------------- the restatement
def entropy_h3(log_std):
    """H3: f32(sum_j ((0.5 + 0.9189385332046727) + f64(log_std[j]))) from 0.0 in f64, j from 0."""
    e = F64(0.0)
    for j in range(2):
        e = e + ((F64(0.5) + F64(HALF_LOG_2PI)) + F64(log_std[j]))
    return F32(e)


def lsd_h6(d_log_prob, d_entropy, actions, mean, std):
    """H6 in L1's order: per row and j the term f64(d_log_prob) (z z - 1) + f64(d_entropy), z = (f64(a) -
    f64(mean)) / f64(std), one rounding per operation; lc.block_sum; rounded once."""
    z = (actions.astype(F64) - mean.astype(F64)) / np.asarray(std, F32).astype(F64)
    zz = z * z
    zm = zz - 1.0
    p = d_log_prob.astype(F64)[:, None] * zm
    t = p + d_entropy.astype(F64)[:, None]
    return np.array([lc.block_sum(t[:, j]) for j in range(2)], F64).astype(F32)


def restate(w, activation, x, mistake=None):
    """Forward and backward in f64 from the formulas -> a dict of FWD_OUT + BWD_OUT + the 13 weight
    gradients under "g_" + name.  mistake: one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    W = {k: np.asarray(v, F64) for k, v in w.items()}
    relu = activation == "relu"
    act = (lambda t: np.where(t > 0, t, 0.0)) if relu else np.tanh

    def dact(d, a):
        if relu:
            return np.where((a >= 0) if mistake == "relu_ge" else (a > 0), d, 0.0)
        return d * ((1.0 - a) if mistake == "one_minus_a" else (1.0 - a * a))

    out = {}
    h = dict(pi=x["h_pi"].astype(F64), vf=x["h_vf"].astype(F64))
    if mistake == "critic_fed_h_pi":
        h["vf"] = h["pi"]
    nets = dict(pi=("w1", "b1", "w2", "b2", "w3", "b3"), vf=("v1", "vb1", "v2", "vb2", "v3", "vb3"))
    for net, (w1, b1, w2, b2, w3, b3) in nets.items():
        a1 = act(h[net] @ W[w1].T + W[b1])
        a2 = act(a1 @ W[w2].T + W[b2])
        out["a1_" + net], out["a2_" + net] = a1, a2
        out["head_" + net] = a2 @ W[w3].T + W[b3]
    mean, ls = out.pop("head_pi"), W["log_std"]
    std = np.exp(ls)
    out["mean"], out["values"] = mean, out.pop("head_vf")[:, 0]
    diff = x["actions"].astype(F64) - mean
    z = diff if mistake == "z_without_std" else diff / std
    out["log_prob"] = (-0.5 * z * z - ls - HALF_LOG_2PI).sum(-1)
    e = (HALF_LOG_2PI + ls).sum() if mistake == "entropy_plus_one_dropped" else (0.5 + HALF_LOG_2PI + ls).sum()
    out["entropy"] = np.full(len(mean), e)
    dv, dlp, dent = (x[k].astype(F64) for k in ("d_values", "d_log_prob", "d_entropy"))
    out["d_mean"] = dlp[:, None] * (z / std)
    zm = z * z if mistake == "lsd_missing_minus_one" else z * z - 1.0
    out["d_log_std"] = (dlp[:, None] * zm + dent[:, None]).sum(0)
    for net, (w1, b1, w2, b2, w3, b3), d_out in (("pi", nets["pi"], out["d_mean"]), ("vf", nets["vf"], dv[:, None])):
        a1, a2 = out["a1_" + net], out["a2_" + net]
        d_z2 = dact(d_out @ W[w3], a2)
        d_z1 = dact(d_z2 @ (W[w2].T if mistake == "w2_not_transposed" else W[w2]), a1)
        out["d_z2_" + net], out["d_z1_" + net] = d_z2, d_z1
        out["d_h_" + net] = d_z1 @ W[w1]
        out["g_" + w3], out["g_" + b3] = d_out.T @ a2, d_out.sum(0)
        out["g_" + w2], out["g_" + b2] = d_z2.T @ a1, d_z2.sum(0)
        out["g_" + w1], out["g_" + b1] = d_z1.T @ h[net], d_z1.sum(0)
    out["g_log_std"] = out["d_log_std"]
    return out


def torch_reference(ref, w, activation, x, dtype):
    """tests/_ppo_reference.heads in `dtype` under torch.autograd.grad with the rows' three gradients as
    grad_outputs -> the dict restate() returns.  The biases enter as per-row copies [R, n], whose gradients
    are the pre-activation gradients d_z1, d_z2 and d_mean; a bias's own gradient is their sum over the rows
    in `dtype`."""
    import torch
    R = len(x["actions"])
    t = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in x.items()}
    p = {key: torch.from_numpy(np.asarray(w[k])).to(dtype).requires_grad_() for k, key in zip(TENSORS, TENSOR_KEYS)}
    per_row = {"b1": "d_z1_pi", "b2": "d_z2_pi", "b3": "d_mean", "vb1": "d_z1_vf", "vb2": "d_z2_vf", "vb3": "d_values_row"}
    q = dict(p)
    for k, key in zip(TENSORS, TENSOR_KEYS):
        if k in per_row:
            q[key] = p[key].detach().expand(R, -1).clone().requires_grad_()
    h_pi, h_vf = t["h_pi"].requires_grad_(), t["h_vf"].requires_grad_()
    values, log_prob, entropy = ref.heads(q, h_pi, h_vf, t["actions"], activation)
    names = [k for k in TENSORS]
    leaves = [q[key] for key in TENSOR_KEYS] + [h_pi, h_vf]
    grads = torch.autograd.grad([values, log_prob, entropy], leaves, [t["d_values"], t["d_log_prob"], t["d_entropy"]])
    out = dict(values=values, log_prob=log_prob, entropy=entropy, d_h_pi=grads[-2], d_h_vf=grads[-1])
    for k, g in zip(names, grads):
        if k in per_row:
            out[per_row[k]] = g
            out["g_" + k] = g.sum(0)
        else:
            out["g_" + k] = g
    out["d_log_std"] = out["g_log_std"]
    out.pop("d_values_row")
    return {k: v.detach().to(torch.float64).numpy() for k, v in out.items()}


BACKWARD = ("d_h_pi", "d_h_vf", "d_z1_pi", "d_z2_pi", "d_z1_vf", "d_z2_vf", "d_mean", "d_log_std") + \
    tuple("g_" + k for k in TENSORS)
FORWARD = ("values", "log_prob")


def d_refs(ref, w, activation, x):
    """-> (the f64 reference, {quantity: d_ref}): d_ref = max |f32 torch run - f64 torch run| of the same
    restatement, per quantity, never pooled."""
    import torch
    r64 = torch_reference(ref, w, activation, x, torch.float64)
    r32 = torch_reference(ref, w, activation, x, torch.float32)
    return r64, {k: float(np.abs(r32[k] - r64[k]).max()) for k in r64}


def errors(got, want, keys):
    """{quantity: max |got - want|} over `keys`."""
    return {k: float(np.abs(np.asarray(got[k], F64) - want[k]).max()) for k in keys}


def agrees(got, want, d_ref):
    """The tests' agreement between the host build's outputs (with the weight gradients under "g_" names)
    and a restatement: every BACKWARD quantity within 4 x d_ref, the entropy bit for bit."""
    err = errors(got, want, BACKWARD)
    ok = all(err[k] <= 4 * d_ref[k] for k in err)
    return ok and np.array_equal(np.asarray(got["entropy"], F32).view(np.uint32),
                                 np.asarray(want["entropy"], F64).astype(F32).view(np.uint32))
