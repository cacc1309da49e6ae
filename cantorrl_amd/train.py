"""The RecurrentPPO update on the device: the LSTM over a stored sequence with per-step resets as a
differentiable op (libhedgeactor's lstm_seq_fwd_kernel / lstm_seq_bwd_kernel, contract F1-F2 and
B1-B4 of include/hedge_actor.h), sb3_contrib's evaluate_actions and RecurrentPPO.train's loss on
top of it, in torch.

    policy = RecurrentPolicy.from_sb3_zip("final_model.zip")
    col = RolloutCollector(DeviceVecNormalize(venv), policy, gamma=0.98242, gae_lambda=0.91788, seed=7)
    module = RecurrentPPOModule.from_policy(policy)
    opt = torch.optim.Adam(module.parameters(), lr=1e-4, eps=1e-5)
    while True:
        buf = col.collect(256, buffer=buf)
        stats = ppo_update(module, opt, buf, envs_per_batch=1024)
        policy.load_state_dict(module.state_dict())

With opt = DeviceAdam(module.parameters(), lr=1e-4, eps=1e-5) the clip and the optimizer step are
libhedgeactor's ha_adam_step (two launches, contract O1-O5), and policy.load_device_state_dict(
module.state_dict()) re-packs the policy on the device: an iteration without a host round trip.

With ppo_update(loss="kernel") the loss, its statistics and its gradients with respect to values,
log_prob and entropy are libhedgeactor's ha_ppo_loss (ppo_loss_kernel, contract L1-L6).

With RecurrentPPOModule(heads="kernel") the part after the LSTMs (the two 64-64 MLPs, action_net, value_net,
the log-probability and the entropy) is libhedgeactor's ha_ppo_heads_forward / _backward (ppo_heads, contract
H1-H6): on a freshly collected buffer evaluate_actions then returns the buffer's own values and log_probs.

By default only the LSTM is a kernel: nn.LSTM has no per-step reset, so sb3_contrib's
_process_sequence runs one LSTM call per time step, forward and again in autograd's backward.  Here a workgroup walks all L
steps of its 32 envs inside one launch, actor and critic side by side.  The MLPs, the heads, the
Gaussian log-probability, the loss and the optimizer are batched over L B rows and stay with torch.
There is no torch fallback for the LSTM: a missing library is an error.  The LSTM's weight gradients are
sums of d_gates over the L B rows: blocked torch GEMMs by default (weight_grads), or with
weight_grads="kernel" libhedgeactor's lstm_wgrad_kernel (lstm_seq_weight_grads, contract W1-W4).
"""
import ctypes
import functools

import torch
from torch.autograd.function import once_differentiable

from .agent import (ACT_DIM, HIDDEN, MLP, OBS_DIM, POLICY_KEYS, STATE_NAMES, _check, _normalization, _read_sb3_zip,
                    load)
from ._bind import stream_of as _stream   # the current stream of a torch.device (raw handle)

_VP = ctypes.c_void_p
NET_INPUTS = ("h0", "c0", "w_ih", "w_hh", "b_ih", "b_hh")   # lstm_sequence's per-network arguments


class HaLstmSeqNet(ctypes.Structure):
    _fields_ = [(k, _VP) for k in ("w_ih", "w_hh", "b_ih", "b_hh", "h0", "c0", "h", "c", "gates")]


class HaLstmSeqBwd(ctypes.Structure):
    _fields_ = [(k, _VP) for k in ("w_hh", "c0", "c", "gates", "d_h", "d_gates")]


class HaLstmSeqWgrad(ctypes.Structure):
    _fields_ = [(k, _VP) for k in ("d_gates", "h", "h0", "d_w_ih", "d_w_hh", "d_b")]


WGRAD_BLOCK, WGRAD_CHUNK = 128, 64   # HA_WGRAD_BLOCK, HA_WGRAD_CHUNK of include/hedge_actor.h
WEIGHT_GRADS = ("torch", "kernel")


def _weight_grads_mode(mode):
    if mode not in WEIGHT_GRADS:
        raise ValueError(f"weight_grads must be one of {WEIGHT_GRADS}, not {mode!r}")
    return mode


def _f32(t, shape, name, device):
    """t as a contiguous, 16-byte aligned float32 tensor of `shape` on `device` (no copy when it is)."""
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or t.device != device:
        raise ValueError(f"{name} must be a float32 tensor of shape {tuple(shape)} on {device}, not "
                         f"{t.dtype} {tuple(t.shape)} on {t.device}")
    t = t.detach().contiguous()
    return t.clone() if t.data_ptr() % 16 else t


def _starts(es, L, B, device):
    if es.dtype == torch.bool:
        es = es.view(torch.uint8)
    if es.dtype != torch.uint8 or tuple(es.shape) != (L, B) or es.device != device:
        raise ValueError(f"episode_starts must be a uint8 / bool [{L}, {B}] tensor on {device}")
    es = es.contiguous()
    return es.clone() if es.data_ptr() % 16 else es


@functools.lru_cache(maxsize=16)
def _seq_shapes(L, B):
    """Every tensor of the three ha_lstm_seq_* structs by field name.  Cached (an update calls with one
    L, B again and again) and therefore shared: read only."""
    G = 4 * HIDDEN
    return dict(w_ih=(G, OBS_DIM), w_hh=(G, HIDDEN), b_ih=(G,), b_hh=(G,), h0=(B, HIDDEN), c0=(B, HIDDEN),
                h=(L, B, HIDDEN), c=(L, B, HIDDEN), gates=(L, B, 4, HIDDEN), d_h=(L, B, HIDDEN),
                d_gates=(L, B, 4, HIDDEN), d_w_ih=(G, OBS_DIM), d_w_hh=(G, HIDDEN), d_b=(G,))


def _seq_call(op, struct, x, like, episode_starts, nets, host, inputs, outputs,
              workspace="ha_lstm_seq_workspace_bytes"):
    """What lstm_seq_forward / _backward / _weight_grads share: ha_<op> on a HIP device or ha_host_<op>
    (host; default: by the tensors' device) over `nets`, one or two dicts with the tensors `inputs` of
    `struct`.  L, B are `like`'s leading dimensions; x is None for the call that takes none; `workspace`
    names the entry point that sizes the device call's workspace, from as many of (n, L, B) as it takes.
    -> per network the tuple of its new `outputs` tensors."""
    lib = load()
    dev = like.device
    host = dev.type == "cpu" if host is None else bool(host)
    if host != (dev.type == "cpu"):
        raise ValueError("host=True takes CPU tensors, host=False tensors on a HIP device")
    if x is not None and (x.dim() != 3 or x.shape[2] != OBS_DIM):
        raise ValueError(f"x must be [L, B, {OBS_DIM}]")
    L, B = int(like.shape[0]), int(like.shape[1])
    shapes = _seq_shapes(L, B)
    # (x, es, keep: the aligned copies live until the call is enqueued)
    if x is not None:
        x = _f32(x, (L, B, OBS_DIM), "x", dev)
    es = _starts(episode_starts, L, B, dev)
    lead = (es.data_ptr(),) if x is None else (x.data_ptr(), es.data_ptr())
    n = len(nets)
    arr = (struct * max(n, 1))()
    keep, out = [], []
    for k, net in enumerate(nets[:2]):
        s = arr[k]
        for name in inputs:
            t = _f32(net[name], shapes[name], name, dev)
            keep.append(t)
            setattr(s, name, t.data_ptr())
        new = tuple([torch.empty(shapes[name], dtype=torch.float32, device=dev) for name in outputs])
        for name, t in zip(outputs, new):
            setattr(s, name, t.data_ptr())
        out.append(new)
    if host:
        st = getattr(lib, "ha_host_" + op)(n, L, B, *lead, arr)
    else:
        with torch.cuda.device(dev):
            size = getattr(lib, workspace)   # sized by n alone, or by n, L, B
            ws = torch.empty(size(n) if len(size.argtypes) == 1 else size(n, L, B), dtype=torch.uint8, device=dev)
            st = getattr(lib, "ha_" + op)(n, L, B, *lead, arr, ws.data_ptr(), _stream(dev))
    _check(lib, st, "ha_" + op)
    return out


def lstm_seq_forward(x, episode_starts, nets, host=None):
    """ha_lstm_seq_forward (ha_host_lstm_seq_forward with host=True; default: by x's device).
    x [L,B,13] f32, episode_starts [L,B] u8 / bool, nets: one or two dicts of NET_INPUTS tensors ->
    a list of (h [L,B,128], c [L,B,128], gates [L,B,4,128]) per network.  No autograd."""
    return _seq_call("lstm_seq_forward", HaLstmSeqNet, x, x, episode_starts, nets, host, NET_INPUTS,
                     ("h", "c", "gates"))


def lstm_seq_backward(episode_starts, nets, host=None):
    """ha_lstm_seq_backward: nets = one or two dicts of w_hh [512,128], c0 [B,128], c [L,B,128], gates
    [L,B,4,128], d_h [L,B,128] -> a list of d_gates [L,B,4,128] per network.  No autograd."""
    out = _seq_call("lstm_seq_backward", HaLstmSeqBwd, None, nets[0]["d_h"], episode_starts, nets, host,
                    ("w_hh", "c0", "c", "gates", "d_h"), ("d_gates",))
    return [dg for dg, in out]


def lstm_seq_weight_grads(x, episode_starts, nets, host=None):
    """ha_lstm_seq_weight_grads (contract W1-W4): x [L,B,13], episode_starts [L,B], nets = one or two
    dicts of d_gates [L,B,4,128], h [L,B,128] (the forward's), h0 [B,128] -> a list of (d_w_ih [512,13],
    d_w_hh [512,128], d_b [512]) f32 per network; d_b is db_ih and db_hh.  No autograd."""
    return _seq_call("lstm_seq_weight_grads", HaLstmSeqWgrad, x, x, episode_starts, nets, host,
                     ("d_gates", "h", "h0"), ("d_w_ih", "d_w_hh", "d_b"), "ha_lstm_seq_weight_grads_workspace_bytes")


def weight_grads(d_gates, x, h, h0, episode_starts, rows=1 << 18, block=128):
    """The LSTM's weight gradients from d_gates [L,B,4,128], as f64 tensors: dW_ih = d_gates^T x,
    dW_hh = d_gates^T h_prev, db_ih = db_hh = sum d_gates, with h_prev = h shifted by one step, h0 in
    front, zeroed where episode_starts.  The sums run over L B rows: one batched f32 GEMM against
    [x | h_prev] sums blocks of `block` rows, and the blocks' results are added in f64 (about `rows`
    rows a pass).  One f32 GEMM over all rows misses the tests' 4 x d_ref bound by its own rounding,
    f64 GEMMs of these shapes are 30 x slower."""
    L, B = d_gates.shape[:2]
    f64, G, K = torch.float64, 4 * HIDDEN, OBS_DIM + HIDDEN
    steps = max(1, rows // B)
    w = torch.zeros((G, K), dtype=f64, device=d_gates.device)
    b = torch.zeros(G, dtype=f64, device=d_gates.device)
    for t0 in range(0, L, steps):
        t1 = min(t0 + steps, L)
        n = (t1 - t0) * B
        dg = d_gates[t0:t1].reshape(n, G)
        first = (h0 if t0 == 0 else h[t0 - 1]).unsqueeze(0)
        keep = (episode_starts[t0:t1] == 0).to(h.dtype).unsqueeze(-1)
        xh = torch.cat([x[t0:t1], torch.cat([first, h[t0:t1 - 1]], 0) * keep], -1).reshape(n, K)
        nb = n // block
        if nb:
            d3 = dg[:nb * block].view(nb, block, G)
            w += torch.bmm(d3.transpose(1, 2), xh[:nb * block].view(nb, block, K)).sum(0, dtype=f64)
            b += d3.sum(1).sum(0, dtype=f64)
        if n > nb * block:
            w += (dg[nb * block:].t() @ xh[nb * block:]).to(f64)
            b += dg[nb * block:].sum(0).to(f64)
    return w[:, :OBS_DIM], w[:, OBS_DIM:], b, b.clone()


class _LstmSeq(torch.autograd.Function):
    """h of one or two networks over the same x and episode_starts; per network the six NET_INPUTS.
    weight_grads ("torch" / "kernel", lstm_sequence's keyword) is how backward forms the weight gradients."""

    @staticmethod
    def forward(ctx, host, weight_grads, x, episode_starts, *tensors):
        n = len(tensors) // len(NET_INPUTS)
        nets = [dict(zip(NET_INPUTS, tensors[6 * k:6 * k + 6])) for k in range(n)]
        out = lstm_seq_forward(x, episode_starts, nets, host=host)
        saved = [x, episode_starts]
        for net, (h, c, gates) in zip(nets, out):
            saved += [net["h0"], net["c0"], net["w_hh"], h, c, gates]
        ctx.save_for_backward(*saved)
        ctx.host, ctx.n, ctx.weight_grads = host, n, weight_grads
        return tuple(h for h, _, _ in out)

    @staticmethod
    @once_differentiable
    def backward(ctx, *d_h):
        x, es = ctx.saved_tensors[:2]
        per = [ctx.saved_tensors[2 + 6 * k:8 + 6 * k] for k in range(ctx.n)]
        nets = []
        for (h0, c0, w_hh, h, c, gates), d in zip(per, d_h):
            d = torch.zeros_like(h) if d is None else d
            nets.append(dict(w_hh=w_hh, c0=c0, c=c, gates=gates, d_h=d))
        d_gates = lstm_seq_backward(es, nets, host=ctx.host)
        grads = [None, None, None, None]
        if ctx.weight_grads == "kernel":   # both networks in one call
            wg = lstm_seq_weight_grads(x, es, [dict(d_gates=dg, h=h, h0=h0)
                                               for (h0, c0, w_hh, h, c, gates), dg in zip(per, d_gates)], host=ctx.host)
            for d_w_ih, d_w_hh, d_b in wg:
                grads += [None, None, d_w_ih, d_w_hh, d_b, d_b.clone()]
            return tuple(grads)
        for (h0, c0, w_hh, h, c, gates), dg in zip(per, d_gates):
            grads += [None, None, *(g.to(torch.float32) for g in weight_grads(dg, x, h, h0, es))]
        return tuple(grads)


def lstm_sequence(x, episode_starts, h0, c0, w_ih, w_hh, b_ih, b_hh, host=None, weight_grads="torch"):
    """The LSTM (13 -> 128, one layer, torch's gate order) over x [L,B,13] from (h0, c0) [B,128], the
    state zeroed before every step where episode_starts [L,B] is set -> h [L,B,128], differentiable
    in the four weight tensors.  x, h0 and c0 receive no gradient (SB3 stores them as constants).
    One forward and one backward launch; host=True (default for CPU tensors) runs the host build.
    weight_grads: "torch" forms the weight gradients from d_gates with train.weight_grads (blocked
    f32 GEMMs added in f64), "kernel" with ha_lstm_seq_weight_grads (contract W1-W4: the same bits on
    the device and on the host build)."""
    host = x.device.type == "cpu" if host is None else bool(host)
    return _LstmSeq.apply(host, _weight_grads_mode(weight_grads), x, episode_starts, h0, c0, w_ih, w_hh, b_ih, b_hh)[0]


def lstm_sequence_pair(x, episode_starts, actor, critic, host=None, weight_grads="torch"):
    """lstm_sequence for actor and critic in one launch each way: `actor`, `critic` are the NET_INPUTS
    tuples (h0, c0, w_ih, w_hh, b_ih, b_hh) -> (h_pi, h_vf)."""
    host = x.device.type == "cpu" if host is None else bool(host)
    return _LstmSeq.apply(host, _weight_grads_mode(weight_grads), x, episode_starts, *actor, *critic)


# --------------------------------------------------------------------------- the heads as kernels
HEADS = ("torch", "kernel")
HEADS_TENSORS = ("w1", "b1", "w2", "b2", "w3", "b3", "log_std", "v1", "vb1", "v2", "vb2", "v3", "vb3")
_HEADS_SHAPES = dict(w1=(MLP, HIDDEN), b1=(MLP,), w2=(MLP, MLP), b2=(MLP,), w3=(ACT_DIM, MLP), b3=(ACT_DIM,),
                     log_std=(ACT_DIM,), v1=(MLP, HIDDEN), vb1=(MLP,), v2=(MLP, MLP), vb2=(MLP,), v3=(1, MLP), vb3=(1,))
HEADS_FWD_IN = ("h_pi", "h_vf", "actions")
HEADS_FWD_OUT = ("values", "log_prob", "entropy", "mean", "a1_pi", "a2_pi", "a1_vf", "a2_vf")
HEADS_BWD_IN = ("d_values", "d_log_prob", "d_entropy", "actions", "mean", "a1_pi", "a2_pi", "a1_vf", "a2_vf")
HEADS_BWD_OUT = ("d_h_pi", "d_h_vf", "d_z1_pi", "d_z2_pi", "d_z1_vf", "d_z2_vf", "d_mean", "d_log_std")


class HaPpoHeadsWeights(ctypes.Structure):
    _fields_ = [(k, _VP) for k in HEADS_TENSORS] + [("activation", ctypes.c_int32)]


class HaPpoHeadsFwd(ctypes.Structure):
    _fields_ = [(k, _VP) for k in HEADS_FWD_IN + HEADS_FWD_OUT]


class HaPpoHeadsBwd(ctypes.Structure):
    _fields_ = [(k, _VP) for k in HEADS_BWD_IN + HEADS_BWD_OUT]


def _heads_mode(mode):
    if mode not in HEADS:
        raise ValueError(f"heads must be one of {HEADS}, not {mode!r}")
    return mode


def _heads_row_shapes(R):
    one, two, mid, wide = (R,), (R, ACT_DIM), (R, MLP), (R, HIDDEN)
    return dict(h_pi=wide, h_vf=wide, actions=two, values=one, log_prob=one, entropy=one, mean=two, a1_pi=mid,
                a2_pi=mid, a1_vf=mid, a2_vf=mid, d_values=one, d_log_prob=one, d_entropy=one, d_h_pi=wide, d_h_vf=wide,
                d_z1_pi=mid, d_z2_pi=mid, d_z1_vf=mid, d_z2_vf=mid, d_mean=two, d_log_std=(ACT_DIM,))


def _heads_call(op, struct, rows, inputs, outputs, weights, activation, host):
    """What ppo_heads_forward / _backward share: ha_<op> on a HIP device or ha_host_<op> over `rows`, a dict
    of the `inputs` tensors with R rows each, and `weights`, the 13 HEADS_TENSORS -> a dict of the new
    `outputs` tensors."""
    lib = load()
    if activation not in ("tanh", "relu"):
        raise ValueError(f"activation must be 'tanh' or 'relu', not {activation!r}")
    first = rows[inputs[0]]
    dev, R = first.device, int(first.shape[0]) if first.dim() else 0
    host = dev.type == "cpu" if host is None else bool(host)
    if host != (dev.type == "cpu"):
        raise ValueError("host=True takes CPU tensors, host=False tensors on a HIP device")
    if len(weights) != len(HEADS_TENSORS):
        raise ValueError(f"weights: the {len(HEADS_TENSORS)} tensors {HEADS_TENSORS}")
    shapes = _heads_row_shapes(R)
    w, io, keep = HaPpoHeadsWeights(), struct(), []
    for name, t in zip(HEADS_TENSORS, weights):
        t = _f32(t, _HEADS_SHAPES[name], name, dev)
        keep.append(t)
        setattr(w, name, t.data_ptr())
    w.activation = 1 if activation == "relu" else 0
    for name in inputs:
        t = _f32(rows[name], shapes[name], name, dev)
        keep.append(t)
        setattr(io, name, t.data_ptr())
    out = {name: torch.empty(shapes[name], dtype=torch.float32, device=dev) for name in outputs}
    for name, t in out.items():
        setattr(io, name, t.data_ptr())
    if host:
        st = getattr(lib, "ha_host_" + op)(R, ctypes.byref(w), ctypes.byref(io))
    else:
        with torch.cuda.device(dev):
            ws = torch.empty(lib.ha_ppo_heads_workspace_bytes(R) or 16, dtype=torch.uint8, device=dev)
            st = getattr(lib, "ha_" + op)(R, ctypes.byref(w), ctypes.byref(io), ws.data_ptr(), _stream(dev))
    _check(lib, st, "ha_" + op)
    return out


def ppo_heads_forward(h_pi, h_vf, actions, weights, activation="tanh", host=None):
    """ha_ppo_heads_forward (contract H1-H3; CPU tensors run ha_host_ppo_heads_forward, the same bits):
    h_pi, h_vf [R,128], actions [R,2], weights = the 13 HEADS_TENSORS in torch layout -> a dict of values,
    log_prob, entropy [R], mean [R,2] and a1_pi, a2_pi, a1_vf, a2_vf [R,64] (saved for the backward).
    No autograd.  A refusal of the library is a ValueError with its message."""
    return _heads_call("ppo_heads_forward", HaPpoHeadsFwd, dict(h_pi=h_pi, h_vf=h_vf, actions=actions), HEADS_FWD_IN,
                       HEADS_FWD_OUT, weights, activation, host)


def ppo_heads_backward(d_values, d_log_prob, d_entropy, actions, saved, weights, activation="tanh", host=None):
    """ha_ppo_heads_backward (contract H4-H6): the three gradients [R], actions [R,2] and `saved`, the
    forward's dict (mean, a1_pi, a2_pi, a1_vf, a2_vf) -> a dict of d_h_pi, d_h_vf [R,128], d_z1_pi, d_z2_pi,
    d_z1_vf, d_z2_vf [R,64], d_mean [R,2], d_log_std [2].  No autograd."""
    rows = dict(saved, d_values=d_values, d_log_prob=d_log_prob, d_entropy=d_entropy, actions=actions)
    return _heads_call("ppo_heads_backward", HaPpoHeadsBwd, rows, HEADS_BWD_IN, HEADS_BWD_OUT, weights, activation, host)


def _blocked_tn(d, x, block=128):
    """d^T x and d's column sums over the rows of d [R,m], x [R,k] as f64 tensors: one batched f32 GEMM sums
    blocks of `block` rows, the blocks' results are added in f64 (as weight_grads)."""
    R, f64 = d.shape[0], torch.float64
    nb = R // block
    w = torch.zeros((d.shape[1], x.shape[1]), dtype=f64, device=d.device)
    b = torch.zeros(d.shape[1], dtype=f64, device=d.device)
    if nb:
        d3 = d[:nb * block].view(nb, block, -1)
        w += torch.bmm(d3.transpose(1, 2), x[:nb * block].view(nb, block, -1)).sum(0, dtype=f64)
        b += d3.sum(1).sum(0, dtype=f64)
    if R > nb * block:
        w += (d[nb * block:].t() @ x[nb * block:]).to(f64)
        b += d[nb * block:].sum(0).to(f64)
    return w, b


def heads_weight_grads(d_z, inp):
    """The 13 gradients of HEADS_TENSORS, f32, from the per-row tensors: d_z = ppo_heads_backward's dict plus
    d_values [R]; inp = dict(h_pi, h_vf, a1_pi, a2_pi, a1_vf, a2_vf).  dW = d^T input and db = sum d per layer
    through _blocked_tn (blocks of 128 rows in one batched f32 GEMM, the blocks added in f64); log_std's is
    contract H6's d_log_std."""
    f32 = torch.float32
    g = {}
    for net, (w1, b1, w2, b2, w3, b3), d_out in (("pi", HEADS_TENSORS[:6], d_z["d_mean"]),
                                                 ("vf", HEADS_TENSORS[7:], d_z["d_values"].reshape(-1, 1))):
        for wn, bn, d, x in ((w1, b1, d_z["d_z1_" + net], inp["h_" + net]), (w2, b2, d_z["d_z2_" + net], inp["a1_" + net]),
                             (w3, b3, d_out, inp["a2_" + net])):
            w, b = _blocked_tn(d, x)
            g[wn], g[bn] = w.to(f32), b.to(f32)
    g["log_std"] = d_z["d_log_std"]
    return tuple(g[k] for k in HEADS_TENSORS)


class _PpoHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, host, activation, h_pi, h_vf, actions, *weights):
        lead = h_pi.shape[:-1]
        flat = (h_pi.reshape(-1, HIDDEN), h_vf.reshape(-1, HIDDEN), actions.reshape(-1, ACT_DIM))
        out = ppo_heads_forward(*flat, weights, activation, host=host)
        ctx.save_for_backward(*flat, *weights, *(out[k] for k in HEADS_BWD_IN[4:]))
        ctx.host, ctx.activation, ctx.lead = host, activation, lead
        return tuple(out[k].view(lead) for k in ("values", "log_prob", "entropy"))

    @staticmethod
    @once_differentiable
    def backward(ctx, d_values, d_log_prob, d_entropy):
        h_pi, h_vf, actions = ctx.saved_tensors[:3]
        weights = ctx.saved_tensors[3:3 + len(HEADS_TENSORS)]
        saved = dict(zip(HEADS_BWD_IN[4:], ctx.saved_tensors[3 + len(HEADS_TENSORS):]))
        R = h_pi.shape[0]
        d = [torch.zeros(R, dtype=torch.float32, device=h_pi.device) if g is None else g.reshape(R)
             for g in (d_values, d_log_prob, d_entropy)]
        out = ppo_heads_backward(*d, actions, saved, weights, ctx.activation, host=ctx.host)
        grads = heads_weight_grads(dict(out, d_values=d[0]), dict(saved, h_pi=h_pi, h_vf=h_vf))
        return (None, None, out["d_h_pi"].view(*ctx.lead, HIDDEN), out["d_h_vf"].view(*ctx.lead, HIDDEN), None, *grads)


def ppo_heads(h_pi, h_vf, actions, w1, b1, w2, b2, w3, b3, log_std, v1, vb1, v2, vb2, v3, vb3, activation="tanh",
              host=None):
    """The part of evaluate_actions after the LSTMs as libhedgeactor's kernels (contract H1-H6 of
    include/hedge_actor.h): h_pi, h_vf [..., 128], actions [..., 2] and the 13 HEADS_TENSORS -> (values,
    log_prob, entropy) [...], differentiable in h_pi, h_vf and the 13 tensors; actions get no gradient.
    Forward: heads_pack_kernel + heads_fwd_kernel; backward: heads_pack_kernel + heads_bwd_kernel +
    heads_lsd_kernel, then the weight gradients from the per-row gradients with heads_weight_grads (torch).
    host=True (default for CPU tensors) runs the host build: the same bits."""
    host = h_pi.device.type == "cpu" if host is None else bool(host)
    return _PpoHeads.apply(host, activation, h_pi, h_vf, actions, w1, b1, w2, b2, w3, b3, log_std, v1, vb1, v2, vb2, v3,
                           vb3)


# --------------------------------------------------------------------------- the policy as a torch module
class _Lstm(torch.nn.Module):
    """The four tensors of a one-layer nn.LSTM under nn.LSTM's names (a container: the op is lstm_sequence)."""

    def __init__(self):
        super().__init__()
        P = torch.nn.Parameter
        self.weight_ih_l0 = P(torch.zeros(4 * HIDDEN, OBS_DIM))
        self.weight_hh_l0 = P(torch.zeros(4 * HIDDEN, HIDDEN))
        self.bias_ih_l0 = P(torch.zeros(4 * HIDDEN))
        self.bias_hh_l0 = P(torch.zeros(4 * HIDDEN))

    def tensors(self):
        return self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0, self.bias_hh_l0


class _MlpExtractor(torch.nn.Module):
    def __init__(self, act):
        super().__init__()
        L = torch.nn.Linear
        self.policy_net = torch.nn.Sequential(L(HIDDEN, MLP), act(), L(MLP, MLP), act())
        self.value_net = torch.nn.Sequential(L(HIDDEN, MLP), act(), L(MLP, MLP), act())


class RecurrentPPOModule(torch.nn.Module):
    """sb3_contrib's RecurrentActorCriticPolicy (MlpLstmPolicy: lstm_actor and lstm_critic 13 -> 128,
    net_arch 64-64, a state-independent log_std) with its 21 tensors under the checkpoint's own names:
    state_dict() feeds RecurrentPolicy.load_state_dict as it is.  activation: "tanh" (SB3's default)
    or "relu".  obs_mean / obs_var: the statistics a RecurrentPolicy applies to raw obs (contract step
    2); leave them out when the buffer holds normalised obs (a DeviceVecNormalize env).  weight_grads:
    lstm_sequence's keyword, passed on by evaluate_actions.  heads: "torch" runs the part after the LSTMs
    (self.heads) in torch, "kernel" as ppo_heads (ha_ppo_heads_forward / _backward, contract H1-H6)."""

    def __init__(self, activation="tanh", obs_mean=None, obs_var=None, clip_obs=10.0, epsilon=1e-8,
                 weight_grads="torch", heads="torch"):
        super().__init__()
        self.weight_grads = _weight_grads_mode(weight_grads)
        self.heads_mode = _heads_mode(heads)
        acts = {"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU}
        if activation not in acts:
            raise ValueError(f"activation must be one of {sorted(acts)}, not {activation!r}")
        if (obs_mean is None) != (obs_var is None):
            raise ValueError("obs_mean and obs_var come together")
        self.activation = activation
        self.lstm_actor, self.lstm_critic = _Lstm(), _Lstm()
        self.mlp_extractor = _MlpExtractor(acts[activation])
        self.action_net = torch.nn.Linear(MLP, ACT_DIM)
        self.value_net = torch.nn.Linear(MLP, 1)
        self.log_std = torch.nn.Parameter(torch.zeros(ACT_DIM))
        self.clip_obs, self.epsilon = clip_obs, float(epsilon)
        if obs_mean is not None:
            for name, v in (("obs_mean", obs_mean), ("obs_var", obs_var)):
                t = torch.as_tensor(v, dtype=torch.float64).reshape(-1).clone()
                if t.numel() != OBS_DIM:
                    raise ValueError(f"{name} has {t.numel()} entries, the obs has {OBS_DIM}")
                self.register_buffer(name, t, persistent=False)
        else:
            self.obs_mean = self.obs_var = None

    # ------------------------------------------------------------------ loaders
    @classmethod
    def from_state_dict(cls, sd, normalization=None, device=None, **kw):
        mean, var, over = _normalization(normalization)
        m = cls(obs_mean=mean, obs_var=var, **dict(over, **kw))
        m.load_state_dict({k: torch.as_tensor(sd[k]).to(torch.float32) for k, _, _ in POLICY_KEYS})
        return m if device is None else m.to(device)

    @classmethod
    def from_sb3_zip(cls, path, normalization=None, **kw):
        """An SB3 `model.save()` zip: its policy.pth is a plain torch state dict."""
        return cls.from_state_dict(_read_sb3_zip(path), normalization=normalization, **kw)

    @classmethod
    def from_policy(cls, policy, device=None, weight_grads="torch", heads="torch"):
        """The tensors, activation and statistics of an agent.RecurrentPolicy, on its device."""
        _, a = policy._host_weights()   # after a load_device_state_dict: the tensors it read
        m = cls(activation=policy.activation, obs_mean=a.get("obs_mean"), obs_var=a.get("obs_var"),
                clip_obs=policy.clip_obs, epsilon=policy.epsilon, weight_grads=weight_grads, heads=heads)
        m.load_state_dict({k: torch.from_numpy(a[f].copy()) for k, f, _ in POLICY_KEYS})
        return m.to(policy.device_name if device is None else device)

    # ------------------------------------------------------------------ evaluate_actions
    def normalize_obs(self, obs):
        """Contract step 2 in torch f64: f32(clip((f64(obs) - mean) / sqrt(var + epsilon), +-clip))."""
        if self.obs_mean is None:
            return obs
        q = (obs.to(torch.float64) - self.obs_mean) / torch.sqrt(self.obs_var + self.epsilon)
        if self.clip_obs is not None:
            q = torch.clamp(q, -float(self.clip_obs), float(self.clip_obs))
        return q.to(torch.float32)

    def heads(self, h_pi, h_vf, actions):
        """The part after the LSTMs: values, log_prob, entropy of `actions` (trailing shapes [] each)."""
        mean = self.action_net(self.mlp_extractor.policy_net(h_pi))
        values = self.value_net(self.mlp_extractor.value_net(h_vf)).squeeze(-1)
        dist = torch.distributions.Normal(mean, torch.ones_like(mean) * self.log_std.exp())
        return values, dist.log_prob(actions).sum(-1), dist.entropy().sum(-1)

    def heads_tensors(self):
        """The 13 tensors after the LSTMs in HEADS_TENSORS' order."""
        pi, vf = self.mlp_extractor.policy_net, self.mlp_extractor.value_net
        return (pi[0].weight, pi[0].bias, pi[2].weight, pi[2].bias, self.action_net.weight, self.action_net.bias,
                self.log_std, vf[0].weight, vf[0].bias, vf[2].weight, vf[2].bias, self.value_net.weight,
                self.value_net.bias)

    def evaluate_actions(self, obs, actions, episode_starts, states0, host=None):
        """sb3_contrib's evaluate_actions over whole sequences: obs [L,B,13], actions [L,B,2],
        episode_starts [L,B], states0 = (h_pi, c_pi, h_vf, c_vf) [B,128] before step 0 ->
        (values, log_prob, entropy), each [L,B]."""
        x = self.normalize_obs(obs)
        h_pi, h_vf = lstm_sequence_pair(x, episode_starts, (states0[0], states0[1], *self.lstm_actor.tensors()),
                                        (states0[2], states0[3], *self.lstm_critic.tensors()), host=host,
                                        weight_grads=self.weight_grads)
        if self.heads_mode == "kernel":
            return ppo_heads(h_pi, h_vf, actions, *self.heads_tensors(), activation=self.activation, host=host)
        return self.heads(h_pi, h_vf, actions)


# --------------------------------------------------------------------------- the update
def ppo_loss(values, log_prob, entropy, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef,
             normalize_advantage=True, clip_range_vf=None, old_values=None):
    """sb3_contrib 2.6.0 RecurrentPPO.train's loss for one minibatch without padding (mask all ones)
    -> (loss, stats).  clip_range_vf (None: no value clip) clips the value's move away from old_values,
    the rollout's values of the same rows, as SB3 does."""
    adv = advantages
    if normalize_advantage:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(log_prob - old_log_prob)
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    if clip_range_vf is not None:
        if old_values is None:
            raise ValueError("clip_range_vf needs old_values")
        values = old_values + torch.clamp(values - old_values, -clip_range_vf, clip_range_vf)
    value_loss = ((returns - values) ** 2).mean()
    entropy_loss = -entropy.mean()
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    with torch.no_grad():
        log_ratio = log_prob - old_log_prob
        stats = dict(loss=loss.detach(), policy_gradient_loss=policy_loss.detach(), value_loss=value_loss.detach(),
                     entropy_loss=entropy_loss.detach(), approx_kl=((torch.exp(log_ratio) - 1) - log_ratio).mean(),
                     clip_fraction=(torch.abs(ratio - 1) > clip_range).float().mean())
    return loss, stats


class HaPpoLossHyper(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("clip_range", "clip_range_vf", "ent_coef", "vf_coef")] + \
               [("normalize_advantage", ctypes.c_int32)]


class HaPpoLossIo(ctypes.Structure):
    _fields_ = [(k, _VP) for k in ("values", "log_prob", "entropy", "old_log_prob", "advantages", "returns",
                                   "old_values", "d_values", "d_log_prob", "d_entropy", "stats")]


LOSS_BLOCK, LOSS_MAX_BLOCKS = 1024, 4096   # HA_LOSS_* of include/hedge_actor.h
LOSS_STATS = ("loss", "policy_gradient_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction",
              "adv_mean", "adv_std")       # the order of ha_ppo_loss_io.stats
LOSSES = ("torch", "kernel")


def ppo_loss_kernel(values, log_prob, entropy, old_log_prob, advantages, returns, clip_range, ent_coef, vf_coef,
                    normalize_advantage=True, clip_range_vf=None, old_values=None):
    """ppo_loss and its backward as libhedgeactor's ha_ppo_loss (contract L1-L6 of include/hedge_actor.h:
    four launches, two without normalisation; CPU tensors run ha_host_ppo_loss, the same bits) ->
    (stats, (d_values, d_log_prob, d_entropy)): ppo_loss's statistics plus adv_mean and adv_std as 0-d
    tensors, and the loss's gradients with respect to the first three arguments in their shape.  The
    inputs are float32 tensors of one shape on one device; they are detached.  Nothing synchronises with
    the host.  A refusal of the library is a ValueError with its message."""
    lib = load()
    shape, dev = values.shape, values.device
    names = ("values", "log_prob", "entropy", "old_log_prob", "advantages", "returns", "old_values")
    given = (values, log_prob, entropy, old_log_prob, advantages, returns, old_values)
    if clip_range_vf is None:
        given, cv = given[:6], 0.0
    else:
        cv = float(clip_range_vf)
        if not cv > 0.0:
            raise ValueError(f"clip_range_vf = {clip_range_vf} must be > 0, or None for no value clip")
        if old_values is None:
            raise ValueError("clip_range_vf needs old_values")
    io, keep = HaPpoLossIo(), []
    for name, t in zip(names, given):
        if t.dtype != torch.float32 or t.shape != shape or t.device != dev:
            raise ValueError(f"{name} must be a float32 tensor of shape {tuple(shape)} on {dev}, not "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")
        t = t.detach().contiguous()
        keep.append(t)
        setattr(io, name, t.data_ptr())
    grads = tuple(torch.empty(shape, dtype=torch.float32, device=dev) for _ in range(3))
    out = torch.empty(len(LOSS_STATS), dtype=torch.float32, device=dev)
    io.d_values, io.d_log_prob, io.d_entropy, io.stats = (*(g.data_ptr() for g in grads), out.data_ptr())
    hy = HaPpoLossHyper(float(clip_range), cv, float(ent_coef), float(vf_coef), int(bool(normalize_advantage)))
    n = values.numel()
    if dev.type == "cpu":
        st = lib.ha_host_ppo_loss(n, ctypes.byref(io), ctypes.byref(hy))
    else:
        with torch.cuda.device(dev):
            ws = torch.empty(lib.ha_ppo_loss_workspace_bytes(n) or 8, dtype=torch.uint8, device=dev)
            st = lib.ha_ppo_loss(n, ctypes.byref(io), ctypes.byref(hy), ws.data_ptr(), _stream(dev))
    _check(lib, st, "ha_ppo_loss")
    return dict(zip(LOSS_STATS, out.unbind(0))), grads


class HaAdamTensor(ctypes.Structure):
    _fields_ = [(k, _VP) for k in ("param", "grad", "exp_avg", "exp_avg_sq")] + [("numel", ctypes.c_int64)]


class HaAdamHyper(ctypes.Structure):
    _fields_ = [(k, ctypes.c_double) for k in ("lr", "beta1", "beta2", "eps", "max_grad_norm")] + \
               [("t", ctypes.c_int64), ("grad_norm_out", _VP)]


OPT_BLOCK, OPT_MAX_TENSORS, OPT_MAX_BLOCKS = 256, 64, 4096   # HA_OPT_* of include/hedge_actor.h


class DeviceAdam(torch.optim.Optimizer):
    """torch.optim.Adam (no weight decay, no amsgrad) with the gradient-norm clip in front, as
    libhedgeactor's ha_adam_step: two launches for all the parameters, arithmetic contract O1-O5 of
    include/hedge_actor.h, the same bits from the host build (CPU parameters run ha_host_adam_step).

        opt = DeviceAdam(module.parameters(), lr=1e-4, eps=1e-5)
        loss.backward()
        grad_norm = opt.clip_and_step(0.5)     # clip_grad_norm_(params, 0.5) + Adam.step()

    One parameter group of up to 64 contiguous float32 tensors on one device, 2^20 elements in blocks
    of 256.  param_groups[0]["lr"] is read at every step (schedulers work); state_dict() has
    torch.optim.Adam's layout (step, exp_avg, exp_avg_sq per parameter) and loads into one, and back.
    Nothing synchronises with the host."""

    _prep = None   # what does not change from step to step (_prepare); not part of the pickled state

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        if not 0.0 <= lr or not 0.0 <= eps or not all(0.0 <= b < 1.0 for b in betas):
            raise ValueError(f"DeviceAdam: lr {lr} and eps {eps} must be >= 0, betas {betas} in [0, 1)")
        # torch.optim.Adam's keys, so that either optimizer runs a state dict of the other
        defaults = dict(torch.optim.Adam([torch.zeros(1)]).defaults, lr=lr, betas=tuple(betas), eps=eps)
        super().__init__(params, defaults)
        load()              # a missing library is an error here, not at the first step

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._prep = None   # new state tensors

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        self._prep = None

    def _prepare(self):
        """The parameters checked, their state made, the ctypes array with everything but the gradients
        filled in, the workspace -> (params, array, step counters, device, workspace)."""
        if len(self.param_groups) != 1:
            raise ValueError("DeviceAdam runs one parameter group")
        params = self.param_groups[0]["params"]
        if not 1 <= len(params) <= OPT_MAX_TENSORS:
            raise ValueError(f"DeviceAdam takes 1 to {OPT_MAX_TENSORS} parameters, not {len(params)}")
        arr = (HaAdamTensor * len(params))()
        dev, steps = params[0].device, []
        for a, p in zip(arr, params):
            st = self.state[p]
            if not st:
                st["step"] = torch.zeros((), dtype=torch.float32)   # on the host, as torch.optim.Adam keeps it
                st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            for what, x in (("parameter", p), ("state exp_avg", st["exp_avg"]), ("state exp_avg_sq", st["exp_avg_sq"])):
                if x.dtype != torch.float32 or not x.is_contiguous() or x.device != dev or x.shape != p.shape:
                    raise ValueError(f"DeviceAdam: every {what} must be a contiguous float32 tensor on {dev}")
            if st["step"].device.type != "cpu":   # a fused torch.optim.Adam's: reading it each step would wait
                st["step"] = st["step"].detach().to("cpu", torch.float32)
            steps.append(st["step"])
            a.exp_avg, a.exp_avg_sq, a.numel = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), p.numel()
        if len({int(s) for s in steps}) != 1:
            raise ValueError(f"DeviceAdam: the parameters' step counts differ ({sorted({int(s) for s in steps})})")
        ws = None
        if dev.type != "cpu":
            size = load().ha_adam_workspace_bytes(len(params), arr)
            if not size:
                _check(load(), load().ha_adam_step(len(params), arr, None, None, None), "ha_adam_step")   # says why
            ws = torch.empty(size, dtype=torch.uint8, device=dev)
        self._prep = (params, arr, steps, dev, ws)
        return self._prep

    @torch.no_grad()
    def clip_and_step(self, max_grad_norm):
        """clip_grad_norm_(params, max_grad_norm) and Adam's step; max_grad_norm None, <= 0 or inf: no
        clip.  -> the gradients' norm before the clip, a scalar tensor on the parameters' device."""
        params, arr, steps, dev, ws = self._prep or self._prepare()
        group = self.param_groups[0]
        if group["weight_decay"] or group["amsgrad"] or group["maximize"]:
            raise ValueError("DeviceAdam has no weight_decay, amsgrad or maximize")
        f32 = torch.float32
        for a, p in zip(arr, params):   # the gradients are new tensors after every zero_grad(set_to_none=True)
            g = p.grad
            if g is None:
                raise ValueError("DeviceAdam: a parameter has no gradient (every tensor of the call is updated)")
            if g.dtype != f32 or g.device != dev or not g.is_contiguous():
                raise ValueError(f"DeviceAdam: every gradient must be a contiguous float32 tensor on {dev}")
            a.param, a.grad = p.data_ptr(), g.data_ptr()
        norm = torch.empty((), dtype=f32, device=dev)
        hy = HaAdamHyper(float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                         0.0 if max_grad_norm is None else float(max_grad_norm), int(steps[0]) + 1, norm.data_ptr())
        if dev.type == "cpu":
            st = load().ha_host_adam_step(len(params), arr, ctypes.byref(hy))
        else:
            with torch.cuda.device(dev):
                st = load().ha_adam_step(len(params), arr, ctypes.byref(hy), ws.data_ptr(), _stream(dev))
        _check(load(), st, "ha_adam_step")
        torch._foreach_add_(steps, 1)
        return norm

    def step(self, closure=None):
        """Adam's step without a clip."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self.clip_and_step(None)
        return loss


def minibatch(buffer, idx, k0, k1):
    """Envs `idx` (an int64 tensor) x steps [k0, k1) of a RolloutBuffer -> a dict of contiguous tensors
    and states0, the LSTM states before step k0."""
    sl = slice(k0, k1)
    mb = {name: getattr(buffer, name)[sl].index_select(1, idx)
          for name in ("observations", "actions", "episode_starts", "log_probs", "advantages", "returns")}
    if k0 == 0:
        mb["states0"] = tuple(getattr(buffer, s).index_select(0, idx) for s in STATE_NAMES)
    else:
        st = buffer.states[k0].index_select(0, idx)
        mb["states0"] = tuple(st[:, i].contiguous() for i in range(4))
    return mb


def ppo_update(module, optimizer, buffer, *, n_epochs=10, envs_per_batch=None, window=None, clip_range=0.3,
               ent_coef=1e-5, vf_coef=0.5, max_grad_norm=0.5, normalize_advantage=True, generator=None,
               loss="torch", clip_range_vf=None):
    """RecurrentPPO.train over a collect.RolloutBuffer: n_epochs passes, each over a fresh permutation
    of the envs (from `generator`, a torch.Generator on the buffer's device) cut into groups of
    envs_per_batch (default: all), each group x each time window one optimizer step.  window=None: the
    whole K steps from buffer.h_pi ...; window=W (dividing K): W steps from buffer.states[k0], which
    collect(states=True) stores.  Defaults: the reference's default_hpo_params (train_ppo_v2.py:601-605:
    clip_range 0.3, ent_coef 1e-5, vf_coef 0.5, max_grad_norm 0.5, n_epochs 10).  An optimizer with a
    clip_and_step method (DeviceAdam) clips and steps through it, any other through clip_grad_norm_ and
    step().  loss: "torch" is ppo_loss under autograd; "kernel" is ppo_loss_kernel (ha_ppo_loss, contract
    L1-L6) on the heads' detached outputs, its three gradients handed to autograd where the heads stand (on
    a module with heads="kernel" they enter ppo_heads' backward, ha_ppo_heads_backward, as they are).
    clip_range_vf (None: no value clip) is SB3's, against buffer.values.  target_kl is not built.
    Nothing synchronises
    with the host; returns the last minibatch's statistics and the mean loss as device scalars."""
    if loss not in LOSSES:
        raise ValueError(f"loss must be one of {LOSSES}, not {loss!r}")
    K, n = buffer.k_steps, buffer.n_envs
    W = K if window is None else int(window)
    if W < 1 or K % W:
        raise ValueError(f"window = {window} must divide the buffer's {K} steps")
    if W != K and buffer.states is None:
        raise ValueError("window < K starts from the states of step k0: collect the buffer with states=True")
    per = n if envs_per_batch is None else int(envs_per_batch)
    if per < 1:
        raise ValueError("envs_per_batch must be >= 1")
    dev = buffer.observations.device
    params = [p for p in module.parameters() if p.requires_grad]
    stats, total, count = {}, None, 0
    for _ in range(int(n_epochs)):
        perm = torch.randperm(n, device=dev, generator=generator)
        for lo in range(0, n, per):
            idx = perm[lo:lo + per]
            for k0 in range(0, K, W):
                mb = minibatch(buffer, idx, k0, k0 + W)
                values, log_prob, entropy = module.evaluate_actions(mb["observations"], mb["actions"],
                                                                    mb["episode_starts"], mb["states0"])
                old_values = None if clip_range_vf is None else buffer.values[k0:k0 + W].index_select(1, idx)
                args = (values, log_prob, entropy, mb["log_probs"], mb["advantages"], mb["returns"], clip_range,
                        ent_coef, vf_coef, normalize_advantage, clip_range_vf, old_values)
                optimizer.zero_grad(set_to_none=True)
                if loss == "kernel":
                    stats, grads = ppo_loss_kernel(*args)
                    torch.autograd.backward([values, log_prob, entropy], list(grads))
                else:
                    total_loss, stats = ppo_loss(*args)
                    total_loss.backward()
                if hasattr(optimizer, "clip_and_step"):   # DeviceAdam: the clip and the step in two launches
                    stats["grad_norm"] = optimizer.clip_and_step(max_grad_norm)
                else:
                    stats["grad_norm"] = torch.nn.utils.clip_grad_norm_(params, max_grad_norm)
                    optimizer.step()
                total = stats["loss"] if total is None else total + stats["loss"]
                count += 1
    if count:
        stats["mean_loss"] = total / count
    return stats
