"""Device time of the RecurrentPPO update's LSTM (cantorrl_amd.train): lstm_sequence_pair forward plus
backward (two launches each way: the packing kernel and the sequence kernel, then the weight-gradient
GEMMs) against -- same box, same process -- the all-torch composition of the same op: sb3_contrib's
_process_sequence loop of one cell per time step with the state zeroed at episode starts, under
autograd, f32.  And one ppo_update epoch over a buffer of the first shape.  HIP events around each
call, warm-up first, the median.

    python tools/train_time.py [--reps R] [--out FILE.jsonl] [--shapes L,B ...] [--weight-grads torch|kernel|both]
                               [--optimizer] [--loss] [--heads]

--weight-grads torch (the default) times lstm_sequence_pair as it is called by default, its weight
gradients from train.weight_grads.  kernel times forward plus backward with weight_grads="kernel", and
ha_lstm_seq_weight_grads alone on the backward's d_gates: per network and for the pair in one call,
beside its two floors (2 x 512 x 142 FLOP a row at the 155 TFLOP/s f32-MFMA rate; 2,048 + 512 + 52 + 1
bytes a row at the 6.29 TB/s copy ceiling).  both adds train.weight_grads alone on the same tensors,
the baseline, in the same process.

Default shapes: L = 256 with B = 4,096 and 16,384 (the largest power of two at which the all-torch
composition's saved activations, about 8 KB per step, env and network, still fit beside the kernel's
3 KB), and L = 32, B = 2 (the reference's BATCH_SIZE_AGENT = 32 steps of N_ENVS = 2).  One JSON line
per shape; with --out they are appended to the file as well (profiles/train_time_*.jsonl).
FLOP per env-step and network: 2 x 512 x 141 forward, 2 x 512 x 128 backward.

--optimizer times, instead, the seam between two rollouts on the module's 21 tensors: clip_grad_norm_ +
torch.optim.Adam.step() (default and fused=True) against train.DeviceAdam.clip_and_step (HIP events, and
wall time to completion), RecurrentPolicy.load_state_dict against load_device_state_dict (wall time with
the Python call included: until the call returns, and until the device is done), and one ppo_update
epoch per --shapes entry with each optimizer.

--loss times, instead, the PPO loss: train.ppo_loss forward plus autograd's backward to values, log_prob
and entropy against train.ppo_loss_kernel (ha_ppo_loss) on the same tensors at 64, 262,144 and 2^22 rows,
beside the bytes floor (40 B a row at the 6.29 TB/s copy ceiling), and one ppo_update epoch with
loss="torch" and loss="kernel" (DeviceAdam) at 32 x 2 (envs_per_batch 1) and 256 x 4,096 (envs_per_batch
1,024).  Both paths run in this process.

--heads times, instead, the part of evaluate_actions after the LSTMs, forward plus backward to h_pi, h_vf and
the 13 tensors: RecurrentPPOModule.heads under autograd against train.ppo_heads (ha_ppo_heads_forward /
_backward, then the weight gradients' torch GEMMs) on the same tensors at 64, 262,144 and 1,048,576 rows, the
six kernel launches alone beside their bytes floor (5,160 B a row at the 6.29 TB/s copy ceiling), and one
ppo_update epoch (DeviceAdam, loss="kernel", weight_grads="kernel") with heads="torch" and heads="kernel" at
32 x 2 (envs_per_batch 1) and 256 x 4,096 (envs_per_batch 1,024).  Both paths run in this process.
"""
import argparse
import copy
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from actor_time import median_us  # noqa: E402
from cantorrl_amd import train  # noqa: E402
from cantorrl_amd.agent import POLICY_KEYS  # noqa: E402
from cantorrl_amd.collect import RolloutBuffer  # noqa: E402

FLOP_FWD, FLOP_BWD = 2 * 512 * 141, 2 * 512 * 128
FLOP_WGRAD, BYTES_WGRAD = 2 * 512 * 142, 2048 + 512 + 52 + 1   # per row and network
PEAK_F32_MFMA, COPY_CEILING = 155e12, 6.29e12                 # FLOP/s, B/s (measured, MI355X)
DEV = "cuda:0"


def torch_lstm_loop(x, es, h0, c0, w_ih, w_hh, b_ih, b_hh):
    h, c = h0, c0
    hs = []
    for t in range(x.shape[0]):
        keep = (es[t] == 0).to(x.dtype).unsqueeze(-1)
        h, c = h * keep, c * keep
        i, f, g, o = (x[t] @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh).chunk(4, -1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h)
    return torch.stack(hs)


def module(rng):
    m = train.RecurrentPPOModule()
    m.load_state_dict({k: torch.from_numpy((rng.uniform(-1, 1, shape) / np.sqrt(shape[-1])).astype(np.float32))
                       for k, _, shape in POLICY_KEYS})
    return m.to(DEV)


def measure_weight_grads(r, x, es, nets, d_h, reps, mode):
    """The weight gradients alone, on the d_gates of the backward kernel."""
    L, B = es.shape
    with torch.no_grad():
        fwd = train.lstm_seq_forward(x, es, [dict(zip(train.NET_INPUTS, n)) for n in nets])
        bwd = [dict(w_hh=n[3], c0=n[1], c=o[1], gates=o[2], d_h=d) for n, o, d in zip(nets, fwd, d_h)]
        d_gates = train.lstm_seq_backward(es, bwd)
    wn = [dict(d_gates=dg, h=o[0], h0=n[0]) for dg, o, n in zip(d_gates, fwd, nets)]
    rows = L * B
    r["wgrad_kernel_net_us"] = [round(median_us(lambda k=k: train.lstm_seq_weight_grads(x, es, [wn[k]]), reps, 3), 1)
                                for k in range(2)]
    r["wgrad_kernel_pair_us"] = round(median_us(lambda: train.lstm_seq_weight_grads(x, es, wn), reps, 3), 1)
    r["wgrad_floor_flop_us"] = round(rows * FLOP_WGRAD / PEAK_F32_MFMA * 1e6, 1)
    r["wgrad_floor_bytes_us"] = round(rows * BYTES_WGRAD / COPY_CEILING * 1e6, 1)
    per_net = r["wgrad_kernel_pair_us"] / 2
    r["wgrad_kernel_frac_of_flop_floor"] = round(r["wgrad_floor_flop_us"] / per_net, 3)
    r["wgrad_kernel_frac_of_bytes_floor"] = round(r["wgrad_floor_bytes_us"] / per_net, 3)
    r["wgrad_kernel_tflops"] = round(rows * FLOP_WGRAD / per_net / 1e6, 2)
    if mode == "both":
        r["wgrad_torch_net_us"] = [round(median_us(lambda k=k: train.weight_grads(d_gates[k], x, fwd[k][0], nets[k][0], es),
                                                   reps, 3), 1) for k in range(2)]
        r["wgrad_speedup_per_net"] = round(sum(r["wgrad_torch_net_us"]) / r["wgrad_kernel_pair_us"], 2)


def measure(L, B, reps, mode="torch"):
    rng = np.random.default_rng(0)
    m = module(rng)
    g = torch.Generator(device=DEV).manual_seed(1)
    x = torch.rand((L, B, 13), device=DEV, generator=g) * 4 - 2
    es = (torch.rand((L, B), device=DEV, generator=g) < 0.004).to(torch.uint8)
    st = [torch.rand((B, 128), device=DEV, generator=g) - 0.5 for _ in range(4)]
    d_h = [torch.randn((L, B, 128), device=DEV, generator=g) for _ in range(2)]
    nets = ((st[0], st[1], *m.lstm_actor.tensors()), (st[2], st[3], *m.lstm_critic.tensors()))

    def kernel_fwd():
        with torch.no_grad():
            train.lstm_sequence_pair(x, es, *nets)

    def kernel_both():
        m.zero_grad(set_to_none=True)
        h = train.lstm_sequence_pair(x, es, *nets)
        torch.autograd.backward(h, d_h)

    def torch_fwd():
        with torch.no_grad():
            for n in nets:
                torch_lstm_loop(x, es, *n)

    def torch_both():
        m.zero_grad(set_to_none=True)
        h = [torch_lstm_loop(x, es, *n) for n in nets]
        torch.autograd.backward(h, d_h)

    def kernel_both_wgrad():
        m.zero_grad(set_to_none=True)
        h = train.lstm_sequence_pair(x, es, *nets, weight_grads="kernel")
        torch.autograd.backward(h, d_h)

    r = dict(L=L, B=B, reps=reps, device=torch.cuda.get_device_name(0))
    r["kernel_fwd_us"] = round(median_us(kernel_fwd, reps, 3), 1)
    r["kernel_fwd_bwd_us"] = round(median_us(kernel_both, reps, 3), 1)
    if mode != "torch":
        r["weight_grads"] = mode
        r["kernel_fwd_bwd_wgrad_kernel_us"] = round(median_us(kernel_both_wgrad, reps, 3), 1)
        measure_weight_grads(r, x, es, nets, d_h, reps, mode)
    if mode == "kernel":   # the all-torch composition is the default mode's comparison
        return r, m
    treps = reps if L * B <= 2 ** 20 else max(reps // 10, 3)   # the loop is 256 x ~40 launches a pass
    r["torch_fwd_us"] = round(median_us(torch_fwd, treps, 2), 1)
    r["torch_fwd_bwd_us"] = round(median_us(torch_both, treps, 2), 1)
    r["torch_reps"] = treps
    r["speedup_fwd_bwd"] = round(r["torch_fwd_bwd_us"] / r["kernel_fwd_bwd_us"], 2)
    r["kernel_fwd_tflops"] = round(2 * L * B * FLOP_FWD / r["kernel_fwd_us"] / 1e6, 2)
    r["kernel_us_per_step_fwd"] = round(r["kernel_fwd_us"] / L, 2)
    r["kernel_us_per_step_bwd"] = round((r["kernel_fwd_bwd_us"] - r["kernel_fwd_us"]) / L, 2)
    return r, m


def measure_update(m, K, n, per, reps):
    return measure_update_with(m, torch.optim.Adam(m.parameters(), lr=1e-5, eps=1e-5), K, n, per, reps)


def measure_update_with(m, opt, K, n, per, reps, **kw):
    buf = RolloutBuffer(K, n, DEV)
    g = torch.Generator(device=DEV).manual_seed(2)
    for name in ("observations", "actions", "rewards", "values", "advantages", "returns", "h_pi", "c_pi", "h_vf", "c_vf"):
        t = getattr(buf, name)
        t.copy_(torch.randn(t.shape, device=DEV, generator=g) * 0.5)
    buf.log_probs.fill_(-1.0)
    buf.episode_starts.copy_((torch.rand((K, n), device=DEV, generator=g) < 0.004).to(torch.uint8))
    us = median_us(lambda: train.ppo_update(m, opt, buf, n_epochs=1, envs_per_batch=per, **kw), reps, 1)
    return dict(ppo_update_epoch_us=round(us, 1), K=K, n_envs=n, envs_per_batch=per, minibatches=-(-n // per), update_reps=reps)


def wall_us(fn, reps, warmup=3):
    """Median wall time of fn() with the Python call included, the device idle before each call ->
    (until the call returns, until the device has finished what it enqueued), microseconds."""
    ret, done = [], []
    for k in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if k >= warmup:
            ret.append((t1 - t0) * 1e6)
            done.append((t2 - t0) * 1e6)
    return round(statistics.median(ret), 1), round(statistics.median(done), 1)


def measure_optimizer(shapes, reps):
    """--optimizer: (a) the clip and the optimizer step over the module's 21 tensors, torch's
    clip_grad_norm_ + torch.optim.Adam.step() (default and fused=True) against DeviceAdam.clip_and_step,
    HIP events; (b) RecurrentPolicy.load_state_dict against load_device_state_dict, wall time; and one
    ppo_update epoch per shape and optimizer.  Every baseline runs in this process, beside what it is
    compared with."""
    from cantorrl_amd.agent import RecurrentPolicy
    rng = np.random.default_rng(0)
    m = module(rng)
    r = dict(mode="optimizer", reps=reps, device=torch.cuda.get_device_name(0), tensors=len(list(m.parameters())),
             floats=sum(p.numel() for p in m.parameters()))
    g = torch.Generator(device=DEV).manual_seed(4)
    makers = (("torch_adam", lambda ps: torch.optim.Adam(ps, lr=1e-5, eps=1e-5)),
              ("torch_adam_fused", lambda ps: torch.optim.Adam(ps, lr=1e-5, eps=1e-5, fused=True)),
              ("device_adam", lambda ps: train.DeviceAdam(ps, lr=1e-5, eps=1e-5)))
    for name, make in makers:
        mm = copy.deepcopy(m)
        ps = list(mm.parameters())
        for p in ps:
            p.grad = torch.randn(p.shape, device=DEV, generator=g) * 0.1
        opt = make(ps)

        def torch_step():
            torch.nn.utils.clip_grad_norm_(ps, 0.5)
            opt.step()

        fn = (lambda: opt.clip_and_step(0.5)) if name == "device_adam" else torch_step
        r[f"clip_step_{name}_us"] = round(median_us(fn, reps, 3), 1)
        r[f"clip_step_{name}_wall_us"] = wall_us(fn, reps)[1]
    for base in ("torch_adam", "torch_adam_fused"):
        r[f"device_adam_speedup_vs_{base}"] = round(r[f"clip_step_{base}_us"] / r["clip_step_device_adam_us"], 2)
    # (b) the refresh: the module's tensors into a live policy handle
    pol = RecurrentPolicy({k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}, device=DEV)
    pol.reset_states(2)
    r["load_state_dict_return_us"], r["load_state_dict_done_us"] = wall_us(lambda: pol.load_state_dict(m.state_dict()), reps)
    r["load_device_state_dict_return_us"], r["load_device_state_dict_done_us"] = wall_us(
        lambda: pol.load_device_state_dict(m.state_dict()), reps)
    r["refresh_device_us"] = round(median_us(lambda: pol.load_device_state_dict(m.state_dict()), reps, 3), 1)
    r["refresh_speedup_done"] = round(r["load_state_dict_done_us"] / r["load_device_state_dict_done_us"], 2)
    pol.close()
    lines = [r]
    for L, B in shapes:
        u = dict(mode="optimizer_update", L=L, B=B, device=r["device"])
        for name, make in makers:
            mm = copy.deepcopy(m)
            res = measure_update_with(mm, make(mm.parameters()), L, B, max(B // 4, 1), max(reps // 5, 3))
            u[f"ppo_update_epoch_{name}_us"] = res.pop("ppo_update_epoch_us")
            u.update(res)
            del mm
            torch.cuda.empty_cache()
        lines.append(u)
    return lines


LOSS_ROWS = (64, 262144, 1 << 22)
LOSS_UPDATES = ((32, 2, 1), (256, 4096, 1024))   # K, n, envs_per_batch
BYTES_LOSS = 40                                  # per row: six f32 read (a seventh with a value clip), three f32 written, each once


def measure_loss(reps):
    """--loss: the loss alone per row count (forward plus the backward to the heads' three outputs), then
    one ppo_update epoch per shape with either loss path."""
    hyper = (0.3, 1e-5, 0.5)
    lines = []
    g = torch.Generator(device=DEV).manual_seed(5)
    for rows in LOSS_ROWS:
        t = [torch.randn(rows, device=DEV, generator=g) for _ in range(6)]
        t[1] = t[3] + 0.3 * t[1]                  # log_prob around old_log_prob: ratios on both sides of the clip
        leaves = [x.clone().requires_grad_() for x in t[:3]]

        def torch_path():
            loss, _ = train.ppo_loss(*leaves, *t[3:], *hyper)
            torch.autograd.grad(loss, leaves)

        r = dict(mode="loss", rows=rows, reps=reps, device=torch.cuda.get_device_name(0))
        r["loss_torch_us"] = round(median_us(torch_path, reps, 3), 1)
        r["loss_kernel_us"] = round(median_us(lambda: train.ppo_loss_kernel(*t, *hyper), reps, 3), 1)
        r["loss_kernel_no_norm_us"] = round(median_us(lambda: train.ppo_loss_kernel(*t, *hyper, False), reps, 3), 1)
        r["loss_speedup"] = round(r["loss_torch_us"] / r["loss_kernel_us"], 2)
        r["loss_floor_bytes_us"] = round(rows * BYTES_LOSS / COPY_CEILING * 1e6, 2)
        r["loss_kernel_frac_of_bytes_floor"] = round(r["loss_floor_bytes_us"] / r["loss_kernel_us"], 3)
        lines.append(r)
        del t, leaves
        torch.cuda.empty_cache()
    m = module(np.random.default_rng(0))
    for K, n, per in LOSS_UPDATES:
        u = dict(mode="loss_update", optimizer="device_adam", device=torch.cuda.get_device_name(0))
        for loss in train.LOSSES:
            mm = copy.deepcopy(m)
            res = measure_update_with(mm, train.DeviceAdam(mm.parameters(), lr=1e-5, eps=1e-5), K, n, per, reps,
                                      loss=loss)
            u[f"ppo_update_epoch_loss_{loss}_us"] = res.pop("ppo_update_epoch_us")
            u.update(res)
            del mm
            torch.cuda.empty_cache()
        u["loss_kernel_speedup"] = round(u["ppo_update_epoch_loss_torch_us"] / u["ppo_update_epoch_loss_kernel_us"], 3)
        lines.append(u)
    return lines


HEADS_ROWS = (64, 262144, 1 << 20)
# per row, each once.  Forward: h_pi, h_vf (1,024) and actions (8) read; a1, a2 of both networks (1,024), mean (8),
# values, log_prob, entropy (12) written.  Backward: a1, a2 (1,024), the three gradients (12), actions, mean (16)
# read; d_h (1,024), d_z1, d_z2 (1,024), d_mean (8) written.
BYTES_HEADS = (1024 + 8 + 1024 + 8 + 12) + (1024 + 12 + 16 + 1024 + 1024 + 8)


def measure_heads(reps):
    """--heads: the heads alone per row count (forward plus backward to h and the 13 tensors), then one
    ppo_update epoch per shape with either heads path."""
    lines = []
    g = torch.Generator(device=DEV).manual_seed(6)
    m = module(np.random.default_rng(0))
    for rows in HEADS_ROWS:
        h = [(torch.rand((rows, 128), device=DEV, generator=g) * 2 - 1).requires_grad_() for _ in range(2)]
        actions = torch.randn((rows, 2), device=DEV, generator=g)
        d = [torch.randn(rows, device=DEV, generator=g) / rows for _ in range(3)]
        w = list(m.heads_tensors())

        def torch_path():
            torch.autograd.grad(m.heads(h[0], h[1], actions), h + w, d)

        def kernel_path():
            torch.autograd.grad(train.ppo_heads(h[0], h[1], actions, *w), h + w, d)

        def kernels_alone():
            f = train.ppo_heads_forward(h[0], h[1], actions, w)
            train.ppo_heads_backward(*d, actions, {k: f[k] for k in train.HEADS_BWD_IN[4:]}, w)

        r = dict(mode="heads", rows=rows, reps=reps, device=torch.cuda.get_device_name(0))
        r["heads_torch_us"] = round(median_us(torch_path, reps, 3), 1)
        r["heads_kernel_us"] = round(median_us(kernel_path, reps, 3), 1)
        r["heads_kernels_alone_us"] = round(median_us(kernels_alone, reps, 3), 1)
        r["heads_speedup"] = round(r["heads_torch_us"] / r["heads_kernel_us"], 2)
        r["heads_floor_bytes_us"] = round(rows * BYTES_HEADS / COPY_CEILING * 1e6, 2)
        r["heads_kernels_frac_of_bytes_floor"] = round(r["heads_floor_bytes_us"] / r["heads_kernels_alone_us"], 3)
        lines.append(r)
        del h, actions, d
        torch.cuda.empty_cache()
    for K, n, per in LOSS_UPDATES:
        u = dict(mode="heads_update", optimizer="device_adam", loss="kernel", weight_grads="kernel",
                 device=torch.cuda.get_device_name(0))
        for heads in train.HEADS:
            mm = copy.deepcopy(m)
            mm.heads_mode, mm.weight_grads = heads, "kernel"
            res = measure_update_with(mm, train.DeviceAdam(mm.parameters(), lr=1e-5, eps=1e-5), K, n, per, reps,
                                      loss="kernel")
            u[f"ppo_update_epoch_heads_{heads}_us"] = res.pop("ppo_update_epoch_us")
            u.update(res)
            del mm
            torch.cuda.empty_cache()
        u["heads_kernel_speedup"] = round(u["ppo_update_epoch_heads_torch_us"] / u["ppo_update_epoch_heads_kernel_us"], 3)
        lines.append(u)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=["256,4096", "256,16384", "32,2"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out")
    ap.add_argument("--weight-grads", choices=("torch", "kernel", "both"), default="torch")
    ap.add_argument("--optimizer", action="store_true",
                    help="time the clip + optimizer step and the policy refresh against their baselines instead")
    ap.add_argument("--loss", action="store_true",
                    help="time ppo_loss_kernel against ppo_loss, alone and inside ppo_update, instead")
    ap.add_argument("--heads", action="store_true",
                    help="time ppo_heads against RecurrentPPOModule.heads, alone and inside ppo_update, instead")
    a = ap.parse_args()
    lines = []
    if a.heads:
        lines = [json.dumps(r) for r in measure_heads(a.reps)]
        print("\n".join(lines), flush=True)
    elif a.loss:
        lines = [json.dumps(r) for r in measure_loss(a.reps)]
        print("\n".join(lines), flush=True)
    elif a.optimizer:
        lines = [json.dumps(r) for r in measure_optimizer([tuple(int(v) for v in s.split(",")) for s in a.shapes], a.reps)]
        print("\n".join(lines), flush=True)
    for k, s in enumerate([] if a.optimizer or a.loss or a.heads else a.shapes):
        L, B = (int(v) for v in s.split(","))
        r, m = measure(L, B, a.reps, a.weight_grads)
        if k == 0 and a.weight_grads != "kernel":
            r.update(measure_update(m, L, B, max(B // 4, 1), max(a.reps // 5, 3)))
        del m
        torch.cuda.empty_cache()
        lines.append(json.dumps(r))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
