"""Device time of the RecurrentPPO actor (libhedgeactor, agent.RecurrentActor): ha_step alone,
HedgingVecEnv.rollout_actor per step (ha_step + he_step + ha_accumulate), and -- same box, same
process -- what a user has without the kernel: the same step composed from torch ops on the
device (torch.nn.LSTMCell + Linear, f32).  HIP events around each call, warm-up first, the median.

    python tools/actor_time.py [n_envs ...] [--reps R] [--out FILE.jsonl]

Defaults: 65,536 envs and 2 (the reference's N_ENVS).  One JSON line per size; with --out they are
appended to the file as well (profiles/actor_time_*.jsonl).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cantorrl_amd.agent import ACTOR_KEYS, RECORD_INFO_KEYS, RecurrentActor  # noqa: E402
from cantorrl_amd.vec_env import HedgingVecEnv  # noqa: E402

FLOP_PER_ENV_STEP = 2 * (512 * 141 + 64 * 128 + 64 * 64 + 2 * 64)   # 169,216
F32_MATRIX_PEAK = 157.3e12
GEN = dict(s0=496.48001098632812, variance=0.029028, mu=0.04, dt=1 / 252, episode_length=252)


def median_us(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3


class TorchActor(torch.nn.Module):
    """The same step from torch ops: normalise, reset the state, LSTMCell, two Linear + tanh,
    the action head, clip."""

    def __init__(self, w, mean, var):
        super().__init__()
        self.cell = torch.nn.LSTMCell(13, 128)
        self.l1, self.l2, self.head = torch.nn.Linear(128, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 2)
        with torch.no_grad():
            for p, f in ((self.cell.weight_ih, "w_ih"), (self.cell.weight_hh, "w_hh"), (self.cell.bias_ih, "b_ih"),
                         (self.cell.bias_hh, "b_hh"), (self.l1.weight, "w1"), (self.l1.bias, "b1"),
                         (self.l2.weight, "w2"), (self.l2.bias, "b2"), (self.head.weight, "w3"), (self.head.bias, "b3")):
                p.copy_(torch.from_numpy(w[f]))
        self.register_buffer("mean", torch.from_numpy(mean).float())
        self.register_buffer("inv_sd", torch.from_numpy(1.0 / np.sqrt(var + 1e-8)).float())

    @torch.no_grad()
    def forward(self, obs, start, h, c):
        x = torch.clamp((obs - self.mean) * self.inv_sd, -10.0, 10.0)
        keep = (1 - start).to(torch.float32).unsqueeze(1)
        h, c = self.cell(x, (h * keep, c * keep))
        a = torch.tanh(self.l2(torch.tanh(self.l1(h))))
        return torch.clamp(self.head(a), -1.0, 1.0), h, c


def measure(n, reps):
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    w = {f: (rng.uniform(-1, 1, shape) / np.sqrt(shape[-1])).astype(np.float32) for _, f, shape in ACTOR_KEYS}
    mean, var = rng.uniform(-1, 1, 13), rng.uniform(0.5, 2.0, 13)
    actor = RecurrentActor(w, obs_mean=mean, obs_var=var, device=dev)
    obs = torch.from_numpy(rng.uniform(-2, 2, (n, 13)).astype(np.float32)).to(dev)
    start = torch.zeros(n, dtype=torch.uint8, device=dev)
    out = torch.empty((n, 2), device=dev)
    actor.reset_states(n)
    t_kernel = median_us(lambda: actor.step(obs, start, out=out), reps)

    ta = TorchActor(w, mean, var).to(dev)
    st = [torch.zeros((n, 128), device=dev), torch.zeros((n, 128), device=dev)]

    def torch_step():
        _, st[0], st[1] = ta(obs, start, st[0], st[1])
    t_torch = median_us(torch_step, reps)

    venv = HedgingVecEnv(n, mode="gbm", generate=GEN, seed=42, return_numpy=False, info_keys=RECORD_INFO_KEYS)
    venv.reset_tensors()
    recs = torch.zeros((2 * n, 80), dtype=torch.uint8, device=dev)
    cnt = torch.zeros(1, dtype=torch.int64, device=dev)
    K = 16
    t_roll = median_us(lambda: venv.rollout_actor(actor, K, records=recs, record_count=cnt), max(reps // 4, 5), 2) / K
    act = torch.zeros((n, 2), device=dev)
    t_env = median_us(lambda: venv.step_tensors(act, terminal_obs=False), reps)
    venv.close()
    actor.close()
    tf = n * FLOP_PER_ENV_STEP / (t_kernel * 1e-6)
    return dict(n_envs=n, ha_step_us=round(t_kernel, 2), torch_step_us=round(t_torch, 2),
                rollout_actor_us_per_step=round(t_roll, 2), he_step_us=round(t_env, 2),
                ha_step_tflops=round(tf / 1e12, 3), frac_f32_matrix_peak=round(tf / F32_MATRIX_PEAK, 4),
                speedup_vs_torch=round(t_torch / t_kernel, 2), reps=reps, device=torch.cuda.get_device_name(0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n_envs", nargs="*", type=int, default=[65536, 2])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out")
    a = ap.parse_args()
    for n in a.n_envs:
        line = json.dumps(measure(n, a.reps))
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
