"""Device time of rollout collection (agent.RecurrentPolicy, collect.RolloutCollector): ha_step (the
actor alone, the yardstick's unit), ha_policy_step (actor + critic + sampling + log-prob, one launch),
ha_gae at K = 256, RolloutCollector.collect per step, and -- same box, same process -- what a user
has without the kernel: the same step composed from torch ops on the device (two LSTMCells, six
Linears, Normal.sample / log_prob, f32).  HIP events around each call, warm-up first, the median.

    python tools/collect_time.py [n_envs ...] [--reps R] [--out FILE.jsonl]

Defaults: 65,536 envs and 2 (the reference's N_ENVS).  One JSON line per size; with --out they are
appended to the file as well (profiles/collect_time_*.jsonl).  ha_policy_step is ha_step's tile work
twice plus, per env, one Philox block, one Box-Muller and two f64 divisions, so the yardstick is
2 x ha_step of the same run (`policy_over_2x_actor`, target <= 1.10).
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from actor_time import GEN, median_us  # noqa: E402
from cantorrl_amd.agent import ACTOR_KEYS, POLICY_KEYS, RecurrentActor, RecurrentPolicy  # noqa: E402
from cantorrl_amd.collect import RolloutCollector  # noqa: E402
from cantorrl_amd.vec_env import HedgingVecEnv  # noqa: E402

GAMMA, GAE_LAMBDA, K_GAE = 0.9824221777549808, 0.9178809896340236, 256


class TorchPolicy(torch.nn.Module):
    """The same step from torch ops: normalise, reset the states, two LSTMCells, 2 x (two Linear +
    tanh + head), Normal.sample, log_prob, clip."""

    def __init__(self, w, mean, var):
        super().__init__()
        L = torch.nn.Linear
        self.cell_pi, self.cell_vf = torch.nn.LSTMCell(13, 128), torch.nn.LSTMCell(13, 128)
        self.p1, self.p2, self.p3 = L(128, 64), L(64, 64), L(64, 2)
        self.v1, self.v2, self.v3 = L(128, 64), L(64, 64), L(64, 1)
        pairs = ((self.cell_pi.weight_ih, "w_ih"), (self.cell_pi.weight_hh, "w_hh"), (self.cell_pi.bias_ih, "b_ih"),
                 (self.cell_pi.bias_hh, "b_hh"), (self.p1.weight, "w1"), (self.p1.bias, "b1"), (self.p2.weight, "w2"),
                 (self.p2.bias, "b2"), (self.p3.weight, "w3"), (self.p3.bias, "b3"),
                 (self.cell_vf.weight_ih, "c_w_ih"), (self.cell_vf.weight_hh, "c_w_hh"), (self.cell_vf.bias_ih, "c_b_ih"),
                 (self.cell_vf.bias_hh, "c_b_hh"), (self.v1.weight, "v1"), (self.v1.bias, "vb1"), (self.v2.weight, "v2"),
                 (self.v2.bias, "vb2"), (self.v3.weight, "v3"), (self.v3.bias, "vb3"))
        with torch.no_grad():
            for p, f in pairs:
                p.copy_(torch.from_numpy(w[f]))
        self.register_buffer("mean", torch.from_numpy(mean).float())
        self.register_buffer("inv_sd", torch.from_numpy(1.0 / np.sqrt(var + 1e-8)).float())
        self.register_buffer("log_std", torch.from_numpy(w["log_std"]))

    @torch.no_grad()
    def forward(self, obs, start, st):
        x = torch.clamp((obs - self.mean) * self.inv_sd, -10.0, 10.0)
        keep = (1 - start).to(torch.float32).unsqueeze(1)
        h_pi, c_pi = self.cell_pi(x, (st[0] * keep, st[1] * keep))
        h_vf, c_vf = self.cell_vf(x, (st[2] * keep, st[3] * keep))
        mean = self.p3(torch.tanh(self.p2(torch.tanh(self.p1(h_pi)))))
        value = self.v3(torch.tanh(self.v2(torch.tanh(self.v1(h_vf))))).flatten()
        dist = torch.distributions.Normal(mean, self.log_std.exp().expand_as(mean))
        a = dist.sample()
        return a, torch.clamp(a, -1.0, 1.0), value, dist.log_prob(a).sum(-1), (h_pi, c_pi, h_vf, c_vf)


def measure(n, reps):
    dev = "cuda:0"
    rng = np.random.default_rng(0)
    w = {f: (rng.uniform(-1, 1, shape) / np.sqrt(shape[-1])).astype(np.float32) for _, f, shape in POLICY_KEYS}
    mean, var = rng.uniform(-1, 1, 13), rng.uniform(0.5, 2.0, 13)
    obs = torch.from_numpy(rng.uniform(-2, 2, (n, 13)).astype(np.float32)).to(dev)
    start = torch.zeros(n, dtype=torch.uint8, device=dev)

    actor = RecurrentActor({f: w[f] for _, f, _ in ACTOR_KEYS}, obs_mean=mean, obs_var=var, device=dev)
    out = torch.empty((n, 2), device=dev)
    actor.reset_states(n)
    t_actor = median_us(lambda: actor.step(obs, start, out=out), reps)
    actor.close()

    pol = RecurrentPolicy(w, obs_mean=mean, obs_var=var, device=dev)
    pol.reset_states(n)
    res = pol.step(obs, start, 1, 0)
    idx = [0]

    def policy_step():
        idx[0] += 1
        pol.step(obs, start, 1, idx[0], out=res)
    t_policy = median_us(policy_step, reps)

    K = K_GAE
    cols = [torch.from_numpy(rng.normal(0, 1, (K, n)).astype(np.float32)).to(dev) for _ in range(2)]
    es = torch.from_numpy((rng.uniform(size=(K, n)) < 0.004).astype(np.uint8)).to(dev)
    lv, ld = torch.zeros(n, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev)
    adv, ret = torch.empty((K, n), device=dev), torch.empty((K, n), device=dev)
    t_gae = median_us(lambda: pol.gae(cols[0], cols[1], es, lv, ld, GAMMA, GAE_LAMBDA, advantages=adv, returns=ret), reps)
    del cols, es, adv, ret

    tp = TorchPolicy(w, mean, var).to(dev)
    st = [tuple(torch.zeros((n, 128), device=dev) for _ in range(4))]

    def torch_step():
        st[0] = tp(obs, start, st[0])[4]
    t_torch = median_us(torch_step, reps)

    venv = HedgingVecEnv(n, mode="gbm", generate=GEN, seed=42, return_numpy=False, info_keys=("per_share_step_pnl",))
    col = RolloutCollector(venv, pol, GAMMA, GAE_LAMBDA, seed=7)
    Kc = 16
    buf = col.collect(Kc)
    t_collect = median_us(lambda: col.collect(Kc, buffer=buf), max(reps // 4, 5), 2) / Kc
    act = torch.zeros((n, 2), device=dev)
    t_env = median_us(lambda: venv.step_tensors(act, terminal_obs=False, info=False), reps)
    venv.close()
    pol.close()
    return dict(n_envs=n, ha_step_us=round(t_actor, 2), ha_policy_step_us=round(t_policy, 2),
                policy_over_2x_actor=round(t_policy / (2 * t_actor), 4), ha_gae_k256_us=round(t_gae, 2),
                collect_us_per_step=round(t_collect, 2), he_step_us=round(t_env, 2), torch_step_us=round(t_torch, 2),
                speedup_vs_torch=round(t_torch / t_policy, 2), reps=reps, device=torch.cuda.get_device_name(0))


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
