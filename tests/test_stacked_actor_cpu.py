"""StackedRecurrentActor on the CPU (no GPU needed): ha_host_stack_step, contract S1-S5 of
include/hedge_actor.h, against torch's stacked nn.LSTM + MLP in f64, against RecurrentActor at
128 x 1 bit for bit, and the refusals.

Tolerance of the f64 comparison: measured, not chosen.  The same torch module run in f32 on the same
inputs deviates from the f64 run by d_ref per quantity; the build has to stay within 4 x d_ref (two
valid f32 summation orders of the same terms, chain against blocked)."""
import ctypes

import numpy as np
import pytest
import torch

from cantorrl_amd import agent
from cantorrl_amd.agent import RecurrentActor, StackedRecurrentActor

CLIP, STEPS = 2.0, 3


def make_case(hid, nl, n, obs_dim=13):
    """Seeded weights as an SB3 state dict, statistics, and STEPS steps of obs / episode_start (a few
    envs start at step 1)."""
    torch.manual_seed(1000 * hid + nl)
    lstm = torch.nn.LSTM(obs_dim, hid, nl)
    mlp = torch.nn.Sequential(torch.nn.Linear(hid, 64), torch.nn.Tanh(), torch.nn.Linear(64, 64), torch.nn.Tanh(),
                              torch.nn.Linear(64, 2))
    sd = {"lstm_actor." + k: v for k, v in lstm.state_dict().items()}
    sd.update({f"mlp_extractor.policy_net.{i}.{p}": getattr(mlp[i], p).detach() for i in (0, 2) for p in ("weight", "bias")})
    sd.update({"action_net.weight": mlp[4].weight.detach(), "action_net.bias": mlp[4].bias.detach(),
               "log_std": torch.zeros(2)})
    rng = np.random.default_rng(hid + nl + n)
    stats = {"obs_mean": rng.uniform(-1, 1, obs_dim), "obs_var": rng.uniform(4, 36, obs_dim)}
    obs = rng.uniform(-10, 10, (STEPS, n, obs_dim)).astype(np.float32)
    start = np.zeros((STEPS, n), np.uint8)
    start[1, ::3] = 1
    return sd, stats, obs, start, (lstm, mlp)


def torch_sequence(mods, stats, obs, start, dtype):
    """The module stepped one time step at a time in `dtype`, the state zeroed at starts ->
    actions, mean [T,n,2], h, c [T,NL,n,H] as f64 arrays."""
    lstm, mlp = (m.to(dtype) for m in mods)
    z = np.clip((obs.astype(np.float64) - stats["obs_mean"]) / np.sqrt(stats["obs_var"] + 1e-8), -CLIP, CLIP)
    x = torch.from_numpy(z.astype(np.float32)).to(dtype)   # S2: rounded once to f32
    h = torch.zeros(lstm.num_layers, obs.shape[1], lstm.hidden_size, dtype=dtype)
    c = torch.zeros_like(h)
    out = {k: [] for k in ("actions", "mean", "h", "c")}
    with torch.no_grad():
        for t in range(obs.shape[0]):
            keep = torch.from_numpy(1.0 - start[t]).to(dtype)[None, :, None]
            y, (h, c) = lstm(x[t][None], (h * keep, c * keep))
            mean = mlp(y[0])
            for k, v in (("actions", mean.clamp(-1.0, 1.0)), ("mean", mean), ("h", h), ("c", c)):
                out[k].append(v.double().numpy())
    return {k: np.stack(v) for k, v in out.items()}


def host_sequence(actor, obs, start, n):
    """host_step over the steps -> the same dict, plus obs_norm [T,n,13]."""
    h, c = (np.zeros(actor._state_shape(n), np.float32) for _ in range(2))
    out = {k: [] for k in ("actions", "mean", "obs_norm", "h", "c")}
    for t in range(obs.shape[0]):
        mean, xn = np.empty((n, 2), np.float32), np.empty((n, 13), np.float32)
        a = actor.host_step(obs[t], start[t], h, c, mean_out=mean, obs_norm_out=xn)
        for k, v in (("actions", a), ("mean", mean), ("obs_norm", xn), ("h", h.copy()), ("c", c.copy())):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


@pytest.mark.parametrize("hid,nl", [(128, 2), (256, 1), (512, 4)])
def test_host_step_matches_torch_f64_within_4_d_ref(hid, nl):
    n = 33
    sd, stats, obs, start, mods = make_case(hid, nl, n)
    f32 = torch_sequence(mods, stats, obs, start, torch.float32)
    f64 = torch_sequence(mods, stats, obs, start, torch.float64)
    got = host_sequence(StackedRecurrentActor.from_state_dict(sd, normalization=stats, clip_obs=CLIP), obs, start, n)
    assert got["h"].shape == (STEPS, nl, n, hid) and np.abs(got["h"][-1]).mean() > 0.0
    for k in ("actions", "mean", "h", "c"):
        d_ref, err = float(np.abs(f32[k] - f64[k]).max()), float(np.abs(got[k] - f64[k]).max())
        print(f"{hid} x {nl} {k}: build {err:.3e} torch f32 {d_ref:.3e}")
        assert d_ref > 0.0 and err <= 4 * d_ref, (k, err, d_ref)


def test_128_x_1_equals_recurrent_actor_bitwise():
    n = 33
    sd, stats, obs, start, _ = make_case(128, 1, n)
    got = host_sequence(StackedRecurrentActor.from_state_dict(sd, normalization=stats, clip_obs=CLIP), obs, start, n)
    old = host_sequence(RecurrentActor.from_state_dict(sd, normalization=stats, clip_obs=CLIP), obs, start, n)
    for k in old:
        assert np.array_equal(got[k].reshape(old[k].shape).view(np.uint32), old[k].view(np.uint32)), k


@pytest.mark.parametrize("hid,nl,obs_dim,drop", [(64, 1, 13, None), (128, 5, 13, None), (128, 1, 12, None),
                                                 (128, 2, 13, "lstm_actor.weight_hh_l1")])
def test_loader_refuses_other_architectures(hid, nl, obs_dim, drop):
    sd = make_case(hid, nl, 1, obs_dim)[0]
    sd.pop(drop, None)
    with pytest.raises(ValueError):
        StackedRecurrentActor.from_state_dict(sd)


def test_abi_refuses_hidden_192():
    sd, _, obs, start, _ = make_case(128, 1, 1)
    actor = StackedRecurrentActor.from_state_dict(sd)
    w = agent.HaStackWeights.from_buffer_copy(actor._w)
    w.hidden = 192
    z, a = np.zeros((1, 1, 128), np.float32), np.zeros((1, 2), np.float32)
    st = actor.lib.ha_host_stack_step(ctypes.byref(w), 1, obs[0].ctypes.data, start[0].ctypes.data, z.ctypes.data,
                                      z.ctypes.data, a.ctypes.data, None, None)
    assert st == 2 and b"hidden" in actor.lib.ha_last_error(None)
