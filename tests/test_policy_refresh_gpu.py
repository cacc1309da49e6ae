"""RecurrentPolicy.load_device_state_dict on the GPU (ha_policy_refresh, policy_pack_kernel): a handle
re-packed from device tensors against a fresh handle made from the same values on the host, bit for
bit; the host copies that follow on demand; what it refuses; and the training iteration it closes with
train.DeviceAdam: collect -> ppo_update -> load_device_state_dict -> collect."""
import copy

import numpy as np
import pytest

from test_policy_collect_cpu import bits, make_policy, policy_state_dict, random_policy_weights, zero_states
from test_ppo_update_gpu import HYPER, clipped_grads, rollout, states0

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cantorrl_amd import train  # noqa: E402
from cantorrl_amd.agent import (POLICY_KEYS, STATE_NAMES, STEP_OUTPUTS, RecurrentPolicy,  # noqa: E402
                                policy_weights_from_state_dict)

DEV = "cuda:0"
SEED = 0x51ED270B9F3C11A7


def fields(kind):
    if kind == "golden":
        return policy_weights_from_state_dict(policy_state_dict())
    return random_policy_weights(7)


def statistics(with_stats):
    rng = np.random.default_rng(99)
    return dict(obs_mean=rng.uniform(-1, 1, 13), obs_var=rng.uniform(4, 36, 13)) if with_stats else {}


def on_device(weights):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in weights.items()}


def three_steps(pol, n, deterministic, rng_seed=5):
    """Three device steps from zeroed states (starts: all, some, none) -> ([outputs per step], states)."""
    rng = np.random.default_rng(rng_seed)
    pol.reset_states(n)
    outs, inputs = [], []
    for s, start in enumerate((np.ones(n, np.uint8), (rng.uniform(size=n) < 0.5).astype(np.uint8), np.zeros(n, np.uint8))):
        obs = rng.uniform(-10, 10, (n, 13)).astype(np.float32)
        out = {name: torch.full((n,) + tail, 7.0, device=DEV) for name, tail in STEP_OUTPUTS}
        outs.append(pol.step(torch.from_numpy(obs).to(DEV), torch.from_numpy(start).to(DEV), SEED, 40 + s,
                             deterministic=deterministic, env_id_offset=3 * n, out=out))
        inputs.append((obs, start))
    torch.cuda.synchronize()
    return outs, [t.clone() for t in pol.states], inputs


@pytest.mark.parametrize("with_stats", [True, False])
@pytest.mark.parametrize("deterministic", [False, True])
@pytest.mark.parametrize("kind", ["golden", "random"])
@pytest.mark.parametrize("n", [1, 33, 65])
def test_refreshed_handle_equals_a_fresh_handle_and_the_host_build_bitwise(n, kind, deterministic, with_stats):
    a, b = fields("random" if kind == "golden" else "golden"), fields(kind)
    pol = RecurrentPolicy(a, device=DEV, **statistics(with_stats))
    before, _, _ = three_steps(pol, n, deterministic)
    pol.load_device_state_dict(on_device(b))
    fresh = RecurrentPolicy(b, device=DEV, **statistics(with_stats))
    got, got_states, inputs = three_steps(pol, n, deterministic)
    want, want_states, _ = three_steps(fresh, n, deterministic)
    for s in range(3):
        for name, _ in STEP_OUTPUTS:
            assert torch.equal(got[s][name], want[s][name]), (name, s)
    for name, x, y in zip(STATE_NAMES, got_states, want_states):
        assert torch.equal(x, y), name
    assert not torch.equal(before[2]["values"], got[2]["values"])        # the refresh changed the tensors
    assert not torch.equal(before[2]["actions"], got[2]["actions"])
    # the host build of the refreshed object runs the new tensors too (the download happens here)
    host = zero_states(n)
    for s, (obs, start) in enumerate(inputs):
        h = pol.host_step(obs, start, host, SEED, 40 + s, deterministic=deterministic, env_id_offset=3 * n)
        for name, _ in STEP_OUTPUTS:
            assert np.array_equal(bits(got[s][name].cpu().numpy()), bits(h[name])), (name, s)
    for name, x, y in zip(STATE_NAMES, got_states, host):
        assert np.array_equal(bits(x.cpu().numpy()), bits(y)), name
    pol.close()
    fresh.close()


def test_host_copies_follow_a_refresh_on_demand():
    b = fields("random")
    pol = make_policy("golden", device=DEV)
    sd_b = {key: torch.from_numpy(b[f].copy()).to(DEV) for key, f, _ in POLICY_KEYS}   # a state dict's own names
    pol.load_device_state_dict(sd_b)
    for t in sd_b.values():
        t.add_(1.0)            # enqueued behind the refresh: the handle and its copy hold the values it read
    m = train.RecurrentPPOModule.from_policy(pol)
    got = m.state_dict()
    for key, f, _ in POLICY_KEYS:
        assert got[key].device.type == "cuda"
        assert np.array_equal(bits(got[key].cpu().numpy()), bits(b[f])), key
    # a later host upload of other values wins over the refresh, and a refresh after it wins again
    a = fields("golden")
    pol.load_state_dict(a)
    assert np.array_equal(pol._host_weights()[1]["c_w_hh"], a["c_w_hh"])
    pol.load_device_state_dict(on_device(b))
    assert np.array_equal(bits(pol._host_weights()[1]["c_w_hh"]), bits(b["c_w_hh"]))
    assert np.array_equal(bits(pol._host_weights()[1]["log_std"]), bits(b["log_std"]))
    # a policy without a handle yet makes one
    cold = RecurrentPolicy(a, device=DEV)
    assert cold._h is None
    cold.load_device_state_dict(on_device(b))
    n = 33
    want, _, _ = three_steps(RecurrentPolicy(b, device=DEV), n, False)
    got, _, _ = three_steps(cold, n, False)
    assert torch.equal(got[2]["log_probs"], want[2]["log_probs"]) and torch.equal(got[2]["values"], want[2]["values"])
    # closing keeps the refreshed values: a handle made afterwards runs them
    cold.close()
    again, _, _ = three_steps(cold, n, False)
    assert torch.equal(again[2]["values"], want[2]["values"])
    cold.close()
    pol.close()


def test_refresh_refuses_what_is_not_a_device_float32_tensor_of_the_shape_and_keeps_the_handle():
    n = 33
    pol = make_policy("random", device=DEV)
    before, _, _ = three_steps(pol, n, True)
    good = on_device(fields("golden"))
    for field, bad, match in (("w_hh", good["w_hh"].cpu(), "on cuda"), ("w1", good["w1"].double(), "float32"),
                              ("c_b_ih", good["c_b_ih"][:-1].clone(), "shape"), ("v3", good["v3"].t(), "shape"),
                              ("w_ih", good["w_hh"][:, :13], "contiguous"),
                              ("log_std", good["log_std"].cpu().numpy(), "float32")):
        with pytest.raises(ValueError, match=match):
            pol.load_device_state_dict(dict(good, **{field: bad}))
    missing = dict(good)
    del missing["vb3"]
    with pytest.raises(ValueError, match="vb3"):
        pol.load_device_state_dict(missing)
    after, _, _ = three_steps(pol, n, True)
    for name, _ in STEP_OUTPUTS:
        assert torch.equal(before[2][name], after[2][name]), name
    assert not pol._host_stale
    pol.close()


def test_collect_device_adam_update_refresh_collect_cycle():
    pol, venv, col, buf = rollout()
    m = train.RecurrentPPOModule.from_policy(pol)
    opt = train.DeviceAdam(m.parameters(), lr=1e-3, eps=1e-5)
    with torch.no_grad():
        v0 = m.evaluate_actions(buf.observations, buf.actions, buf.episode_starts, states0(buf))[0].clone()
    gen = torch.Generator(device=DEV).manual_seed(3)
    stats = train.ppo_update(m, opt, buf, n_epochs=2, envs_per_batch=16, window=8, generator=gen, **HYPER)
    with torch.no_grad():
        v1 = m.evaluate_actions(buf.observations, buf.actions, buf.episode_starts, states0(buf))[0]
    assert all(bool(torch.isfinite(v)) for v in stats.values())
    assert stats["grad_norm"].device.type == "cuda" and float(stats["grad_norm"]) > 0.0
    assert float((v1 - v0).abs().max()) > 1e-4          # the update changed the critic
    assert int(opt.state[m.log_std]["step"]) == 2 * 3 * 2   # epochs x groups of 16 among 33 envs x windows
    pol.load_device_state_dict(m.state_dict())
    buf2 = col.collect(16, states=True)
    torch.cuda.synchronize()
    with torch.no_grad():
        v2, lp2, _ = m.evaluate_actions(buf2.observations, buf2.actions, buf2.episode_starts, states0(buf2))
    # the collector now runs the updated tensors: the module reproduces what it stored
    assert torch.isfinite(buf2.values).all()
    assert float((v2 - buf2.values).abs().max()) <= 1e-4 * max(1.0, float(buf2.values.abs().max()))
    ckpt = make_policy("golden", device=DEV)
    m0 = train.RecurrentPPOModule.from_policy(ckpt)
    with torch.no_grad():
        old = m0.evaluate_actions(buf2.observations, buf2.actions, buf2.episode_starts, states0(buf2))[0]
    assert float((old - buf2.values).abs().max()) > 1e-4   # and the checkpoint's own tensors do not
    venv.close()
    pol.close()
    ckpt.close()


def test_one_minibatch_with_device_adam_moves_the_parameters_as_torch_adam_does():
    """The reference: Adam's first step (m-hat = g, v-hat = g g) in f64 from the all-torch f64 module's
    clipped gradient.  d_ref: how far ppo_update with torch.optim.Adam lands from it, per tensor; the
    same update with DeviceAdam has to stay within 4 x d_ref plus one ulp of the largest parameter."""
    pol, venv, col, buf = rollout()
    lr, eps = 1e-3, 1e-5
    m = train.RecurrentPPOModule.from_policy(pol)
    g64 = clipped_grads(copy.deepcopy(m).double(), buf)
    before = {k: p.detach().clone() for k, p in m.named_parameters()}
    moved = {}
    for name, make in (("torch", lambda ps: torch.optim.Adam(ps, lr=lr, eps=eps)),
                       ("device", lambda ps: train.DeviceAdam(ps, lr=lr, eps=eps))):
        mm = copy.deepcopy(m)
        stats = train.ppo_update(mm, make(mm.parameters()), buf, n_epochs=1, **HYPER)
        torch.cuda.synchronize()
        assert bool(torch.isfinite(stats["grad_norm"])) and stats["grad_norm"].device.type == "cuda"
        moved[name] = {k: p.detach().double() - before[k].double() for k, p in mm.named_parameters()}
    assert len(before) == 21
    for k in before:
        want = -lr * g64[k] / (g64[k].abs() + eps)
        d_ref = float((moved["torch"][k] - want).abs().max())
        err = float((moved["device"][k] - want).abs().max())
        ulp = float(torch.finfo(torch.float32).eps * before[k].abs().max())
        print(f"{k}: DeviceAdam {err:.3e} torch.optim.Adam {d_ref:.3e} ulp {ulp:.3e} |step| {float(want.abs().max()):.3e}")
        assert float(want.abs().max()) > 0.0, k
        assert err <= 4 * d_ref + ulp, (k, err, d_ref, ulp)
    venv.close()
    pol.close()
