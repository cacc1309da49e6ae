"""lstm_seq_fwd_kernel / lstm_seq_bwd_kernel on the GPU against the host build of the same arithmetic
bit for bit (h, c, gates, d_gates; one network and the actor / critic pair; every shape and start
pattern of test_lstm_seq_cpu.py) -- which is also the hardware check that the backward's
v_mfma_f32_32x32x2_f32 chain over K = 512 is the contract's k-ordered fmaf chain --, against the
states a RolloutCollector stored, and torch.autograd through lstm_sequence on the device within the
CPU test's bound (4 x d_ref against the f64 restatement)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_lstm_seq_cpu import (ACTOR, BS, GRAD_NAMES, LS, PATTERNS, WEIGHTS, autograd_reference, d_h_for, host_backward,
                               net_inputs, seq_case)
from test_policy_collect_cpu import bits, critic_golden, make_policy

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cantorrl_amd import train  # noqa: E402
from cantorrl_amd.collect import RolloutCollector  # noqa: E402

DEV = "cuda:0"


def on_device(nets):
    return [{k: v.to(DEV) for k, v in n.items()} for n in nets]


@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", WEIGHTS)
def test_device_forward_and_backward_equal_the_host_build_bitwise(kind, pattern, B):
    for L in LS:
        case = seq_case(kind, pattern, L, B)
        d_h = d_h_for(case)
        want_dg = host_backward(kind, case, d_h)
        x, es = torch.from_numpy(case["x"]).to(DEV), torch.from_numpy(case["es"]).to(DEV)
        nets = on_device(net_inputs(kind, case["states"]))
        for pick in ((0, 1), (0,), (1,)):   # the pair in one launch, then each network alone
            out = train.lstm_seq_forward(x, es, [nets[k] for k in pick])
            bwd = [dict(w_hh=nets[k]["w_hh"], c0=nets[k]["c0"], c=o[1], gates=o[2], d_h=d_h[k].to(DEV))
                   for k, o in zip(pick, out)]
            dg = train.lstm_seq_backward(es, bwd)
            torch.cuda.synchronize()
            for k, o, g in zip(pick, out, dg):
                for name, got, want in zip(("h", "c", "gates"), o, case["out"][k]):
                    assert np.array_equal(bits(got.cpu().numpy()), bits(want.numpy())), (name, L, k, pick)
                assert np.array_equal(bits(g.cpu().numpy()), bits(want_dg[k].numpy())), ("d_gates", L, k, pick)
        assert float(want_dg[0].abs().max()) > 1e-3 and torch.isfinite(want_dg[1]).all()


def short_replay_env(n, seed):
    """The replay golden's tables cut to 6-step episodes: episode ends fall inside a 16-step rollout."""
    from cantorrl_amd.vec_env import HedgingVecEnv
    from oracle.hedging_oracle import load_golden
    cfg, d = load_golden(os.path.join(GOLDEN, "g1_v2_train.npz"))
    tables = tuple(np.ascontiguousarray(d[k][:, :T]) for k, T in (("paths", 7), ("volatilities", 7), ("call_prices_atm", 6),
                                                                   ("put_prices_atm", 6)))
    return HedgingVecEnv(n, tables=tables, variant=int(d["variant"]), seed=seed, info_keys=("per_share_step_pnl",),
                         return_numpy=False, device=DEV, **cfg)


def test_sequence_reproduces_the_states_the_collector_stored():
    n, K = 33, 16
    c = critic_golden()
    pol = make_policy("golden", norm=False, device=DEV)
    venv = short_replay_env(n, 11)
    col = RolloutCollector(venv, pol, float(c["gamma"]), float(c["gae_lambda"]), seed=5)
    col.collect(5)                      # the rollout under test begins mid-episode, from non-zero states
    buf = col.collect(K, states=True)
    torch.cuda.synchronize()
    es = buf.episode_starts
    assert es.shape == (K, n) and es[1:].sum() >= 2 * n and not es[0].any() and buf.h_pi.abs().mean() > 0
    m = train.RecurrentPPOModule.from_policy(pol)
    actor = (buf.h_pi, buf.c_pi, *m.lstm_actor.tensors())
    critic = (buf.h_vf, buf.c_vf, *m.lstm_critic.tensors())
    with torch.no_grad():
        h_pi, h_vf = train.lstm_sequence_pair(buf.observations, es, actor, critic)
    nets = [dict(zip(train.NET_INPUTS, t)) for t in (actor, critic)]
    out = train.lstm_seq_forward(buf.observations, es, nets)
    torch.cuda.synchronize()
    assert torch.equal(h_pi, out[0][0]) and torch.equal(h_vf, out[1][0])
    for k in range(K - 1):
        nxt = buf.states[k + 1].cpu().numpy()   # the states fed to step k + 1 = the states step k left
        for i, (net, which) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
            assert np.array_equal(bits(out[net][which][k].cpu().numpy()), bits(nxt[:, i])), (k, i)
    for i, t in enumerate(pol.states):          # and the last step left the policy's live states
        net, which = divmod(i, 2)
        assert np.array_equal(bits(out[net][which][K - 1].cpu().numpy()), bits(t.cpu().numpy()))
    venv.close()
    pol.close()


@pytest.mark.parametrize("kind", WEIGHTS)
def test_autograd_on_the_device_within_4_d_ref(kind):
    for pattern, L, B in (("mid", 9, 33), ("ends", 40, 65)):
        case = seq_case(kind, pattern, L, B)
        cpu_nets = net_inputs(kind, case["states"])
        nets = on_device(cpu_nets)
        x, es = torch.from_numpy(case["x"]), torch.from_numpy(case["es"])
        d_h = d_h_for(case)
        w = [[n[k].clone().requires_grad_() for k in ACTOR] for n in nets]
        h = train.lstm_sequence_pair(x.to(DEV), es.to(DEV), (nets[0]["h0"], nets[0]["c0"], *w[0]),
                                     (nets[1]["h0"], nets[1]["c0"], *w[1]))
        ((h[0] * d_h[0].to(DEV)).sum() + (h[1] * d_h[1].to(DEV)).sum()).backward()
        torch.cuda.synchronize()
        for k in range(2):
            assert np.array_equal(bits(h[k].detach().cpu().numpy()), bits(case["out"][k][0].numpy()))
            r64 = autograd_reference(cpu_nets[k], x, es, d_h[k], torch.float64)
            r32 = autograd_reference(cpu_nets[k], x, es, d_h[k], torch.float32)
            for name, p, b, r in zip(GRAD_NAMES[1:], w[k], r32[1:], r64[1:]):
                err, d_ref = float((p.grad.cpu().double() - r).abs().max()), float((b - r).abs().max())
                print(f"{kind} {pattern} L {L} B {B} net {k} {name}: device {err:.3e} reference {d_ref:.3e}")
                assert err <= 4 * d_ref, (name, err, d_ref)
