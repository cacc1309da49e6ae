"""lstm_wgrad_kernel / lstm_wgrad_reduce_kernel on the GPU against the host build of contract W1-W4
bit for bit (d_w_ih, d_w_hh, d_b; one network and the actor / critic pair) -- which is also the
hardware check that v_mfma_f32_32x32x2_f32 with the row index as its k accumulates a block in W1's
order --, torch.autograd through lstm_sequence(weight_grads="kernel") on the device and one PPO
minibatch of a weight_grads="kernel" module within 4 x d_ref of the f64 restatement, and the default
path's gradients unchanged."""
import copy

import numpy as np
import pytest

import _ppo_reference as ref
from test_lstm_seq_cpu import (ACTOR, BS, GRAD_NAMES, LS, PATTERNS, WEIGHTS, bits, d_h_for, host_backward, net_inputs, policy,
                               seq_case, torch_lstm_loop)
from test_lstm_wgrad_cpu import BLOCK, CHUNK, T, host_wgrad, random_case, references
from test_ppo_update_gpu import HYPER, loop_evaluate, rollout, states0

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cantorrl_amd import train  # noqa: E402

DEV = "cuda:0"
PICKS = ((0, 1), (0,), (1,))   # the pair in one call, then each network alone


def assert_device_equals_host(x, es, nets, what):
    """nets: two dicts of NumPy d_gates, h, h0."""
    want = host_wgrad(x, es, nets)
    xd, ed = T(x).to(DEV), T(es).to(DEV)
    dn = [{k: T(v).to(DEV) for k, v in n.items()} for n in nets]
    for pick in PICKS:
        got = train.lstm_seq_weight_grads(xd, ed, [dn[k] for k in pick])
        torch.cuda.synchronize()
        for k, g in zip(pick, got):
            for name, a, b in zip(("d_w_ih", "d_w_hh", "d_b"), g, want[k]):
                assert np.array_equal(bits(a.cpu().numpy()), bits(b)), (what, name, k, pick)
    assert all(np.abs(w[1]).max() > 0 or es.all() for w in want)


def real_nets(kind, case):
    d_gates = host_backward(kind, case, d_h_for(case))
    return [dict(d_gates=dg.numpy(), h=o[0].numpy(), h0=case["states"][2 * k])
            for k, (dg, o) in enumerate(zip(d_gates, case["out"]))]


@pytest.mark.parametrize("B", BS)
def test_device_equals_the_host_build_bitwise_on_the_sequence_cases(B):
    for L in LS:
        case = seq_case("golden", "mid", L, B)
        assert_device_equals_host(case["x"], case["es"], real_nets("golden", case), (L, B))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", WEIGHTS)
def test_device_equals_the_host_build_bitwise_with_every_start_pattern(kind, pattern):
    case = seq_case(kind, pattern, 40, 65)
    assert_device_equals_host(case["x"], case["es"], real_nets(kind, case), (kind, pattern))


@pytest.mark.parametrize("L,B", ((1, BLOCK), (1, BLOCK + 1), (3, 43), (2, BLOCK * CHUNK // 2 + 1)))
def test_device_equals_the_host_build_bitwise_on_random_tensors(L, B):
    """A whole block, a block and one row, an odd row count, and R = BLOCK CHUNK + 2: a chunk edge
    and a short last block."""
    x, es, nets = random_case(L, B, 7 * L + B, quantised=False)
    assert (L, B) == (3, 43) or L * B in (BLOCK, BLOCK + 1, BLOCK * CHUNK + 2)
    assert_device_equals_host(x, es, nets, (L, B))


def test_autograd_on_the_device_within_4_d_ref():
    kind, pattern, L, B = "golden", "mid", 40, 65
    case = seq_case(kind, pattern, L, B)
    nets = [{k: v.to(DEV) for k, v in n.items()} for n in net_inputs(kind, case["states"])]
    x, es = T(case["x"]).to(DEV), T(case["es"]).to(DEV)
    d_h = d_h_for(case)
    w = [[n[k].clone().requires_grad_() for k in ACTOR] for n in nets]
    h = train.lstm_sequence_pair(x, es, (nets[0]["h0"], nets[0]["c0"], *w[0]), (nets[1]["h0"], nets[1]["c0"], *w[1]),
                                 weight_grads="kernel")
    ((h[0] * d_h[0].to(DEV)).sum() + (h[1] * d_h[1].to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    for k in range(2):
        r64, r32 = references(kind, pattern, L, B, k)
        for name, p, b, r in zip(GRAD_NAMES[1:], w[k], r32[1:], r64[1:]):
            err, d_ref = float((p.grad.cpu().double() - r).abs().max()), float((b - r).abs().max())
            print(f"net {k} {name}: device {err:.3e} reference {d_ref:.3e} ratio {err / d_ref:.2f}")
            assert p.grad.dtype == torch.float32 and err <= 4 * d_ref, (name, err, d_ref)
        assert torch.equal(w[k][2].grad, w[k][3].grad)


def minibatch_grads(m, buf, evaluate, loss_fn=ref.loss):
    """The gradient RecurrentPPO.train takes for the whole buffer as one minibatch, in m's dtype, as f64,
    BEFORE the gradient-norm clip; loss_fn: the restated loss for the reference side, train.ppo_loss for
    the module under test.  The clip multiplies all 21 tensors by one coefficient whose rounding
    error is that of the largest tensor (action_net): after it a small tensor's distance from the f64
    restatement is the norm's error, not the tensor's own (measured: 14 x d_ref on value_net.bias,
    which no kernel touches, with either weight_grads mode), so the tensors are compared as they
    leave backward()."""
    dt = m.log_std.dtype
    v, lp, ent = evaluate(m)
    loss, _ = loss_fn(v, lp, ent, buf.log_probs.to(dt), buf.advantages.to(dt), buf.returns.to(dt),
                      HYPER["clip_range"], HYPER["ent_coef"], HYPER["vf_coef"])
    m.zero_grad()
    loss.backward()
    return {k: p.grad.detach().to(torch.float64) for k, p in m.named_parameters()}


def test_one_minibatch_and_an_update_cycle_in_kernel_mode():
    pol, venv, col, buf = rollout()
    m = train.RecurrentPPOModule.from_policy(pol, weight_grads="kernel")
    assert m.weight_grads == "kernel"

    def loop(mod):
        return loop_evaluate(mod, buf.observations, buf.actions, buf.episode_starts, states0(buf))

    def loop_module_heads(mod):
        """The restatement up to the LSTMs' outputs, then the module's own heads."""
        x = ref.normalize(buf.observations, ref.constants(mod))
        s = states0(buf)
        h_pi = torch_lstm_loop(x, buf.episode_starts, s[0], s[1], *mod.lstm_actor.tensors())
        h_vf = torch_lstm_loop(x, buf.episode_starts, s[2], s[3], *mod.lstm_critic.tensors())
        return mod.heads(h_pi, h_vf, buf.actions)

    # The f64 side is the restatement throughout (tests/_ppo_reference.py: its heads and its loss).  The
    # f32 side, which only sizes the bound, keeps the module's heads over the all-torch LSTM loop: with
    # the restated heads there too, d_ref of mlp_extractor.policy_net.0.bias (64 elements, one draw of
    # f32 noise) came out at 9.5e-8 on an MI355X and this build's unchanged 3.95e-7 at 4.17 x d_ref.
    # What the heads compute is held by test_ppo_loss_cpu.py and the replay tests.
    g32 = minibatch_grads(copy.deepcopy(m), buf, loop_module_heads)
    g64 = minibatch_grads(copy.deepcopy(m).double(), buf, loop)
    got = minibatch_grads(m, buf, lambda mod: mod.evaluate_actions(buf.observations, buf.actions, buf.episode_starts,
                                                                   states0(buf)), train.ppo_loss)
    torch.cuda.synchronize()
    assert len(got) == 21
    for k, g in got.items():
        d_ref = float((g32[k] - g64[k]).abs().max())
        err = float((g - g64[k]).abs().max())
        print(f"{k}: kernel mode {err:.3e} reference {d_ref:.3e} ratio {err / d_ref:.2f}")
        assert float(g.abs().max()) > 0.0 and err <= 4 * d_ref, (k, err, d_ref)
    # collect -> ppo_update -> load_state_dict -> collect
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, eps=1e-5)
    gen = torch.Generator(device=DEV).manual_seed(3)
    stats = train.ppo_update(m, opt, buf, n_epochs=2, envs_per_batch=16, window=8, generator=gen, **HYPER)
    assert all(bool(torch.isfinite(v)) for v in stats.values())
    pol.load_state_dict(m.state_dict())
    buf2 = col.collect(16, states=True)
    torch.cuda.synchronize()
    assert torch.isfinite(buf2.values).all() and torch.isfinite(buf2.log_probs).all()
    venv.close()
    pol.close()


def test_the_default_is_unchanged():
    assert train.RecurrentPPOModule().weight_grads == "torch"
    kind, L, B = "golden", 40, 65
    case = seq_case(kind, "mid", L, B)
    nets = [{k: v.to(DEV) for k, v in n.items()} for n in net_inputs(kind, case["states"])]
    x, es = T(case["x"]).to(DEV), T(case["es"]).to(DEV)
    d_h = [d.to(DEV) for d in d_h_for(case)]
    # a default module's LSTM tensors through the call its evaluate_actions makes, through
    # lstm_sequence_pair with the keyword left out, and through _LstmSeq itself
    grads = []
    for call in (lambda m, a, c: train.lstm_sequence_pair(x, es, a, c, weight_grads=m.weight_grads),
                 lambda m, a, c: train.lstm_sequence_pair(x, es, a, c),
                 lambda m, a, c: train._LstmSeq.apply(False, "torch", x, es, *a, *c)):
        m = train.RecurrentPPOModule.from_policy(policy(kind), device=DEV)
        h = call(m, (nets[0]["h0"], nets[0]["c0"], *m.lstm_actor.tensors()),
                 (nets[1]["h0"], nets[1]["c0"], *m.lstm_critic.tensors()))
        ((h[0] * d_h[0]).sum() + (h[1] * d_h[1]).sum()).backward()
        grads.append([p.grad for p in (*m.lstm_actor.tensors(), *m.lstm_critic.tensors())])
    torch.cuda.synchronize()
    for other in grads[1:]:
        assert all(torch.equal(a, b) for a, b in zip(grads[0], other))
    # and they are train.weight_grads' sums, the function the parent commit shipped
    out = train.lstm_seq_forward(x, es, nets)
    bwd = [dict(w_hh=n["w_hh"], c0=n["c0"], c=o[1], gates=o[2], d_h=d) for n, o, d in zip(nets, out, d_h)]
    for k, dg in enumerate(train.lstm_seq_backward(es, bwd)):
        want = [g.to(torch.float32) for g in train.weight_grads(dg, x, out[k][0], nets[k]["h0"], es)]
        assert all(torch.equal(a, b) for a, b in zip(grads[0][4 * k:4 * k + 4], want))
