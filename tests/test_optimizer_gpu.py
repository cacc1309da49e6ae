"""ha_adam_step on the GPU (opt_norm_kernel, opt_adam_kernel) against the host build of the same
arithmetic bit for bit, on the cases of test_optimizer_cpu.py, and against the f64 restatement within
4 x the error of torch's own clip_grad_norm_ + torch.optim.Adam on the GPU."""
import ctypes

import numpy as np
import pytest

from test_optimizer_cpu import (CLIPS, HYPER, Hyper, Tensor, bits, copy_state, five_steps_against_f64, host_step,
                                make_state, new_grads, shapes_of, torch_adam_steps)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from cantorrl_amd import agent, train  # noqa: E402

DEV = "cuda:0"
KEYS = ("param", "grad", "exp_avg", "exp_avg_sq")


def to_dev(state):
    return [{k: torch.from_numpy(T[k].copy()).to(DEV) for k in KEYS} for T in state]


def device_step(dstate, t, max_grad_norm, **hyper):
    """ha_adam_step over the device tensors of `dstate`, in place -> (status, grad_norm tensor)."""
    lib = agent.load()
    arr = (Tensor * len(dstate))()
    for a, T in zip(arr, dstate):
        for k in KEYS:
            setattr(a, k, T[k].data_ptr())
        a.numel = T["param"].numel()
    size = lib.ha_adam_workspace_bytes(len(dstate), arr)
    assert size == 8 * sum(-(-T["param"].numel() // 256) for T in dstate)
    ws = torch.full((size,), 0xFF, dtype=torch.uint8, device=DEV)   # garbage: the workspace carries nothing
    norm = torch.full((), float("nan"), device=DEV)
    h = dict(HYPER, **hyper)
    hy = Hyper(h["lr"], h["beta1"], h["beta2"], h["eps"], max_grad_norm, t, norm.data_ptr())
    st = lib.ha_adam_step(len(dstate), arr, ctypes.byref(hy), ws.data_ptr(), train._stream(torch.device(DEV)))
    return st, norm


def assert_device_equals_host(dstate, hstate, what):
    torch.cuda.synchronize()
    for j, (D, H) in enumerate(zip(dstate, hstate)):
        for k in KEYS:   # grad among them: neither build writes it
            assert np.array_equal(bits(D[k].cpu().numpy()), bits(H[k])), (what, j, k)


@pytest.mark.parametrize("clip", sorted(CLIPS))
@pytest.mark.parametrize("kind", ["sizes", "module"])
def test_device_equals_host_build_bitwise_over_five_steps(kind, clip):
    mgn = CLIPS[clip]
    host = make_state(shapes_of(kind), seed=11)
    dev = to_dev(host)
    for t in range(1, 6):
        new_grads(host, 100 + t)
        for D, H in zip(dev, host):
            D["grad"] = torch.from_numpy(H["grad"].copy()).to(DEV)
        hst, hnorm = host_step(host, t, mgn)
        dst, dnorm = device_step(dev, t, mgn)
        assert hst == 0 and dst == 0
        assert_device_equals_host(dev, host, (kind, clip, t))
        assert bits(dnorm.cpu().numpy()) == bits(hnorm), (t, float(dnorm), hnorm)
    assert all(np.abs(H["exp_avg"]).max() > 0 for H in host)


def test_zero_gradient_and_regrouped_tensors_equal_the_host_build_bitwise():
    host = make_state(shapes_of("sizes"), seed=3)
    for T in host:
        T["grad"][...] = 0.0
    dev = to_dev(host)
    assert host_step(host, 1, 0.5)[0] == 0
    st, norm = device_step(dev, 1, 0.5)
    assert st == 0
    assert_device_equals_host(dev, host, "zero gradient")
    assert float(norm) == 0.0
    # one list in two calls without a clip; a tensor cut at a block boundary with one
    one = make_state(shapes_of("sizes"), seed=5)
    d_one, d_two = to_dev(one), to_dev(one)
    assert host_step(one, 3, 0.0)[0] == 0
    assert device_step(d_one, 3, 0.0)[0] == 0
    assert device_step(d_two[:2], 3, 0.0)[0] == 0 and device_step(d_two[2:], 3, 0.0)[0] == 0
    assert_device_equals_host(d_one, one, "one call")
    assert_device_equals_host(d_two, one, "two calls")
    whole = make_state([(1027,)], seed=6, grad_scale=1.0)
    cut = [{k: v[sl].copy() for k, v in whole[0].items()} for sl in (slice(0, 512), slice(512, 1027))]
    d_cut = to_dev(cut)
    hst, hnorm = host_step(whole, 2, 0.5)
    dst, dnorm = device_step(d_cut, 2, 0.5)
    assert hst == 0 and dst == 0 and hnorm > 1.0
    glued = [{k: np.concatenate([d_cut[0][k].cpu().numpy(), d_cut[1][k].cpu().numpy()]) for k in KEYS}]
    assert_device_equals_host([{k: torch.from_numpy(v) for k, v in glued[0].items()}], whole, "cut at a block boundary")
    assert bits(dnorm.cpu().numpy()) == bits(hnorm)


def device_adam_steps(state, grads, mgn):
    ps = [torch.nn.Parameter(torch.from_numpy(T["param"].copy()).to(DEV)) for T in state]
    opt = train.DeviceAdam(ps, lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"])
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy()).to(DEV)
        norm = opt.clip_and_step(mgn)
        assert norm.device.type == "cuda" and norm.dim() == 0
    return [p.detach().cpu().numpy() for p in ps]


@pytest.mark.parametrize("kind", ["sizes", "module"])
def test_device_adam_stays_within_4_d_ref_of_the_f64_restatement(kind):
    res = five_steps_against_f64(device_adam_steps, lambda s, g, m: torch_adam_steps(s, g, m, device=DEV),
                                 shapes_of(kind))
    for j, (err, d_ref, ulp) in enumerate(res):
        print(f"tensor {j}: DeviceAdam {err:.3e} torch {d_ref:.3e} ulp {ulp:.3e}")
        assert err <= 4 * d_ref + ulp, (j, err, d_ref, ulp)
    assert max(d for _, d, _ in res) > 0.0


def test_device_adam_refuses_a_missing_and_a_strided_gradient():
    ps = [torch.nn.Parameter(torch.zeros(5, device=DEV)), torch.nn.Parameter(torch.zeros(3, device=DEV))]
    opt = train.DeviceAdam(ps)
    ps[0].grad = torch.ones(5, device=DEV)
    with pytest.raises(ValueError, match="no gradient"):
        opt.step()
    ps[1].grad = torch.ones(6, device=DEV)[::2]
    assert not ps[1].grad.is_contiguous()
    with pytest.raises(ValueError, match="contiguous float32"):
        opt.step()
    torch.cuda.synchronize()
    assert not ps[0].any() and not opt.state[ps[0]]["exp_avg"].any()   # nothing ran
