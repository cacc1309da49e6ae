"""train.ppo_loss, RecurrentPPOModule.heads and train.minibatch on the CPU (no GPU needed) against
tests/_ppo_reference.py: the loss, its six statistics and autograd's gradients with respect to
values, log_prob and entropy against a NumPy f64 restatement with closed-form gradients; the heads in
f64 against the explicit formulas; minibatch against a buffer whose every element says where it
stands.

Bound of the f64 comparisons: 4 N 2^-52 max |reference| per quantity, N the number of terms of the
longest sum (the rows of the minibatch; 128, the widest inner dimension, for the heads): each term
carries a few f64 roundings and the sum N more."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import _ppo_reference as ref  # noqa: E402
from cantorrl_amd import train  # noqa: E402
from cantorrl_amd.agent import STATE_NAMES  # noqa: E402
from cantorrl_amd.collect import RolloutBuffer  # noqa: E402

CLIP, ENT, VF = 0.3, 1e-5, 0.5
STATS = ("loss", "policy_gradient_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")
F64 = torch.float64


def bound(N, reference):
    return 4 * N * 2.0 ** -52 * float(np.abs(np.asarray(reference)).max())


def loss_inputs(N, ratios, adv, seed):
    rng = np.random.default_rng(seed)
    old = rng.normal(3.0, 1.0, N)
    return dict(values=rng.normal(0, 1, N), log_prob=old + np.log(ratios), entropy=rng.normal(-5.8, 0.1, N),
                old_log_prob=old, advantages=np.asarray(adv, np.float64), returns=rng.normal(0, 1, N))


def regions(stats):
    """The occupied ones of the six (sign of A) x (r below, inside, above the clip range)."""
    r, A = stats["ratio"], stats["adv"]
    where = np.where(r < 1 - CLIP, 0, np.where(r > 1 + CLIP, 2, 1))
    return {(bool(a >= 0), int(w)) for a, w in zip(A, where)}


def assert_loss_matches(x, normalize_advantage):
    N = x["values"].size
    want, want_grads = ref.loss_numpy(**x, clip_range=CLIP, ent_coef=ENT, vf_coef=VF,
                                      normalize_advantage=normalize_advantage)
    # the conditions under which the restatement's branches are the only right ones
    r, A = want["ratio"], want["adv"]
    assert np.minimum(np.abs(r - (1 - CLIP)), np.abs(r - (1 + CLIP))).min() > 1e-6
    assert np.abs(A).min() >= 1e-9
    t = {k: torch.from_numpy(v.copy()) for k, v in x.items()}
    for k in ("values", "log_prob", "entropy"):
        t[k].requires_grad_()
    loss, stats = train.ppo_loss(t["values"], t["log_prob"], t["entropy"], t["old_log_prob"], t["advantages"], t["returns"],
                                 CLIP, ENT, VF, normalize_advantage)
    assert set(stats) == set(STATS)
    grads = torch.autograd.grad(loss, [t["values"], t["log_prob"], t["entropy"]])
    assert abs(float(loss.detach()) - want["loss"]) <= bound(N, want["loss"])
    for k in STATS:
        d = abs(float(stats[k]) - want[k])
        print(f"N {N} normalize {normalize_advantage} {k}: {float(stats[k])!r} reference {want[k]!r} |d| {d:.2e}")
        assert d <= bound(N, want[k]), (k, float(stats[k]), want[k])
    for k, g in zip(("values", "log_prob", "entropy"), grads):
        d = float(np.abs(g.numpy() - want_grads[k]).max())
        print(f"N {N} normalize {normalize_advantage} dL/d{k}: |d| {d:.2e} of {np.abs(want_grads[k]).max():.2e}")
        assert d <= bound(N, want_grads[k]), k
    return want


@pytest.mark.parametrize("normalize_advantage", (True, False))
def test_ppo_loss_with_two_rows(normalize_advantage):
    """N = 2, the smallest N with an unbiased std (a biased one is off by sqrt 2).  Three pairs put a
    row into each of the six regions between them: A is (+, -) in every pair."""
    seen = set()
    for seed, ratios in enumerate(((1.5, 0.9), (0.5, 1.6), (1.1, 0.45))):
        want = assert_loss_matches(loss_inputs(2, np.array(ratios), (0.8, -0.3), seed), normalize_advantage)
        if normalize_advantage:   # (x - mean) / std of two values: +-1 / sqrt 2
            assert np.allclose(np.abs(want["adv"]), 1 / np.sqrt(2), rtol=1e-6, atol=0)
        seen |= regions(want)
    assert len(seen) == 6, seen


@pytest.mark.parametrize("normalize_advantage", (True, False))
def test_ppo_loss_with_all_six_regions_in_one_minibatch(normalize_advantage):
    N = 64
    rng = np.random.default_rng(11)
    kind = np.arange(N) % 3                      # r below, inside, above the clip range
    ratios = np.where(kind == 0, rng.uniform(0.4, 0.65, N), np.where(kind == 1, rng.uniform(0.75, 1.25, N),
                                                                     rng.uniform(1.4, 1.8, N)))
    sign = np.where((np.arange(N) // 3) % 2 == 0, 1.0, -1.0)
    adv = sign * rng.uniform(0.2, 2.0, N) + 0.05   # a mean to subtract
    want = assert_loss_matches(loss_inputs(N, ratios, adv, 5), normalize_advantage)
    assert len(regions(want)) == 6
    assert 0.5 < want["clip_fraction"] < 0.8 and want["approx_kl"] > 0.01
    # both branches of the min carry gradient, and some rows none
    active = ref.loss_numpy(**loss_inputs(N, ratios, adv, 5), clip_range=CLIP, ent_coef=ENT, vf_coef=VF,
                            normalize_advantage=normalize_advantage)[1]["log_prob"] != 0
    assert 0 < active.sum() < N


def test_a_ratio_on_the_clip_edge_is_not_counted_as_clipped():
    """sb3_contrib counts |r - 1| > clip_range, strictly.  The clip range is taken from the ratio itself,
    so that one row stands exactly on the edge; the other is far inside."""
    x = loss_inputs(2, np.array((1.25, 1.01)), (0.8, -0.3), 3)
    t = {k: torch.from_numpy(v.copy()) for k, v in x.items()}
    r = float(torch.exp(t["log_prob"] - t["old_log_prob"])[0])   # the op and the shape ppo_loss uses
    c = r - 1.0
    assert abs(r - 1.0) == c and 0.2 < c < 0.3
    _, stats = train.ppo_loss(t["values"], t["log_prob"], t["entropy"], t["old_log_prob"], t["advantages"], t["returns"],
                              c, ENT, VF)
    assert float(stats["clip_fraction"]) == 0.0
    _, stats = train.ppo_loss(t["values"], t["log_prob"], t["entropy"], t["old_log_prob"], t["advantages"], t["returns"],
                              np.nextafter(c, 0.0), ENT, VF)
    assert float(stats["clip_fraction"]) == 0.5


# --------------------------------------------------------------------------- the heads
def random_module(activation, seed):
    m = train.RecurrentPPOModule(activation=activation).double()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_((torch.rand(p.shape, generator=g, dtype=F64) - 0.5) * 0.4)
    return m, g


@pytest.mark.parametrize("activation", ("tanh", "relu"))
def test_heads_in_f64_match_the_closed_forms(activation):
    L, B, N = 3, 5, 128
    m, g = random_module(activation, 3)
    h_pi, h_vf = (torch.rand((L, B, N), generator=g, dtype=F64) * 2 - 1 for _ in range(2))
    actions = torch.randn((L, B, 2), generator=g, dtype=F64)
    params = dict(m.named_parameters())
    assert len(params) == 21
    got = m.heads(h_pi, h_vf, actions)
    with torch.no_grad():
        want = ref.heads(params, h_pi, h_vf, actions, activation)
    out = [t.detach() for t in got]
    for name, a, b in zip(("values", "log_prob", "entropy"), out, want):
        d = float((a - b).abs().max())
        print(f"{activation} {name}: |d| {d:.2e} of {float(b.abs().max()):.2e}")
        assert tuple(a.shape) == (L, B), name
        assert d <= bound(N, b.numpy()), name
    # the closed forms once more in NumPy, away from torch: sum_j (0.5 + 0.5 ln 2 pi + log_std_j) in every row
    log_std = m.log_std.detach().numpy()
    ent = float((0.5 + 0.5 * np.log(2 * np.pi) + log_std).sum())
    assert float((out[2] - ent).abs().max()) <= bound(N, ent)
    assert float(out[2].max() - out[2].min()) == 0.0
    assert float(out[0].std()) > 1e-3 and float(out[1].std()) > 1e-2   # rows differ where they should
    if activation == "relu":   # the two activations are two functions: some hidden unit is cut off
        pre = h_pi @ params["mlp_extractor.policy_net.0.weight"].t() + params["mlp_extractor.policy_net.0.bias"]
        assert bool((pre < 0).any()) and bool((pre > 0).any())
    # d mean(entropy) / d log_std_j = 1, and no other tensor is touched
    grads = torch.autograd.grad(got[2].mean(), list(params.values()), allow_unused=True)
    for k, gr in zip(params, grads):
        if k == "log_std":
            assert float((gr - 1.0).abs().max()) <= bound(N, 1.0)
        else:
            assert gr is None or float(gr.abs().max()) == 0.0, k


# --------------------------------------------------------------------------- minibatch
FIELDS = {"observations": 1, "actions": 2, "log_probs": 3, "advantages": 4, "returns": 5, "states": 6,
          "h_pi": 7, "c_pi": 8, "h_vf": 9, "c_vf": 10}


def code(field, k, e, j):
    """The value at step k, env e, trailing index j of a field: an integer below 2^24."""
    return FIELDS[field] * 10 ** 6 + k * 10 ** 5 + e * 10 ** 4 + j


def coded_buffer(K, n):
    buf = RolloutBuffer(K, n, "cpu", states=True)
    ks, es = np.arange(K)[:, None, None], np.arange(n)[None, :, None]
    for name in ("observations", "actions", "log_probs", "advantages", "returns", "states"):
        t = getattr(buf, name)
        tail = int(np.prod(t.shape[2:], dtype=np.int64))
        t.copy_(torch.from_numpy(code(name, ks, es, np.arange(tail)[None, None]).astype(np.float32)).reshape(t.shape))
    for name in STATE_NAMES:
        getattr(buf, name).copy_(torch.from_numpy(code(name, 0, np.arange(n)[:, None], np.arange(128)[None]).astype(np.float32)))
    buf.episode_starts.copy_(torch.from_numpy((100 + np.arange(K)[:, None] * n + np.arange(n)[None]).astype(np.uint8)))
    for name in ("rewards", "values"):   # not part of a minibatch
        getattr(buf, name).fill_(-1.0)
    return buf


@pytest.mark.parametrize("k0,k1", ((0, 6), (0, 3), (3, 6), (5, 6)))
def test_minibatch_takes_the_window_and_the_envs_it_is_asked_for(k0, k1):
    K, n = 6, 5
    buf = coded_buffer(K, n)
    assert code("c_vf", 0, n - 1, 127) < 2 ** 24
    idx = torch.tensor([3, 0, 4])   # a shuffled subset
    mb = train.minibatch(buf, idx, k0, k1)
    assert set(mb) == {"observations", "actions", "episode_starts", "log_probs", "advantages", "returns", "states0"}
    ks, es = np.arange(k0, k1)[:, None, None], idx.numpy()[None, :, None]
    for name, tail in (("observations", 13), ("actions", 2), ("log_probs", 1), ("advantages", 1), ("returns", 1)):
        want = code(name, ks, es, np.arange(tail)[None, None]).astype(np.float32)
        want = want if tail > 1 else want[..., 0]
        assert mb[name].dtype == torch.float32 and mb[name].is_contiguous(), name
        assert np.array_equal(mb[name].numpy(), want), name
    want = (100 + np.arange(k0, k1)[:, None] * n + idx.numpy()[None]).astype(np.uint8)
    assert mb["episode_starts"].dtype == torch.uint8 and mb["episode_starts"].is_contiguous()
    assert np.array_equal(mb["episode_starts"].numpy(), want)
    assert len(mb["states0"]) == 4
    for i, (name, s) in enumerate(zip(STATE_NAMES, mb["states0"])):
        if k0 == 0:
            want = code(name, 0, idx.numpy()[:, None], np.arange(128)[None])
        else:
            want = code("states", k0, idx.numpy()[:, None], i * 128 + np.arange(128)[None])
        assert tuple(s.shape) == (3, 128) and s.is_contiguous(), name
        assert np.array_equal(s.numpy(), want.astype(np.float32)), (name, k0)
