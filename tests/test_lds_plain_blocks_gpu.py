"""The plain blocks of lds_rollout_kernel: a full 8-step block in which no lane of a wave meets an
episode boundary runs a second instance of each role's block body with the episode handling
compiled out.  Both bodies must give the tile kernels' rollouts bit for bit -- obs, rewards, done
flags and the checkpointed state after every call -- at the episode lengths around the first one
that has a plain block (T = 10), with launches that start mid-episode and at odd steps, ragged
last blocks, a partial last workgroup, envs reset apart (one wave holding lanes at different
episode steps), the persistent grid and the policy rollout."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

M = 8   # the LDS market block, kLdsM
KS = (5, 64, 13, 71, 256)
N = 130   # two full workgroups and one whose lanes past N mirror env N - 1


def _plain_pattern(T, ks, t0=0):
    """(stepper, producer) plain flags of every full block of launches ks for an env at episode
    step t0 -- the kernels' own tests: e.t + M < T, and 1 <= tpb and tpb + M < T."""
    out, t = [], t0
    for k in ks:
        for b in range(k // M):
            tb = (t + b * M) % T
            out.append((tb + M < T, 1 <= tb and tb + M < T))
        t = (t + k) % T
    return out


def _rollouts(n, gen, kw, ks, monkeypatch, desync=False, grid=None):
    from cantorrl_amd.vec_env import HedgingVecEnv
    g = torch.Generator(device="cuda")
    g.manual_seed(17)
    acts = torch.rand((sum(ks), n, 2), device="cuda", generator=g) * 2.2 - 1.1
    runs = []
    for lds in ("1", "0"):
        monkeypatch.setenv("HE_LDS_ROLLOUT", lds)
        if grid:
            monkeypatch.setenv("HE_LDS_MAX_GRID", str(grid))
        env = HedgingVecEnv(n, mode="gbm", generate=gen, seed=31, global_env_offset=5, return_numpy=False,
                            info_keys=(), **kw)
        got = [env.reset_tensors().clone()]
        a0 = 0
        for j, k in enumerate(ks):
            o, r, t = env.rollout(acts[a0:a0 + k].contiguous())
            got += [o.clone(), r.clone(), t.clone(), torch.from_numpy(env.get_state().copy())]
            a0 += k
            if desync and j == 0:   # every third env starts a new episode: lanes at different steps
                got.append(env.reset_tensors(env_ids=list(range(0, n, 3))).clone())
        env.close()
        runs.append(got)
    assert len(runs[0]) == len(runs[1])
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), i
    return runs[0]


@pytest.mark.parametrize("T", [1, 7, 8, 9, 10, 11, 17, 252])
def test_plain_blocks_equal_tile_rollout(T, monkeypatch):
    """T = 9 has no plain block, T = 10 one producer block (tpb = 1); T = 8 and 9 wrap the episode
    step at k = T and k = T - 1; from T = 10 plain and boundary blocks alternate within a launch."""
    pat = _plain_pattern(T, KS)
    assert any(p for _, p in pat) == (T >= 10) and any(s for s, _ in pat) == (T >= 9)
    if T >= 10:
        assert not all(s for s, _ in pat) and not all(p for _, p in pat)
    got = _rollouts(N, dict(episode_length=T), {}, KS, monkeypatch)
    term = torch.cat(got[3::4])   # [reset obs, (obs, reward, terminated, state) per call]
    assert term.shape == (sum(KS), N)
    want = (torch.arange(1, sum(KS) + 1) % T == 0).to(term.device)
    assert torch.equal(term.bool(), want[:, None].expand(-1, N))


def test_plain_blocks_train_settings(monkeypatch):
    """The training configuration (costs, slippage, time penalty) at the reference's episode
    length, two launches of the headline's K: 244 of every 252 blocks are plain."""
    from test_gpu_parity import LDS_CASES
    _, _, kw, _ = LDS_CASES["train"]
    pat = _plain_pattern(252, (256, 256))
    assert sum(s for s, _ in pat) >= 60 and not all(s for s, _ in pat)
    _rollouts(N, dict(episode_length=252), kw, (256, 256), monkeypatch)


@pytest.mark.parametrize("T", [17, 40])
def test_plain_blocks_desynchronised_envs(T, monkeypatch):
    """Every third env reset after the first call: a wave holds lanes at two episode steps, so some
    blocks are plain for some of its lanes only (the general body), others for all (the plain one)."""
    ks = KS[1:]
    a = _plain_pattern(T, ks, t0=KS[0] % T)   # the envs left alone
    b = _plain_pattern(T, ks, t0=0)           # the envs reset after the first call
    for role in (0, 1):
        assert any(x[role] != y[role] for x, y in zip(a, b))
        assert any(x[role] and y[role] for x, y in zip(a, b))
    _rollouts(N, dict(episode_length=T), {}, KS, monkeypatch, desync=True)


def test_plain_blocks_persistent_grid(monkeypatch):
    """The persistent instance (8 tiles on 5 workgroups, the last tile 2 envs wide), envs reset apart."""
    _rollouts(450, dict(episode_length=17), {}, KS, monkeypatch, desync=True, grid=5)


def test_plain_blocks_policy_rollout(monkeypatch):
    """he_rollout_policy (delta_every_step) at T = 17, LDS against tile: the policy instances share
    the steppers' code and the producers' plain blocks."""
    from cantorrl_amd.vec_env import HedgingVecEnv
    n, T = N, 17
    envs = []
    for lds in (True, False):
        if not lds:
            monkeypatch.setenv("HE_LDS_POLICY", "0")
        envs.append(HedgingVecEnv(n, mode="gbm", generate=dict(episode_length=T), seed=31, return_numpy=False,
                                  info_keys=()))
        monkeypatch.delenv("HE_LDS_POLICY", raising=False)
    recs = [(torch.zeros((64 * n, 80), dtype=torch.uint8, device="cuda"),
             torch.zeros(1, dtype=torch.int64, device="cuda")) for _ in envs]
    for e in envs:
        e.reset_tensors()
    for K in KS:
        outs = []
        for e, (rec, cnt) in zip(envs, recs):
            a = torch.empty((K, n, 2), device="cuda")
            o = torch.empty((K, n, 13), device="cuda")
            r = torch.empty((K, n), device="cuda")
            t = torch.empty((K, n), dtype=torch.uint8, device="cuda")
            e.rollout_policy(K, "delta_every_step", a, o, r, t, rec, cnt)
            torch.cuda.synchronize()
            outs.append((a, o, r, t, torch.from_numpy(e.get_state().copy())))
        for x, y in zip(*outs):
            assert torch.equal(x, y), K
    assert int(recs[0][1].item()) == int(recs[1][1].item()) == n * (sum(KS) // T)
    for e in envs:
        e.close()
