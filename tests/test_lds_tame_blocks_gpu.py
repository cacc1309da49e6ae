"""The tame blocks of lds_rollout_kernel: in a plain 8-step block whose market the producers
flagged tame -- every price in [64, 2^23], every mark positive and finite -- the GBM obs stepper
runs a third instance of its slots with the corner-case guards compiled out.  All three bodies must
give the tile kernels' rollouts bit for bit: obs, rewards, done flags and the checkpointed state
after every call, for markets that are always tame, never tame, tame for some blocks or some lanes
only (prices crossing 64 or 2^23 both ways), for a handle whose constants rule the body out, for
envs reset apart and for the persistent grid (an instance without the tame body).

The tame pattern is worked out here from the tile path's own outputs (S = obs[:, 0] max(S0, 25),
per 64-env tile and 8-step block) and every case asserts what it is meant to exercise."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

M = 8   # the LDS market block, kLdsM
W = 64  # envs per workgroup
KS = (5, 64, 13, 71, 256)
N = 130   # two full workgroups and one whose lanes past N mirror env N - 1
S0_DEFAULT = 496.48001098632812
LO, HI = 64.0, 8388608.0


def _train_kw():
    from test_gpu_parity import LDS_CASES
    return LDS_CASES["train"][2]


def _rollouts(n, gen, kw, ks, monkeypatch, desync=False, grid=None):
    """Both paths' outputs compared with torch.equal; returns the tile path's calls
    [(obs, reward, terminated)], the reset obs and the ids reset after the first call."""
    from cantorrl_amd.vec_env import HedgingVecEnv
    g = torch.Generator(device="cuda")
    g.manual_seed(17)
    acts = torch.rand((sum(ks), n, 2), device="cuda", generator=g) * 2.2 - 1.1
    ids = list(range(0, n, 3)) if desync else []
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
                got.append(env.reset_tensors(env_ids=ids).clone())
        env.close()
        runs.append(got)
    assert len(runs[0]) == len(runs[1])
    for i, (a, b) in enumerate(zip(*runs)):
        assert torch.equal(a, b), i
    tile = [x for x in runs[1] if x.dim() != 1 or x.dtype != torch.uint8]   # without the state blobs
    if desync:
        tile = tile[:4] + tile[5:]
    calls = [tuple(tile[1 + 3 * j:4 + 3 * j]) for j in range(len(ks))]
    return calls, tile[0], ids


def _pattern(calls, reset_obs, ids, s0, n):
    """Per full block and 64-env tile of every call, from the tile path's outputs: 'general' (some
    lane ends an episode in the block), else 'tame' (every lane's 8 prices and the one before them
    in [64, 2^23], marks positive and finite), 'partial' (some lanes only) or 'wild' (none)."""
    scale = max(s0, 25.0)
    prev = (reset_obs[:, 0].double() * scale).cpu()
    s_reset = prev.clone()
    out = []
    for j, (o, _, t) in enumerate(calls):
        S = (o[:, :, 0].double() * scale).cpu()
        ok = ((S >= LO) & (S <= HI) & (o[:, :, 1] > 0).cpu() & (o[:, :, 2] > 0).cpu()
              & torch.isfinite(o[:, :, 1:3]).all(-1).cpu())
        term = t.bool().cpu()
        before = torch.cat([prev[None], S[:-1]])   # the lagged price of every step
        ok &= (before >= LO) & (before <= HI)
        for b in range(o.shape[0] // M):
            sl = slice(b * M, b * M + M)
            for w in range(0, n, W):
                if term[sl, w:w + W].any():
                    out.append("general")
                    continue
                lanes = ok[sl, w:w + W].all(0)
                out.append("tame" if lanes.all() else ("partial" if lanes.any() else "wild"))
        prev = S[-1].clone()
        if j == 0 and ids:
            prev[ids] = s_reset[ids]
    return out


def test_tame_headline_market(monkeypatch):
    """The benchmark's market with the training settings at T = 252: every plain block is tame."""
    gen = dict(s0=S0_DEFAULT, episode_length=252)
    calls, ro, ids = _rollouts(N, gen, _train_kw(), KS, monkeypatch)
    pat = _pattern(calls, ro, ids, gen["s0"], N)
    assert pat.count("tame") >= 100 and "general" in pat
    assert "partial" not in pat and "wild" not in pat


@pytest.mark.parametrize("T", [17, 252])
@pytest.mark.parametrize("s0", [64.2, 70.0])
def test_tame_lower_threshold_crossed(s0, T, monkeypatch):
    """Prices around 64 at sigma = 71 % a year: blocks tame for every lane, for some, for none."""
    gen = dict(s0=s0, variance=0.5, episode_length=T)
    calls, ro, ids = _rollouts(N, gen, {}, KS, monkeypatch)
    pat = _pattern(calls, ro, ids, s0, N)
    print(s0, T, {k: pat.count(k) for k in ("general", "tame", "partial", "wild")})
    assert "tame" in pat and "partial" in pat


def test_tame_upper_threshold_crossed(monkeypatch):
    """S0 = 8.0e6 under 2^23 = 8,388,608: prices cross the upper bound."""
    gen = dict(s0=8.0e6, variance=0.5, episode_length=252)
    calls, ro, ids = _rollouts(N, gen, {}, KS, monkeypatch)
    pat = _pattern(calls, ro, ids, gen["s0"], N)
    print({k: pat.count(k) for k in ("general", "tame", "partial", "wild")})
    S = torch.cat([o[:, :, 0] for o, _, _ in calls]).double() * 8.0e6
    assert (S > HI).any() and (S < HI).any() and (S >= LO).all()
    # blocks with lanes on both sides of the bound, and blocks with every lane past it
    assert "partial" in pat and "wild" in pat


@pytest.mark.parametrize("s0", [30.0, 0.8])
def test_never_tame(s0, monkeypatch):
    """Prices under 64 throughout: the plain body only."""
    gen = dict(s0=s0, episode_length=252)
    calls, ro, ids = _rollouts(N, gen, _train_kw(), KS, monkeypatch)
    pat = _pattern(calls, ro, ids, s0, N)
    assert "wild" in pat and "tame" not in pat and "partial" not in pat


def test_tame_ruled_out_by_the_handle(monkeypatch):
    """Variance 1e-8: the lean kernel still runs, but |d1| is far past 14 (sigma sqrt(tenor) is
    about 3e-5 against |log(S / K)| up to 1e-3) and the out-of-the-money mark is 0 in f32, so the
    host's bound keeps the tame body off although every price is in range."""
    gen = dict(s0=S0_DEFAULT, variance=1e-8, episode_length=252)
    calls, ro, ids = _rollouts(N, gen, {}, KS, monkeypatch)
    marks = torch.cat([o[:, :, 1:3] for o, _, _ in calls])
    S = torch.cat([o[:, :, 0] for o, _, _ in calls]).double() * S0_DEFAULT
    assert (marks == 0).any() and (S >= LO).all() and (S <= HI).all()
    g = torch.cat([o[:, :, 7] for o, _, _ in calls])   # call delta: N(d1) saturated both ways
    assert (g == 0).any() or (g == 1).any()


@pytest.mark.parametrize("s0", [S0_DEFAULT, 64.2])
def test_tame_desynchronised_envs(s0, monkeypatch):
    """Every third env reset after the first call: lanes at different episode steps, so a tile's
    blocks are plain for some of its lanes only while the market is tame."""
    gen = dict(s0=s0, variance=0.5 if s0 < 100 else 0.029028, episode_length=40)
    calls, ro, ids = _rollouts(N, gen, {}, KS, monkeypatch, desync=True)
    pat = _pattern(calls, ro, ids, s0, N)
    assert "general" in pat and "tame" in pat


def test_tame_persistent_grid(monkeypatch):
    """The persistent instance (8 tiles on 5 workgroups, the last tile 2 envs wide) has no tame body:
    it stays equal on a market that is tame throughout."""
    gen = dict(s0=S0_DEFAULT, episode_length=40)
    calls, ro, ids = _rollouts(450, gen, {}, KS, monkeypatch, desync=True, grid=5)
    pat = _pattern(calls, ro, ids, gen["s0"], 450)
    assert "tame" in pat and "wild" not in pat and "partial" not in pat
