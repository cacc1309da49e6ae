"""RolloutCollector: sb3_contrib RecurrentPPO.collect_rollouts on the device.

    policy = RecurrentPolicy.from_sb3_zip("final_model.zip")
    col = RolloutCollector(DeviceVecNormalize(venv), policy, gamma=0.98242, gae_lambda=0.91788, seed=7)
    buf = col.collect(256)          # device tensors, [K, N, ...] = SB3's (buffer_size, n_envs, ...)
    ... the PPO update, in torch ...
    policy.load_state_dict(new_state_dict)
    buf = col.collect(256, buffer=buf)

Per step: the obs and episode_start go into the buffer, one ha_policy_step writes the action, value
and log-probability straight into the buffer's [k] slices, the env is stepped with the clipped action,
the reward is stored and `terminated` becomes the next episode_start.  After the K steps one
ha_policy_step with write_state=False on the final obs gives last_values (SB3's predict_values), and
ha_gae the advantages and returns.  Everything is enqueued on the current stream; nothing
synchronises with the host.
"""
import torch

from .agent import ACT_DIM, HIDDEN, OBS_DIM, STATE_NAMES


class RolloutBuffer:
    """The device tensors of one rollout (attributes): observations [K,N,13], actions [K,N,2],
    rewards, values, log_probs, advantages, returns [K,N] f32, episode_starts [K,N] u8, last_values
    [N] f32, last_dones [N] u8, the LSTM states as they stood before step 0 (h_pi, c_pi, h_vf, c_vf
    [N,128]) and, where asked for, `states` [K,N,4,128]: the states fed to every step."""

    def __init__(self, k_steps, n_envs, device, states=False):
        K, n = int(k_steps), int(n_envs)
        f = dict(dtype=torch.float32, device=device)
        self.k_steps, self.n_envs = K, n
        self.observations = torch.empty((K, n, OBS_DIM), **f)
        self.actions = torch.empty((K, n, ACT_DIM), **f)
        for name in ("rewards", "values", "log_probs", "advantages", "returns"):
            setattr(self, name, torch.empty((K, n), **f))
        self.episode_starts = torch.empty((K, n), dtype=torch.uint8, device=device)
        self.last_values = torch.empty(n, **f)
        self.last_dones = torch.empty(n, dtype=torch.uint8, device=device)
        for name in STATE_NAMES:
            setattr(self, name, torch.empty((n, HIDDEN), **f))
        self.states = torch.empty((K, n, 4, HIDDEN), **f) if states else None


class RolloutCollector:
    """env: a HedgingVecEnv(return_numpy=False) or a DeviceVecNormalize over one (reset_tensors,
    step_tensors).  policy: an agent.RecurrentPolicy on the env's device.  seed: the action noise's
    Philox key, distinct from the env's seed.  env_id_offset: the global id of env 0 (a rank's
    offset), so that the noise does not depend on how the envs are split over ranks."""

    def __init__(self, env, policy, gamma, gae_lambda, seed, env_id_offset=0):
        self.env, self.policy = env, policy
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.seed = int(seed)
        self.env_id_offset = int(env_id_offset)
        self.num_envs = int(env.num_envs)
        self.step_index = 0      # continues across collect() calls
        self._obs = None         # the env's obs tensor (its own fixed buffer)
        self._start = None
        self._env_act = None
        self._scratch = None

    def reset(self):
        """Reset the env and the LSTM states: every env begins an episode."""
        n = self.num_envs
        self._obs = self.env.reset_tensors()
        dev = self._obs.device
        self.policy.reset_states(n)
        self._start = torch.ones(n, dtype=torch.uint8, device=dev)
        self._env_act = torch.empty((n, ACT_DIM), dtype=torch.float32, device=dev)
        self._scratch = {k: torch.empty((n,) + tail, dtype=torch.float32, device=dev)
                         for k, tail in (("actions", (ACT_DIM,)), ("env_actions", (ACT_DIM,)), ("log_probs", ()))}

    def collect(self, k_steps, buffer=None, states=False):
        """k_steps env steps of every env -> a RolloutBuffer (`buffer` is refilled when given).  The
        first call resets the env; later calls go on from where the last one stopped."""
        K, n = int(k_steps), self.num_envs
        if K < 1:
            raise ValueError("k_steps must be >= 1")
        if self._obs is None:
            self.reset()
        pol = self.policy
        if buffer is None:
            buffer = RolloutBuffer(K, n, self._obs.device, states=states)
        elif buffer.k_steps != K or buffer.n_envs != n or (states and buffer.states is None):
            raise ValueError(f"buffer is not a RolloutBuffer of {K} steps x {n} envs" + (" with states" if states else ""))
        b = buffer
        for name, t in zip(STATE_NAMES, pol.states):
            getattr(b, name).copy_(t)
        obs, start = self._obs, self._start
        out = dict(env_actions=self._env_act)
        for k in range(K):
            b.observations[k].copy_(obs)
            b.episode_starts[k].copy_(start)
            if b.states is not None:
                for i, t in enumerate(pol.states):
                    b.states[k, :, i].copy_(t)
            out.update(actions=b.actions[k], values=b.values[k], log_probs=b.log_probs[k])
            pol.step(b.observations[k], b.episode_starts[k], self.seed, self.step_index,
                     env_id_offset=self.env_id_offset, out=out)
            self.step_index += 1
            obs, rew, term, _ = self.env.step_tensors(self._env_act, info=False)
            b.rewards[k].copy_(rew)
            start.copy_(term)
        self._obs = obs
        # SB3: values = policy.predict_values(last obs, lstm_states, dones) -- no state is kept
        b.last_dones.copy_(start)
        pol.step(obs, start, self.seed, self.step_index, deterministic=True, write_state=False,
                 env_id_offset=self.env_id_offset, out=dict(self._scratch, values=b.last_values))
        pol.gae(b.rewards, b.values, b.episode_starts, b.last_values, b.last_dones, self.gamma, self.gae_lambda,
                advantages=b.advantages, returns=b.returns)
        return b
