"""RecurrentActor: the actor of an SB3 RecurrentPPO checkpoint on the device (libhedgeactor,
include/hedge_actor.h): obs 13 -> LSTM 128 -> Linear 64 -> Linear 64 -> Linear 2, one HIP kernel
per step for every env, the recurrent state resident on the device.

    actor = RecurrentActor.from_sb3_zip("final_model.zip", normalization="normalization_stats.pkl")
    records = venv.evaluate_actor(actor, num_episodes=1000)      # vec_env.HedgingVecEnv

RecurrentPolicy is the training-side counterpart: actor and critic (its own LSTM 128 -> 64 -> 64
-> 1), the sampled action, the value and the log-probability of a rollout step in one launch, and
GAE; collect.RolloutCollector fills a rollout buffer with it.

    policy = RecurrentPolicy.from_sb3_zip("final_model.zip")

The arithmetic contract is in the header; `host_step` runs the same code compiled for the host
(no GPU needed).  There is no torch fallback: a missing library is an error.
"""
import ctypes
import io
import os
import pickle
import zipfile

import numpy as np

from . import _bind, _lib

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libhedgeactor.so")
HA_ABI_VERSION = 1
OBS_DIM, HIDDEN, MLP, ACT_DIM = 13, 128, 64, 2
ACTIVATIONS = {"tanh": 0, "relu": 1}
SQUASHES = {"clip": 0, "tanh": 1}

# state-dict key -> (ha_weights field, shape); RecurrentActor ignores the critic's keys
ACTOR_KEYS = (
    ("lstm_actor.weight_ih_l0", "w_ih", (4 * HIDDEN, OBS_DIM)),
    ("lstm_actor.weight_hh_l0", "w_hh", (4 * HIDDEN, HIDDEN)),
    ("lstm_actor.bias_ih_l0", "b_ih", (4 * HIDDEN,)),
    ("lstm_actor.bias_hh_l0", "b_hh", (4 * HIDDEN,)),
    ("mlp_extractor.policy_net.0.weight", "w1", (MLP, HIDDEN)),
    ("mlp_extractor.policy_net.0.bias", "b1", (MLP,)),
    ("mlp_extractor.policy_net.2.weight", "w2", (MLP, MLP)),
    ("mlp_extractor.policy_net.2.bias", "b2", (MLP,)),
    ("action_net.weight", "w3", (ACT_DIM, MLP)),
    ("action_net.bias", "b3", (ACT_DIM,)),
    ("log_std", "log_std", (ACT_DIM,)),
)
# the info columns ha_accumulate sums, in he_episode_record's order
RECORD_INFO_KEYS = ("reward_step", "step_pnl_total", "raw_pnl_deviation_abs", "transaction_costs_total",
                    "reward_pnl_component", "transaction_cost_penalty", "per_share_step_pnl")
EPISODE_SUMS = np.dtype([("s", "<f8", (7,)), ("length", "<i8")])
assert EPISODE_SUMS.itemsize == 64

# the critic of the same checkpoint (RecurrentPolicy): state-dict key -> (ha_policy_weights field, shape)
CRITIC_KEYS = (
    ("lstm_critic.weight_ih_l0", "c_w_ih", (4 * HIDDEN, OBS_DIM)),
    ("lstm_critic.weight_hh_l0", "c_w_hh", (4 * HIDDEN, HIDDEN)),
    ("lstm_critic.bias_ih_l0", "c_b_ih", (4 * HIDDEN,)),
    ("lstm_critic.bias_hh_l0", "c_b_hh", (4 * HIDDEN,)),
    ("mlp_extractor.value_net.0.weight", "v1", (MLP, HIDDEN)),
    ("mlp_extractor.value_net.0.bias", "vb1", (MLP,)),
    ("mlp_extractor.value_net.2.weight", "v2", (MLP, MLP)),
    ("mlp_extractor.value_net.2.bias", "vb2", (MLP,)),
    ("value_net.weight", "v3", (1, MLP)),
    ("value_net.bias", "vb3", (1,)),
)
POLICY_KEYS = ACTOR_KEYS + CRITIC_KEYS
HA_POLICY_ABI_VERSION = 1

POLICY_TENSOR_FLOATS = sum(int(np.prod(shape)) for _, _, shape in POLICY_KEYS)   # HA_POLICY_TENSOR_FLOATS
assert POLICY_TENSOR_FLOATS == 171461

_F = ctypes.POINTER(ctypes.c_float)
_D = ctypes.POINTER(ctypes.c_double)


class HaWeights(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("abi_version", "obs_dim", "hidden", "n_lstm_layers", "mlp_width",
                                               "act_dim", "activation", "squash", "has_clip", "reserved")] + \
               [("clip_obs", ctypes.c_double), ("epsilon", ctypes.c_double)] + \
               [(f, _F) for _, f, _ in ACTOR_KEYS] + [("obs_mean", _D), ("obs_var", _D)]


class HaPolicyWeights(ctypes.Structure):
    _fields_ = [(k, ctypes.c_int32) for k in ("abi_version", "obs_dim", "hidden", "n_lstm_layers", "mlp_width",
                                               "act_dim", "activation", "has_clip")] + \
               [("clip_obs", ctypes.c_double), ("epsilon", ctypes.c_double), ("obs_mean", _D), ("obs_var", _D)] + \
               [(f, _F) for _, f, _ in POLICY_KEYS]


_vp, _i32, _i64, _u64, _f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_double
_W, _PW = ctypes.POINTER(HaWeights), ctypes.POINTER(HaPolicyWeights)
# every entry point of include/hedge_actor.h: symbol -> (restype, argtypes)
SIG = {
    "ha_version": (ctypes.c_char_p, []),
    "ha_last_error": (ctypes.c_char_p, [_vp]),
    "ha_create": (_i32, [_W, ctypes.POINTER(_vp)]),
    "ha_destroy": (_i32, [_vp]),
    "ha_step": (_i32, [_vp, _i64] + [_vp] * 8),
    "ha_accumulate": (_i32, [_vp, _i64, _i64] + [_vp] * 10 + [_i64, _vp, _vp]),
    "ha_host_step": (_i32, [_W, _i64] + [_vp] * 7),
    "ha_policy_last_error": (ctypes.c_char_p, [_vp]),
    "ha_policy_create": (_i32, [_PW, ctypes.POINTER(_vp)]),
    "ha_policy_destroy": (_i32, [_vp]),
    "ha_policy_update": (_i32, [_vp, _PW]),
    "ha_policy_step": (_i32, [_vp, _i64, _i64, _u64, _u64, _i32, _i32] + [_vp] * 13),
    "ha_gae": (_i32, [_i64, _i64, _f64, _f64] + [_vp] * 8),
    "ha_host_policy_step": (_i32, [_PW, _i64, _i64, _u64, _u64, _i32, _i32] + [_vp] * 12),
    "ha_host_gae": (_i32, [_i64, _i64, _f64, _f64] + [_vp] * 7),
    "ha_lstm_seq_workspace_bytes": (ctypes.c_size_t, [_i64]),
    "ha_lstm_seq_forward": (_i32, [_i64, _i64, _i64] + [_vp] * 5),
    "ha_lstm_seq_backward": (_i32, [_i64, _i64, _i64] + [_vp] * 4),
    "ha_host_lstm_seq_forward": (_i32, [_i64, _i64, _i64] + [_vp] * 3),
    "ha_host_lstm_seq_backward": (_i32, [_i64, _i64, _i64] + [_vp] * 2),
    "ha_lstm_seq_weight_grads_workspace_bytes": (ctypes.c_size_t, [_i64, _i64, _i64]),
    "ha_lstm_seq_weight_grads": (_i32, [_i64, _i64, _i64] + [_vp] * 5),
    "ha_host_lstm_seq_weight_grads": (_i32, [_i64, _i64, _i64] + [_vp] * 3),
    "ha_policy_refresh": (_i32, [_vp, _PW, _vp]),
    "ha_policy_download": (_i32, [_vp, _vp, _vp]),
    "ha_adam_workspace_bytes": (ctypes.c_size_t, [_i64, _vp]),
    "ha_adam_step": (_i32, [_i64, _vp, _vp, _vp, _vp]),
    "ha_host_adam_step": (_i32, [_i64, _vp, _vp]),
    "ha_ppo_loss_workspace_bytes": (ctypes.c_size_t, [_i64]),
    "ha_ppo_loss": (_i32, [_i64, _vp, _vp, _vp, _vp]),
    "ha_host_ppo_loss": (_i32, [_i64, _vp, _vp]),
    "ha_ppo_heads_workspace_bytes": (ctypes.c_size_t, [_i64]),
    "ha_ppo_heads_forward": (_i32, [_i64, _vp, _vp, _vp, _vp]),
    "ha_ppo_heads_backward": (_i32, [_i64, _vp, _vp, _vp, _vp]),
    "ha_host_ppo_heads_forward": (_i32, [_i64, _vp, _vp]),
    "ha_host_ppo_heads_backward": (_i32, [_i64, _vp, _vp]),
}
EXPORTS = list(SIG)

_lib_ha = None
_torch = None   # the torch module, from the first device handle on (this module imports without torch)


def load(path=LIB_PATH):
    """Load libhedgeactor (once).  Raises if the in-tree library is missing."""
    global _lib_ha
    if _lib_ha is None:
        _lib_ha = _bind.load(path, SIG, _lib.HedgeEnvError, "There is no torch fallback.")
    return _lib_ha


def _check(lib, status, what, handle=None, last_error="ha_last_error"):
    """Raise for a status other than HE_OK with the message of `handle` (None: the calling thread's,
    which either getter returns); last_error names the getter of the handle's kind."""
    if status != _lib.HE_OK:
        msg = (getattr(lib, last_error)(handle) or b"").decode()
        if status in (_lib.HE_ESHAPE, _lib.HE_EINVAL):
            raise ValueError(f"{what}: {msg}")
        raise _lib.HedgeEnvError(f"{what} failed (status {status}): {msg}")


def _net_from_state_dict(sd, lstm_prefix, mlp_prefix, keys, what):
    """One network (`what`: "actor" or "critic") of an SB3 RecurrentPPO state dict: the tensors of
    `keys` as contiguous f32 arrays by field; ValueError unless it is one LSTM layer and 64 -> 64."""
    stem = lstm_prefix + ".weight_ih"
    layers = sorted({k[len(stem):].split("_l")[-1] for k in sd if k.startswith(stem)})
    if layers != ["0"]:
        raise ValueError(f"{lstm_prefix} has layers {layers}: only n_lstm_layers=1 is built")
    extra = sorted(k for k in sd if k.startswith(mlp_prefix) and k.split(".")[2] not in ("0", "2"))
    if extra:
        raise ValueError(f"{mlp_prefix.split('.')[1]} has layers beyond 64 -> 64: {extra}")
    out = {}
    for key, field, shape in keys:
        if key not in sd:
            raise ValueError(f"state dict has no {key!r}")
        t = sd[key]
        a = t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)
        if tuple(a.shape) != shape:
            raise ValueError(f"{key} has shape {tuple(a.shape)}, this {what} is built for {shape} (obs 13, "
                             f"lstm_hidden_size 128, net_arch 64-64, {'2 actions' if what == 'actor' else '1 value'})")
        out[field] = np.ascontiguousarray(a, dtype=np.float32)
    return out


def weights_from_state_dict(sd):
    """The 11 actor tensors of an SB3 RecurrentPPO state dict as contiguous f32 arrays, keyed by
    ha_weights field; ValueError for any architecture but 13 -> LSTM 128 x 1 -> 64 -> 64 -> 2."""
    return _net_from_state_dict(sd, "lstm_actor", "mlp_extractor.policy_net.", ACTOR_KEYS, "actor")


def policy_weights_from_state_dict(sd):
    """The actor's 11 and the critic's 10 tensors of an SB3 RecurrentPPO state dict, keyed by
    ha_policy_weights field.  ValueError unless the critic has its own LSTM (sb3_contrib's default,
    enable_critic_lstm=True and shared_lstm=False) of the actor's shape."""
    out = weights_from_state_dict(sd)
    if not any(k.startswith("lstm_critic.") for k in sd):
        raise ValueError("state dict has no lstm_critic.*: RecurrentPolicy is built for a critic with its own LSTM "
                         "(enable_critic_lstm=True, shared_lstm=False); shared_lstm=True and a critic without an "
                         "LSTM (enable_critic_lstm=False) are not")
    out.update(_net_from_state_dict(sd, "lstm_critic", "mlp_extractor.value_net.", CRITIC_KEYS, "critic"))
    return out


def _read_sb3_zip(path):
    """The state dict of an SB3 `model.save()` zip: its policy.pth is a plain torch state dict."""
    import torch
    with zipfile.ZipFile(path) as z:
        return torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)


def _normalization(norm):
    """-> (obs_mean, obs_var, overrides) from a dict, a pickle path or a DeviceVecNormalize."""
    if norm is None:
        return None, None, {}
    if isinstance(norm, (str, os.PathLike)):
        with open(norm, "rb") as f:
            norm = pickle.load(f)
    if isinstance(norm, dict):
        return norm["obs_mean"], norm["obs_var"], {}
    rms = norm.obs_rms   # a DeviceVecNormalize (or anything with SB3 VecNormalize's attributes)
    return rms.mean, rms.var, {"clip_obs": float(norm.clip_obs), "epsilon": float(norm.epsilon)}


class _Recurrent:
    """What RecurrentActor and RecurrentPolicy share: the weights struct (self._w, pointing into
    self._arrays) from tensors, statistics and activation, the loaders, the device handle made with
    the first device call, and the validation of a step's inputs.  A subclass names its struct, key
    table, state attributes and entry points, and adds what differs."""

    _struct = _abi = _keys = _fields_of = None   # ctypes struct, its abi_version, key table, state dict -> fields
    _states = ()                                 # the attributes holding [n, ...] device tensors
    _create = _destroy = _last_error = None      # entry-point names

    def __init__(self, weights, obs_mean, obs_var, clip_obs, epsilon, activation, device):
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(ACTIVATIONS)}, not {activation!r}")
        if (obs_mean is None) != (obs_var is None):
            raise ValueError("obs_mean and obs_var come together")
        self.lib = load()
        self._arrays = {}
        w = self._w = self._struct()
        w.abi_version = self._abi
        w.obs_dim, w.hidden, w.n_lstm_layers, w.mlp_width, w.act_dim = OBS_DIM, HIDDEN, 1, MLP, ACT_DIM
        w.activation = ACTIVATIONS[activation]
        w.has_clip = 0 if clip_obs is None else 1
        w.clip_obs = 0.0 if clip_obs is None else float(clip_obs)
        w.epsilon = float(epsilon)
        self._set_tensors(weights)
        if obs_mean is not None:
            for name, v in (("obs_mean", obs_mean), ("obs_var", obs_var)):
                a = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1))
                if a.shape != (OBS_DIM,):
                    raise ValueError(f"{name} has {a.size} entries, the obs has {OBS_DIM}")
                self._arrays[name] = a
                setattr(w, name, a.ctypes.data_as(_D))
        self.activation = activation
        self.clip_obs, self.epsilon = clip_obs, float(epsilon)
        self.device_name = device
        self._h = None          # the library's handle, made with the first device call
        self.device = None
        for k in self._states:  # [n, ...] device tensors (reset_states)
            setattr(self, k, None)

    def _set_tensors(self, weights):
        if any("." in k for k in weights):
            weights = self._fields_of(weights)
        arrays = {}
        for _, field, shape in self._keys:
            a = np.ascontiguousarray(weights[field], dtype=np.float32)
            if a.shape != shape:
                raise ValueError(f"{field} has shape {a.shape}, expected {shape}")
            arrays[field] = a
        self._arrays.update(arrays)   # the struct points into these: they live as long as it does
        for field, a in arrays.items():
            setattr(self._w, field, a.ctypes.data_as(_F))

    # ------------------------------------------------------------------ loaders
    @classmethod
    def from_state_dict(cls, sd, normalization=None, **kw):
        mean, var, over = _normalization(normalization)
        return cls(cls._fields_of(sd), obs_mean=mean, obs_var=var, **dict(over, **kw))

    @classmethod
    def from_sb3_zip(cls, path, normalization=None, **kw):
        """An SB3 `model.save()` zip: its policy.pth is a plain torch state dict."""
        return cls.from_state_dict(_read_sb3_zip(path), normalization=normalization, **kw)

    # ------------------------------------------------------------------ device
    def _handle(self):
        if self._h is None:
            global _torch
            import torch
            _torch = torch
            dev = torch.device(self.device_name)
            if dev.type != "cuda" or not torch.cuda.is_available():
                raise _lib.HedgeEnvError(f"{type(self).__name__}.step runs on a HIP device (cuda:N); "
                                         "host_step is the CPU build")
            dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
            h = ctypes.c_void_p()
            with torch.cuda.device(dev):
                st = getattr(self.lib, self._create)(ctypes.byref(self._w), ctypes.byref(h))
                _check(self.lib, st, self._create, None, self._last_error)
            self._h, self.device = h, dev
        return self._h

    def _stream(self):
        return _bind.stream(self.device.index)

    def _begin_step(self, obs, episode_start):
        """The head of a device step: the handle, and obs [n,13] f32 and episode_start [n] u8 / bool
        device tensors checked -> (handle, n, episode_start as uint8).  One call a step: at small env
        counts the step is bound by this Python."""
        h = self._h if self._h is not None else self._handle()
        torch = _torch
        n = int(obs.shape[0])
        if obs.dtype != torch.float32 or not obs.is_contiguous() or obs.device != self.device or obs.shape[1] != OBS_DIM:
            raise ValueError(f"obs must be a contiguous float32 [n, {OBS_DIM}] tensor on {self.device}")
        if episode_start.dtype == torch.bool:
            episode_start = episode_start.view(torch.uint8)
        if episode_start.dtype != torch.uint8 or episode_start.numel() != n or not episode_start.is_contiguous():
            raise ValueError("episode_start must be a contiguous uint8 / bool [n] tensor")
        return h, n, episode_start

    @staticmethod
    def _host_inputs(obs, episode_start, names, states):
        """host_step's NumPy inputs: obs [n,13] and episode_start [n] converted, `states` (C-contiguous
        float32 [n,128] arrays, updated in place by the call) checked -> (obs, episode_start, n)."""
        obs = np.ascontiguousarray(obs, dtype=np.float32)
        n = obs.shape[0]
        es = np.ascontiguousarray(np.asarray(episode_start).reshape(-1), dtype=np.uint8)
        if obs.shape != (n, OBS_DIM) or es.shape != (n,):
            raise ValueError(f"obs must be [n, {OBS_DIM}] and episode_start [n]")
        for name, a in zip(names, states):
            if not (isinstance(a, np.ndarray) and a.dtype == np.float32 and a.flags.c_contiguous
                    and a.shape == (n, HIDDEN)):
                raise ValueError(f"{name} must be a C-contiguous float32 [{n}, {HIDDEN}] array")
        return obs, es, n

    def close(self):
        if self._h is not None:
            import torch
            torch.cuda.synchronize(self.device)
            getattr(self.lib, self._destroy)(self._h)
            self._h = None
        for k in self._states:
            setattr(self, k, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RecurrentActor(_Recurrent):
    """The deterministic actor of a RecurrentPPO checkpoint.

    weights: {field: array} (weights_from_state_dict) or a state dict.  obs_mean / obs_var (f64
    [13]): VecNormalize's frozen statistics, applied as SB3 does (clip_obs=None: no clip, the
    QuantConnect wrapper); without them the obs are used as they come (e.g. a DeviceVecNormalize
    eval output).  activation: the MLP's ("tanh": SB3's default, "relu": model_wrapper.py);
    squash: "clip" (SB3 predict) or "tanh" (model_wrapper.py)."""

    _struct, _abi, _keys, _fields_of = HaWeights, HA_ABI_VERSION, ACTOR_KEYS, staticmethod(weights_from_state_dict)
    _states = ("h", "c", "_sums")   # h, c [n, 128]; the episode sums
    _create, _destroy, _last_error = "ha_create", "ha_destroy", "ha_last_error"

    def __init__(self, weights, obs_mean=None, obs_var=None, clip_obs=10.0, epsilon=1e-8, activation="tanh",
                 squash="clip", device="cuda:0"):
        if squash not in SQUASHES:
            raise ValueError(f"squash must be one of {sorted(SQUASHES)}, not {squash!r}")
        super().__init__(weights, obs_mean, obs_var, clip_obs, epsilon, activation, device)
        self._w.squash = SQUASHES[squash]
        self.squash = squash

    def reset_states(self, n_envs):
        """Zero h, c (and the episode sums) for n_envs envs."""
        import torch
        self._handle()
        n = int(n_envs)
        if self.h is None or self.h.shape[0] != n:
            self.h = torch.zeros((n, HIDDEN), dtype=torch.float32, device=self.device)
            self.c = torch.zeros((n, HIDDEN), dtype=torch.float32, device=self.device)
            self._sums = torch.zeros((n, EPISODE_SUMS.itemsize), dtype=torch.uint8, device=self.device)
        else:
            self.h.zero_()
            self.c.zero_()
            self._sums.zero_()
        return self.h, self.c

    def step(self, obs, episode_start, out=None, mean_out=None, obs_norm_out=None):
        """obs [n,13] f32, episode_start [n] u8 / bool device tensors -> actions [n,2]; h, c are
        updated in place.  Enqueued on the current stream, no host sync."""
        import torch
        h, n, episode_start = self._begin_step(obs, episode_start)
        if self.h is None or self.h.shape[0] != n:
            self.reset_states(n)
        if out is None:
            out = torch.empty((n, ACT_DIM), dtype=torch.float32, device=self.device)
        for t, w in ((out, ACT_DIM), (mean_out, ACT_DIM), (obs_norm_out, OBS_DIM)):
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n * w):
                raise ValueError("output tensors must be contiguous float32 of the step's shape")
        st = self.lib.ha_step(h, n, obs.data_ptr(), episode_start.data_ptr(), self.h.data_ptr(), self.c.data_ptr(),
                              out.data_ptr(), None if mean_out is None else mean_out.data_ptr(),
                              None if obs_norm_out is None else obs_norm_out.data_ptr(), self._stream())
        _check(self.lib, st, "ha_step", h)
        return out

    def accumulate(self, info, terminated, records, record_count, env_id_offset=0):
        """One env step's info columns ({key: f64 [n] device tensor}, RECORD_INFO_KEYS) into the
        per-env episode sums; envs with `terminated` set append an EPISODE_RECORD row to
        `records` (uint8 [cap, 80]) at `record_count` (int64 [1]) and restart their sums."""
        h = self._handle()
        n = int(terminated.numel())
        cols = [info[k].data_ptr() for k in RECORD_INFO_KEYS]
        cap = 0 if records is None else int(records.shape[0])
        st = self.lib.ha_accumulate(h, n, int(env_id_offset), *cols, terminated.data_ptr(), self._sums.data_ptr(),
                                    None if records is None else records.data_ptr(), cap, record_count.data_ptr(),
                                    self._stream())
        _check(self.lib, st, "ha_accumulate", h)

    # ------------------------------------------------------------------ host
    def host_step(self, obs, episode_start, h, c, mean_out=None, obs_norm_out=None):
        """ha_host_step over NumPy: obs [n,13] f32, episode_start [n], h / c [n,128] f32 C-contiguous
        arrays updated IN PLACE; returns actions [n,2].  The device kernel's arithmetic on the CPU."""
        obs, es, n = self._host_inputs(obs, episode_start, ("h", "c"), (h, c))
        act = np.empty((n, ACT_DIM), np.float32)
        for a, w in ((mean_out, ACT_DIM), (obs_norm_out, OBS_DIM)):
            if a is not None and not (a.dtype == np.float32 and a.flags.c_contiguous and a.shape == (n, w)):
                raise ValueError("mean_out / obs_norm_out must be C-contiguous float32 of the step's shape")
        st = self.lib.ha_host_step(ctypes.byref(self._w), n, obs.ctypes.data, es.ctypes.data, h.ctypes.data,
                                   c.ctypes.data, act.ctypes.data, None if mean_out is None else mean_out.ctypes.data,
                                   None if obs_norm_out is None else obs_norm_out.ctypes.data)
        _check(self.lib, st, "ha_host_step")
        return act


STATE_NAMES = ("h_pi", "c_pi", "h_vf", "c_vf")
# ha_policy_step's outputs: name -> trailing shape
STEP_OUTPUTS = (("actions", (ACT_DIM,)), ("env_actions", (ACT_DIM,)), ("values", ()), ("log_probs", ()),
                ("mean", (ACT_DIM,)), ("obs_norm", (OBS_DIM,)))
_REQUIRED_OUT = ("actions", "env_actions", "values", "log_probs")


class RecurrentPolicy(_Recurrent):
    """Actor and critic of a RecurrentPPO checkpoint for rollout collection (collect.RolloutCollector):
    per step the sampled action, its clipped form, the value and the log-probability of every env in
    one kernel launch (ha_policy_step), and GAE over the filled buffer (ha_gae).

    weights: {field: array} (policy_weights_from_state_dict) or a state dict.  obs_mean / obs_var,
    clip_obs, epsilon, activation: as RecurrentActor; leave the statistics out when the env is a
    DeviceVecNormalize, whose obs are normalised already.  The four LSTM states live on the device
    as h_pi, c_pi, h_vf, c_vf [n, 128].  After a PPO update the new tensors come in through
    load_state_dict (host arrays or tensors, waits for the device) or load_device_state_dict (device
    tensors, one launch on the stream)."""

    _struct, _abi, _keys = HaPolicyWeights, HA_POLICY_ABI_VERSION, POLICY_KEYS
    _fields_of = staticmethod(policy_weights_from_state_dict)
    _states = STATE_NAMES
    _create, _destroy, _last_error = "ha_policy_create", "ha_policy_destroy", "ha_policy_last_error"
    _host_stale = False

    def __init__(self, weights, obs_mean=None, obs_var=None, clip_obs=10.0, epsilon=1e-8, activation="tanh",
                 device="cuda:0"):
        super().__init__(weights, obs_mean, obs_var, clip_obs, epsilon, activation, device)
        self._host_stale = False   # load_device_state_dict ran: self._arrays are older than the handle's tensors

    def load_state_dict(self, sd):
        """New tensors (a state dict or {field: array}) after a PPO update: ha_policy_update re-packs
        and re-uploads them into the existing handle.  Waits for the device; the LSTM states stay."""
        self._set_tensors(sd)
        self._host_stale = False   # all 21 host copies are new, and ha_policy_update uploads them
        if self._h is not None:
            import torch
            with torch.cuda.device(self.device):
                st = self.lib.ha_policy_update(self._h, ctypes.byref(self._w))
            _check(self.lib, st, "ha_policy_update", self._h, "ha_policy_last_error")

    def load_device_state_dict(self, sd):
        """load_state_dict without the host: sd (a state dict such as module.state_dict(), or {field:
        tensor}) holds contiguous float32 tensors on the policy's device, and ha_policy_refresh re-packs
        them into the handle with one launch on the current stream.  Returns without waiting: a step
        enqueued afterwards on that stream runs the new tensors, and the tensors may change again once
        the call has returned only in work enqueued behind it.  Statistics, activation and the LSTM
        states stay.  ValueError (and the handle as it was) for a missing key, a wrong shape or dtype,
        a tensor that is not contiguous or not on the device.  The host copies (host_step,
        RecurrentPPOModule.from_policy) follow on demand: _host_weights."""
        h = self._handle()
        torch = _torch
        dotted = any("." in k for k in sd)
        w = type(self._w).from_buffer_copy(self._w)
        for key, field, shape in self._keys:
            name = key if dotted else field
            t = sd.get(name)
            if t is None:
                raise ValueError(f"state dict has no {name!r}")
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape \
                    or t.device != self.device or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous float32 tensor of shape {shape} on {self.device}, not "
                                 f"{getattr(t, 'dtype', type(t))} {tuple(getattr(t, 'shape', ()))} on "
                                 f"{getattr(t, 'device', 'the host')}")
            setattr(w, field, ctypes.cast(ctypes.c_void_p(t.data_ptr()), _F))
        st = self.lib.ha_policy_refresh(h, ctypes.byref(w), self._stream())
        _check(self.lib, st, "ha_policy_refresh", h, "ha_policy_last_error")
        self._host_stale = True

    def _host_weights(self):
        """(the weights struct, the arrays it points into) for whatever reads the tensors on the host.
        After load_device_state_dict the first call downloads the handle's copy of the tensors the refresh
        read (ha_policy_download: the one wait, on the current stream); later calls cost nothing."""
        if self._host_stale:
            flat = np.empty(POLICY_TENSOR_FLOATS, np.float32)
            with _torch.cuda.device(self.device):
                st = self.lib.ha_policy_download(self._h, flat.ctypes.data, self._stream())
            _check(self.lib, st, "ha_policy_download", self._h, "ha_policy_last_error")
            arrays, o = {}, 0
            for _, field, shape in self._keys:   # POLICY_KEYS is in ha_policy_weights' order
                n = int(np.prod(shape))
                arrays[field] = flat[o:o + n].reshape(shape)
                o += n
            self._set_tensors(arrays)
            self._host_stale = False
        return self._w, self._arrays

    def close(self):
        try:
            if self._h is not None and self._host_stale:
                self._host_weights()   # the handle holds the only copy of the current tensors
        finally:
            super().close()

    @property
    def states(self):
        return tuple(getattr(self, k) for k in STATE_NAMES)

    def reset_states(self, n_envs):
        """Zero the four LSTM states for n_envs envs; returns (h_pi, c_pi, h_vf, c_vf)."""
        import torch
        self._handle()
        n = int(n_envs)
        if self.h_pi is None or self.h_pi.shape[0] != n:
            for k in STATE_NAMES:
                setattr(self, k, torch.zeros((n, HIDDEN), dtype=torch.float32, device=self.device))
        else:
            for t in self.states:
                t.zero_()
        return self.states

    def step(self, obs, episode_start, seed, step_index, deterministic=False, write_state=True, env_id_offset=0,
             out=None):
        """One collection step: obs [n,13] f32, episode_start [n] u8 / bool device tensors ->
        {"actions", "env_actions" [n,2], "values", "log_probs" [n]} (and "mean" [n,2], "obs_norm"
        [n,13] where `out` has them).  `out`: a dict of preallocated contiguous f32 tensors to write
        into, e.g. the [k] slices of a rollout buffer.  The noise of env e is a function of (seed,
        step_index, env_id_offset + e) alone.  write_state=False leaves the LSTM states as they are
        (SB3's predict_values).  Enqueued on the current stream, no host sync."""
        import torch
        h, n, episode_start = self._begin_step(obs, episode_start)
        if self.h_pi is None or self.h_pi.shape[0] != n:
            self.reset_states(n)
        res = dict(out) if out else {}
        ptr = []
        for name, tail in STEP_OUTPUTS:
            t = res.get(name)
            if t is None and name in _REQUIRED_OUT:
                t = res[name] = torch.empty((n,) + tail, dtype=torch.float32, device=self.device)
            if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != self.device
                                  or t.numel() != n * int(np.prod(tail, dtype=np.int64))):
                raise ValueError(f"out[{name!r}] must be a contiguous float32 tensor of {n} x {tail} on {self.device}")
            ptr.append(None if t is None else t.data_ptr())
        st = self.lib.ha_policy_step(h, n, int(env_id_offset), int(seed) & (2 ** 64 - 1), int(step_index),
                                     int(bool(deterministic)), int(bool(write_state)), obs.data_ptr(),
                                     episode_start.data_ptr(), *(t.data_ptr() for t in self.states), *ptr,
                                     self._stream())
        _check(self.lib, st, "ha_policy_step", h, "ha_policy_last_error")
        return res

    def gae(self, rewards, values, episode_starts, last_values, last_dones, gamma, gae_lambda, advantages=None,
            returns=None):
        """SB3's compute_returns_and_advantage over [K,N] device tensors (ha_gae) ->
        (advantages, returns) [K,N] f32.  No host sync."""
        import torch
        self._handle()
        K, n = (int(x) for x in rewards.shape)
        if advantages is None:
            advantages = torch.empty((K, n), dtype=torch.float32, device=self.device)
        if returns is None:
            returns = torch.empty((K, n), dtype=torch.float32, device=self.device)
        u8 = []
        for t in (episode_starts, last_dones):
            u8.append(t.view(torch.uint8) if t.dtype == torch.bool else t)
        for name, t, dt, numel in (("rewards", rewards, torch.float32, K * n), ("values", values, torch.float32, K * n),
                                   ("episode_starts", u8[0], torch.uint8, K * n),
                                   ("last_values", last_values, torch.float32, n), ("last_dones", u8[1], torch.uint8, n),
                                   ("advantages", advantages, torch.float32, K * n),
                                   ("returns", returns, torch.float32, K * n)):
            if t.dtype != dt or not t.is_contiguous() or t.numel() != numel or t.device != self.device:
                raise ValueError(f"{name} must be a contiguous {dt} tensor of {numel} elements on {self.device}")
        st = self.lib.ha_gae(n, K, float(gamma), float(gae_lambda), rewards.data_ptr(), values.data_ptr(),
                             u8[0].data_ptr(), last_values.data_ptr(), u8[1].data_ptr(), advantages.data_ptr(),
                             returns.data_ptr(), self._stream())
        _check(self.lib, st, "ha_gae")
        return advantages, returns

    # ------------------------------------------------------------------ host
    def host_step(self, obs, episode_start, states, seed, step_index, deterministic=False, write_state=True,
                  env_id_offset=0):
        """ha_host_policy_step over NumPy: obs [n,13], episode_start [n], states = (h_pi, c_pi, h_vf,
        c_vf), C-contiguous float32 [n,128] arrays updated IN PLACE (unless write_state=False) ->
        a dict of every output of STEP_OUTPUTS.  The device kernel's arithmetic on the CPU."""
        if len(states) != 4:
            raise ValueError("states is (h_pi, c_pi, h_vf, c_vf)")
        obs, es, n = self._host_inputs(obs, episode_start, STATE_NAMES, states)
        res = {name: np.empty((n,) + tail, np.float32) for name, tail in STEP_OUTPUTS}
        w, _ = self._host_weights()
        st = self.lib.ha_host_policy_step(ctypes.byref(w), n, int(env_id_offset), int(seed) & (2 ** 64 - 1),
                                          int(step_index), int(bool(deterministic)), int(bool(write_state)),
                                          obs.ctypes.data, es.ctypes.data, *(a.ctypes.data for a in states),
                                          *(res[name].ctypes.data for name, _ in STEP_OUTPUTS))
        _check(self.lib, st, "ha_host_policy_step")
        return res

    def host_gae(self, rewards, values, episode_starts, last_values, last_dones, gamma, gae_lambda):
        """ha_host_gae over [K,N] NumPy arrays -> (advantages, returns)."""
        rewards = np.ascontiguousarray(rewards, dtype=np.float32)
        K, n = rewards.shape
        values = np.ascontiguousarray(values, dtype=np.float32)
        es = np.ascontiguousarray(episode_starts, dtype=np.uint8)
        lv = np.ascontiguousarray(last_values, dtype=np.float32)
        ld = np.ascontiguousarray(last_dones, dtype=np.uint8)
        if values.shape != (K, n) or es.shape != (K, n) or lv.shape != (n,) or ld.shape != (n,):
            raise ValueError("rewards, values, episode_starts are [K, N]; last_values, last_dones [N]")
        adv = np.empty((K, n), np.float32)
        ret = np.empty((K, n), np.float32)
        st = self.lib.ha_host_gae(n, K, float(gamma), float(gae_lambda), rewards.ctypes.data, values.ctypes.data,
                                  es.ctypes.data, lv.ctypes.data, ld.ctypes.data, adv.ctypes.data, ret.ctypes.data)
        _check(self.lib, st, "ha_host_gae")
        return adv, ret
