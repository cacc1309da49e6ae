"""ctypes binding of libhedgeenv (include/hedge_env.h).

The shared library is built in-tree (`cantorrl_amd/lib/libhedgeenv.so`, see
`cantorrl_amd/build.py`).  There is no fallback: if the library cannot be
loaded, every constructor raises (the loader itself is _bind.load).
"""
import ctypes
import os

from . import _bind

HERE = os.path.dirname(os.path.abspath(__file__))
# CANTORRL_HEDGEENV_LIB: an alternative build (diagnostic / A-B builds under tools/ab/)
LIB_PATH = os.environ.get("CANTORRL_HEDGEENV_LIB") or os.path.join(HERE, "lib", "libhedgeenv.so")

HE_ABI_VERSION = 4
HE_BOOK_MAX = 8
HE_OBS_DIM = 13
BOOK_TYPES = {"call": 0, "put": 1, "uo_call": 2}
HE_OK, HE_EINVAL, HE_ESHAPE, HE_EHIP, HE_ENOMEM, HE_ESTATE = range(6)
HE_MODE_REPLAY, HE_MODE_GBM, HE_MODE_HESTON = range(3)
HE_LOSS_MSE, HE_LOSS_ABS, HE_LOSS_CVAR, HE_LOSS_OTHER = range(4)
MODES = {"replay": HE_MODE_REPLAY, "gbm": HE_MODE_GBM, "heston": HE_MODE_HESTON}
# he_mark: rolling ATM (rbergomi_sim.py:418,437-446) or the fixed-strike European of
# option_price_assignment.py:10-21,33-49
HE_MARK_ROLLING_ATM, HE_MARK_FIXED_EUROPEAN = range(2)
MARKS = {"rolling_atm": HE_MARK_ROLLING_ATM, "fixed_european": HE_MARK_FIXED_EUROPEAN}


def loss_code(loss_type):
    """hedging_env_v2.py:246-253: "mse", "abs", "cvar", anything else = |x| branch."""
    return {"mse": HE_LOSS_MSE, "abs": HE_LOSS_ABS, "cvar": HE_LOSS_CVAR}.get(loss_type, HE_LOSS_OTHER)


class HeBookOption(ctypes.Structure):
    _fields_ = [
        ("type", ctypes.c_int32),
        ("expiry", ctypes.c_int32),
        ("strike", ctypes.c_double),
        ("barrier", ctypes.c_double),
        ("quantity", ctypes.c_double),
    ]


class HeConfig(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32),
        ("variant", ctypes.c_int32),
        ("mode", ctypes.c_int32),
        ("loss_type", ctypes.c_int32),
        ("n_envs", ctypes.c_int64),
        ("global_env_offset", ctypes.c_int64),
        ("transaction_cost_per_contract", ctypes.c_double),
        ("lambda_cost", ctypes.c_double),
        ("pnl_penalty_weight", ctypes.c_double),
        ("theta_weight", ctypes.c_double),
        ("slippage_bps", ctypes.c_double),
        ("initial_cash", ctypes.c_double),
        ("shares_to_hedge", ctypes.c_int64),
        ("max_contracts_held_per_type", ctypes.c_int32),
        ("max_trade_per_step", ctypes.c_int32),
        ("record_metrics", ctypes.c_int32),
        ("autoreset", ctypes.c_int32),
        ("risk_free_rate", ctypes.c_double),
        ("option_tenor_years", ctypes.c_double),
        ("episode_length", ctypes.c_int32),
        ("device", ctypes.c_int32),
        ("seed", ctypes.c_uint64),
        ("s0", ctypes.c_double),
        ("variance", ctypes.c_double),
        ("mu", ctypes.c_double),
        ("dt", ctypes.c_double),
        ("heston_kappa", ctypes.c_double),
        ("heston_theta", ctypes.c_double),
        ("heston_xi", ctypes.c_double),
        ("heston_rho", ctypes.c_double),
        ("market_block", ctypes.c_int32),
        ("market_prefetch", ctypes.c_int32),
        ("book_size", ctypes.c_int32),
        ("mark", ctypes.c_int32),
        ("book", HeBookOption * HE_BOOK_MAX),
        ("reserved", ctypes.c_double * 7),
    ]


POLICIES = {"no_hedge": 0, "delta_every_step": 1, "delta_threshold": 2}

# he_episode_record as a numpy structured dtype (64 B, include/hedge_env.h)
import numpy as _np  # noqa: E402
EPISODE_RECORD = _np.dtype([("env_id", "<i8"), ("length", "<i4"), ("reserved", "<i4"), ("reward_sum", "<f8"),
                            ("pnl_sum", "<f8"), ("abs_pnl_sum", "<f8"), ("cost_sum", "<f8"),
                            ("pnl_penalty_sum", "<f8"), ("cost_penalty_sum", "<f8"),
                            ("per_share_pnl_sum", "<f8"), ("reserved2", "<f8")])
assert EPISODE_RECORD.itemsize == 80

INFO_FIELDS = [
    ("step_pnl_total", "f8"), ("per_share_step_pnl", "f8"), ("raw_pnl_deviation_abs", "f8"),
    ("transaction_costs_total", "f8"), ("commission_cost", "f8"), ("slippage_cost", "f8"),
    ("reward_pnl_component", "f8"), ("transaction_cost_penalty", "f8"), ("theta_penalty", "f8"),
    ("reward_step", "f8"), ("portfolio_value", "f8"), ("cash", "f8"),
    ("call_contracts", "i4"), ("put_contracts", "i4"),
    ("scaled_float_call", "f4"), ("scaled_float_put", "f4"),
    ("requested_calls_rounded_clipped", "i4"), ("requested_puts_rounded_clipped", "i4"),
    ("actual_calls_traded", "i4"), ("actual_puts_traded", "i4"),
    ("initial_S0_for_episode", "f4"),
    ("current_stock_price", "f4"), ("current_volatility", "f4"),
    ("current_call_price", "f4"), ("current_put_price", "f4"), ("current_step", "i4"),
    ("current_episode_idx", "i4"),
]


class HeInfo(ctypes.Structure):
    _fields_ = [(name, ctypes.c_void_p) for name, _ in INFO_FIELDS]


class HeVecnormParams(ctypes.Structure):
    _fields_ = [
        ("obs_dim", ctypes.c_int32),
        ("training", ctypes.c_int32),
        ("norm_obs", ctypes.c_int32),
        ("norm_reward", ctypes.c_int32),
        ("gamma", ctypes.c_double),
        ("clip_obs", ctypes.c_double),
        ("clip_reward", ctypes.c_double),
        ("epsilon", ctypes.c_double),
        ("moments", ctypes.c_int32),   # HE_VN_MOMENTS_F64 (0) / HE_VN_MOMENTS_SB3
        ("reserved", ctypes.c_int32 * 3),
    ]


HE_VN_MOMENTS_F64, HE_VN_MOMENTS_SB3 = range(2)
HE_VN_SB3_MAX_ENVS = 4096
HE_VN_STEP_MAX_ENVS = 256   # he_vecnorm_attach_step: one step workgroup
VN_MOMENTS = {"f64": HE_VN_MOMENTS_F64, "sb3": HE_VN_MOMENTS_SB3}


class HeVecnormOut(ctypes.Structure):
    """include/hedge_env.h he_vecnorm_out: the eval VecNormalize step's buffers."""
    _fields_ = [(name, ctypes.c_void_p) for name in (
        "stats", "returns", "obs_out", "reward_out", "terminal_obs_out", "ep_return", "ep_length", "ep_return_done",
        "ep_length_done")]

_vp, _i32, _i64, _u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64
_cfgp, _infop, _vnp = ctypes.POINTER(HeConfig), ctypes.POINTER(HeInfo), ctypes.POINTER(HeVecnormParams)
# every entry point of include/hedge_env.h: symbol -> (restype, argtypes)
SIG = {
    "he_config_init": (_i32, [_cfgp, _i32]),
    "he_create": (_i32, [_cfgp, ctypes.POINTER(_vp)]),
    "he_destroy": (_i32, [_vp]),
    "he_last_error": (ctypes.c_char_p, [_vp]),
    "he_version": (ctypes.c_char_p, []),
    "he_load_paths": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64]),
    "he_seed": (_i32, [_vp, _vp, _vp, _i64]),
    "he_reset": (_i32, [_vp, _vp, _i64, _vp, _infop, _vp]),
    "he_reset_episodes": (_i32, [_vp, _vp, _vp, _i64, _vp, _infop, _vp]),
    "he_step": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _infop, _vp]),
    "he_rollout": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "he_rollout_policy": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "he_num_envs": (_i64, [_vp]),
    "he_episode_length": (_i32, [_vp]),
    "he_num_episodes": (_i64, [_vp]),
    "he_get_config": (_i32, [_vp, _cfgp]),
    "he_state_size": (ctypes.c_size_t, [_vp]),
    "he_get_state": (_i32, [_vp, _vp, ctypes.c_size_t]),
    "he_set_state": (_i32, [_vp, _vp, ctypes.c_size_t]),
    "he_pcg64_seed_state": (_i32, [_u64, ctypes.POINTER(ctypes.c_uint64 * 4)]),
    "he_host_episode_draws": (_i32, [_u64, _u64, _i64, _vp]),
    "he_host_philox": (_i32, [_u64, _u64, _u64, ctypes.POINTER(ctypes.c_uint32 * 4)]),
    "he_host_div_by": (_i32, [_vp, _i64, ctypes.c_double, _vp]),
    "he_host_div_byf": (_i32, [_vp, _i64, ctypes.c_float, _vp]),
    "he_host_box_muller": (_i32, [_vp, _vp, _i64, _vp, _vp]),
    "he_time_next_step": (_i32, [_vp, _vp, _vp]),
    "he_sync_market": (_i32, [_vp, _vp]),
    "he_vecnorm_stats_len": (_i64, [_i32]),
    "he_vecnorm_scratch_bytes": (_i64, [_i64, _i32]),
    "he_vecnorm_init": (_i32, [_vp, _i32, _vp]),
    "he_vecnorm_step": (_i32, [_vnp, _i64] + [_vp] * 15 + [_vp]),
    "he_vecnorm_apply": (_i32, [_vnp, _i64] + [_vp] * 15 + [_vp]),
    "he_vecnorm_attach": (_i32, [_vp, _vnp, _vp, _vp, _vp]),
    "he_vecnorm_attach_eval": (_i32, [_vp, _vnp, ctypes.POINTER(HeVecnormOut)]),
    "he_vecnorm_attach_step": (_i32, [_vp, _vnp, ctypes.POINTER(HeVecnormOut), _vp]),
    "he_vecnorm_reset": (_i32, [_vnp, _i64] + [_vp] * 5 + [_vp]),
    "he_host_vecnorm_sb3": (_i32, [_vnp, _i64] + [_vp] * 9),
    "he_fixed_european_marks": (_i32, [_vp, _i64, _i32, ctypes.c_double, _vp, _vp, _vp, _vp]),
    "he_bs_delta_hedge": (_i32, [_vp, _i64, _i32, ctypes.c_double, ctypes.c_double, _vp, _vp]),
    "he_count_nonfinite": (_i32, [_vp, _i64, _vp, _vp]),
    "he_device_rng": (_i32, [_u64, _vp, _vp, _i64, _vp, _vp, _vp]),
    "he_device_math": (_i32, [_i32, _vp, _i64, _vp, _vp]),
    "he_host_math": (_i32, [_i32, _vp, _i64, _vp]),
    "he_host_episode_wrap": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp]),
    "he_episode_summaries": (_i32, [_vp, _vp, _vp]),
    "he_host_alloc": (_i32, [ctypes.c_size_t, ctypes.POINTER(_vp), ctypes.POINTER(_vp)]),
    "he_host_free": (_i32, [_vp]),
    "he_stream_wait": (_i32, [_vp]),
    "he_step_signal": (_i32, [_vp, _vp]),
    "he_signal_seq": (ctypes.c_uint32, [_vp]),
    "he_signal_wait": (_i32, [_vp, _vp, _vp]),
}
EXPORTS = list(SIG)

_lib = None


class HedgeEnvError(RuntimeError):
    pass


def load(path=LIB_PATH):
    """Load libhedgeenv (once).  Raises if the in-tree library is missing.  A build from
    another place (an A/B build of an older tree) may lack the newer entry points."""
    global _lib
    if _lib is None:
        _lib = _bind.load(path, SIG, HedgeEnvError, "There is no CPU fallback.",
                          missing_ok=path != os.path.join(HERE, "lib", "libhedgeenv.so"))
    return _lib


def check(lib, handle, status, what):
    if status != HE_OK:
        msg = lib.he_last_error(handle).decode() if handle else ""
        if status == HE_ESHAPE:
            raise ValueError(msg or "Data shapes are inconsistent.")
        raise HedgeEnvError(f"{what} failed (status {status}): {msg}")


def pcg64_seed_state(seed):
    """Host PCG64(SeedSequence(seed)) state as (state_hi, state_lo, inc_hi, inc_lo)."""
    lib = load()
    arr = (ctypes.c_uint64 * 4)()
    check(lib, None, lib.he_pcg64_seed_state(ctypes.c_uint64(seed), ctypes.byref(arr)), "he_pcg64_seed_state")
    return tuple(arr)


def host_episode_draws(seed, n_paths, count):
    """Host build of the device episode sampler (PCG64 + Lemire), for tests."""
    import numpy as np
    lib = load()
    out = np.zeros(count, np.int64)
    check(lib, None, lib.he_host_episode_draws(seed, n_paths, count, out.ctypes.data), "he_host_episode_draws")
    return out


def host_philox(seed, env_id, n):
    lib = load()
    arr = (ctypes.c_uint32 * 4)()
    check(lib, None, lib.he_host_philox(seed, env_id, n, ctypes.byref(arr)), "he_host_philox")
    return tuple(arr)


def host_div_by(a, b):
    """Host build of the step kernel's reciprocal-multiply division, for tests."""
    import numpy as np
    lib = load()
    a = np.ascontiguousarray(a, np.float64)
    out = np.empty_like(a)
    check(lib, None, lib.he_host_div_by(a.ctypes.data, a.size, float(b), out.ctypes.data), "he_host_div_by")
    return out


def host_div_byf(a, b):
    """Host build of the obs kernels' f32 reciprocal-multiply division, for tests."""
    import numpy as np
    lib = load()
    a = np.ascontiguousarray(a, np.float32)
    out = np.empty_like(a)
    check(lib, None, lib.he_host_div_byf(a.ctypes.data, a.size, float(b), out.ctypes.data), "he_host_div_byf")
    return out


def host_box_muller(u1, u2):
    """Host build of the generate-mode Box-Muller pair, for tests."""
    import numpy as np
    lib = load()
    u1 = np.ascontiguousarray(u1, np.float64)
    u2 = np.ascontiguousarray(u2, np.float64)
    z1 = np.empty_like(u1)
    z2 = np.empty_like(u1)
    check(lib, None, lib.he_host_box_muller(u1.ctypes.data, u2.ctypes.data, u1.size, z1.ctypes.data, z2.ctypes.data),
          "he_host_box_muller")
    return z1, z2
