"""cantorrl_amd: MI355X-native batched dynamic-hedging environment.

The hot path of bcosm/CantorRL (`HedgingEnv.step`, src/env/hedging_env_v2.py)
as HIP kernels behind a C ABI (include/hedge_env.h, libhedgeenv.so), with the
reference's Python interface on top:

* `HedgingVecEnv` -- N envs on one GPU, SB3 VecEnv interface (vec_env.py)
* `HedgingEnv`    -- the single-env gym API with the reference ctor (env.py)
* `RecurrentActor` -- a RecurrentPPO checkpoint's actor as one HIP kernel (agent.py,
  include/hedge_actor.h, libhedgeactor.so), `HedgingVecEnv.evaluate_actor` around it
* `RecurrentPolicy`, `RolloutCollector` -- actor + critic + sampling + log-prob per step in one
  kernel and GAE: RecurrentPPO's collect_rollouts on the device (agent.py, collect.py)
* `lstm_sequence`, `lstm_sequence_pair`, `RecurrentPPOModule`, `ppo_update` -- the LSTM over a stored
  sequence with per-step resets as a differentiable op (one forward and one backward kernel for actor
  and critic), evaluate_actions and RecurrentPPO.train's loss on top of it (train.py)
* `DeviceAdam` -- the gradient-norm clip and Adam's step over all parameters in two launches
  (train.py); `RecurrentPolicy.load_device_state_dict` re-packs the policy from device tensors in one
  launch (agent.py): a training iteration without a host round trip
* `ppo_loss_kernel` -- RecurrentPPO.train's loss, its statistics and its gradients with respect to
  values, log_prob and entropy as kernels with an arithmetic contract (train.py, ha_ppo_loss)
* `ppo_heads`, `ppo_heads_forward`, `ppo_heads_backward`, `heads_weight_grads` -- the part of
  evaluate_actions after the LSTMs (MLPs, action and value heads, log-probability, entropy) and its
  backward down to the LSTMs' outputs as kernels under the step kernel's contract (train.py,
  ha_ppo_heads_forward / _backward); `RecurrentPPOModule(heads="kernel")` routes through it
"""
__version__ = "0.1.0"


def __getattr__(name):
    if name == "HedgingVecEnv":
        from .vec_env import HedgingVecEnv
        return HedgingVecEnv
    if name == "HedgingEnv":
        from .env import HedgingEnv
        return HedgingEnv
    if name == "RecurrentActor":
        from .agent import RecurrentActor
        return RecurrentActor
    if name == "RecurrentPolicy":
        from .agent import RecurrentPolicy
        return RecurrentPolicy
    if name == "RolloutCollector":
        from .collect import RolloutCollector
        return RolloutCollector
    if name in ("lstm_sequence", "lstm_sequence_pair", "RecurrentPPOModule", "ppo_update", "DeviceAdam",
                "ppo_loss_kernel", "ppo_heads", "ppo_heads_forward", "ppo_heads_backward", "heads_weight_grads"):
        from . import train
        return getattr(train, name)
    raise AttributeError(name)
