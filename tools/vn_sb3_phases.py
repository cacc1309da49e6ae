"""Where vn_sb3_kernel's time goes: he_vecnorm_step alone, back to back on fixed inputs (so
GPU-bound), in three settings, with the default mode's two launches beside it:
  train               the full training step;
  train_no_norm_obs   no obs chain and the obs copied: the returns' part and the fixed cost;
  frozen              frozen statistics: the apply alone.

    python tools/vn_sb3_phases.py [OUT.jsonl]
"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from cantorrl_amd.vec_env import HedgingVecEnv  # noqa: E402
from cantorrl_amd.vec_normalize import DeviceVecNormalize  # noqa: E402

KW = dict(loss_type="abs", pnl_penalty_weight=0.001, lambda_cost=0.0001, theta_weight=0.0002, slippage_bps=1.0)
GEN = dict(s0=496.48001098632812, variance=0.029028, mu=0.04, dt=1 / 252, episode_length=252)
out = open(sys.argv[1], "w") if len(sys.argv) > 1 else None
for n in (2, 256, 1024, 4096):
    env = HedgingVecEnv(n, mode="gbm", generate=GEN, seed=42, return_numpy=False, info_keys=(), **KW)
    acts = torch.rand((n, 2), device="cuda") * 2 - 1
    for mode in ("sb3", "f64"):
        for name, kw in (("train", {}), ("train_no_norm_obs", dict(norm_obs=False)),
                         ("frozen", dict(training=False, norm_reward=False))):
            vn = DeviceVecNormalize(env, gamma=0.99, moments=mode, **kw)
            vn.reset_tensors()
            env.step_tensors(acts)
            c = vn._call_args()
            call = lambda: vn.lib.he_vecnorm_step(c[2], n, *c[3], vn._stream())  # noqa: E731
            for _ in range(300):
                assert call() == 0
            torch.cuda.synchronize()
            per = []
            for _ in range(5):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(1000):
                    call()
                b.record()
                torch.cuda.synchronize()
                per.append(a.elapsed_time(b))
            rec = dict(n=n, mode=mode, setting=name, us_per_call=round(statistics.median(per), 3))
            print(json.dumps(rec), flush=True)
            if out:
                out.write(json.dumps(rec) + "\n")
    env.close()
