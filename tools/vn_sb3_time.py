"""Device time of a DeviceVecNormalize step (step_tensors, info=False, no Monitor) in both moments
modes, training and evaluation, at small env counts: HIP events around windows of steps, warmed.

    python tools/vn_sb3_time.py [--modes f64,sb3] [--ns 2,256,4096] [--steps 2000] [--windows 7]
                                [--tree DIR] [--label NAME] [--out FILE]
    python tools/vn_sb3_time.py --summarize FILE [FILE ...]

One JSON line per (mode, phase, n): the median over the windows of the mean step time of a window,
and the windows' min / max.  --tree imports cantorrl_amd from another checkout (a build of the
parent commit, which has the default mode only: --modes f64), so that two commits are timed by
the same script, alternating, in one session.  --summarize reads the lines of several runs and
prints, per (label, mode, phase, n), the median of the runs' medians and their spread (max - min).
"""
import argparse
import json
import os
import statistics
import sys

KW = dict(loss_type="abs", pnl_penalty_weight=0.001, lambda_cost=0.0001, theta_weight=0.0002, slippage_bps=1.0)
GEN = dict(s0=496.48001098632812, variance=0.029028, mu=0.04, dt=1 / 252, episode_length=252)


def summarize(files):
    rows = {}
    for f in files:
        with open(f) as fh:
            for line in fh:
                line = line.strip()
                if line.startswith("{"):
                    r = json.loads(line)
                    rows.setdefault((r["label"], r["mode"], r["phase"], r["n"]), []).append(r["median_us"])
    print(f"{'label':10s} {'mode':4s} {'phase':6s} {'n':>5s} {'runs':>4s} {'median us':>10s} {'spread us':>10s}")
    for (label, mode, phase, n), v in sorted(rows.items(), key=lambda kv: (kv[0][3], kv[0][2], kv[0][1], kv[0][0])):
        print(f"{label:10s} {mode:4s} {phase:6s} {n:5d} {len(v):4d} {statistics.median(v):10.2f} {max(v) - min(v):10.2f}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="f64,sb3")
    ap.add_argument("--ns", default="2,256,4096")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="this")
    ap.add_argument("--out")
    ap.add_argument("--summarize", nargs="+")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    from cantorrl_amd.vec_env import HedgingVecEnv
    from cantorrl_amd.vec_normalize import DeviceVecNormalize
    if not torch.cuda.is_available():
        raise SystemExit("vn_sb3_time.py needs the GPU: nothing is timed without one")
    out = open(args.out, "a") if args.out else None
    for n in (int(x) for x in args.ns.split(",")):
        acts = torch.rand((n, 2), device="cuda") * 2 - 1
        for mode in args.modes.split(","):
            for phase in ("train", "eval"):
                env = HedgingVecEnv(n, mode="gbm", generate=GEN, seed=42, return_numpy=False, info_keys=(), **KW)
                kw = {} if mode == "f64" else dict(moments=mode)   # the parent commit has no such keyword
                vn = DeviceVecNormalize(env, gamma=0.99, **kw)
                vn.reset_tensors()
                for _ in range(200):   # statistics worth normalizing by; code objects loaded
                    vn.step_tensors(acts, info=False)
                if phase == "eval":
                    vn.training, vn.norm_reward = False, False
                    for _ in range(200):
                        vn.step_tensors(acts, info=False)
                torch.cuda.synchronize()
                per = []
                for _ in range(args.windows):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.steps):
                        vn.step_tensors(acts, info=False)
                    b.record()
                    torch.cuda.synchronize()
                    per.append(a.elapsed_time(b) / args.steps * 1e3)
                rec = dict(label=args.label, mode=mode, phase=phase, n=n, steps=args.steps, windows=args.windows,
                           median_us=round(statistics.median(per), 3), min_us=round(min(per), 3),
                           max_us=round(max(per), 3))
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
                vn.close()
    if out:
        out.close()


if __name__ == "__main__":
    main()
