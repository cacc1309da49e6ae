"""Record tests/golden/ag_lossabs_final.npz: the reference's own RecurrentPPO actor driven over
the env golden tests/golden/g1_v2_train.npz.

    python tools/golden/make_golden_actor.py [--reference DIR]

Run where the reference checkout is present (the build container); the tests only read the
file.  Numbers only: no reference source text is written anywhere.

  * quantconnect/model_wrapper.py is imported unmodified, with an empty in-memory stub standing
    in for the QuantConnect `AlgorithmImports` module;
  * src/results/lossabs_final/final_model.zip's policy.pth is loaded through the reference's own
    key mapping (ModelWrapper.LoadSB3Weights, model_wrapper.py:77-110);
  * the statistics are quantconnect/model_files/normalization_stats.pkl;
  * the fed obs are the env golden's reset_obs followed by obs[:-1] (300 steps x 16 envs),
    episode_start is ones followed by terminated[:-1] (the boundary at step 252 is inside).

Two flavours are recorded, each as the f32 actions [300,16,2] per step and h [len(H_STEPS),16,128]
after the steps H_STEPS (every step's h would be 2.4 MB a flavour; the committed file stays under
1 MB, and h at step 299 carries every earlier step's error):
  ref_*  reference-literal: the reference module's forward (ReLU MLP, tanh squash), the obs
         normalised without a clip as ModelWrapper.predict does (model_wrapper.py:131,148);
  sb3_*  SB3's predict(deterministic=True): the SAME submodules composed with torch.tanh in the
         MLP (SB3's default activation_fn), obs clipped at +-10, action = clip(mean, -1, 1), and the
         pre-clip mean.  SB3 / sb3_contrib are not installed here, so this flavour is RESTATED
         from their source, as the VecNormalize goldens are.
The hidden state is zeroed where episode_start is set, as SB3's _process_sequence does.
"""
import argparse
import io
import os
import pickle
import sys
import types
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ACTOR_KEYS = ("lstm_actor.weight_ih_l0", "lstm_actor.weight_hh_l0", "lstm_actor.bias_ih_l0", "lstm_actor.bias_hh_l0",
              "mlp_extractor.policy_net.0.weight", "mlp_extractor.policy_net.0.bias",
              "mlp_extractor.policy_net.2.weight", "mlp_extractor.policy_net.2.bias",
              "action_net.weight", "action_net.bias", "log_std")


H_STEPS = (0, 1, 2, 100, 200, 250, 251, 252, 253, 299)   # 252: the first step of the second episode


class _Log:
    def Log(self, msg):
        pass


def load_reference_model(ref):
    sys.modules.setdefault("AlgorithmImports", types.ModuleType("AlgorithmImports"))
    sys.path.insert(0, os.path.join(ref, "quantconnect"))
    import model_wrapper as mw
    with zipfile.ZipFile(os.path.join(ref, "src", "results", "lossabs_final", "final_model.zip")) as z:
        sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
    wrap = mw.ModelWrapper.__new__(mw.ModelWrapper)   # no ObjectStore here: skip LoadModel
    wrap.algorithm = _Log()
    wrap.model = mw.RecurrentPPOModel(obs_dim=13, action_dim=2, lstm_hidden_size=128)
    wrap.LoadSB3Weights(sd)
    return wrap.model, sd


def drive(model, x, start, flavour):
    """x [T,N,13] f32 normalised obs, start [T,N] bool -> actions, mean, h per step (f32)."""
    T, N = start.shape
    h = torch.zeros(1, N, 128)
    c = torch.zeros(1, N, 128)
    acts, means, hs = [], [], []
    with torch.no_grad():
        for t in range(T):
            keep = torch.from_numpy(1.0 - start[t].astype(np.float32)).view(1, N, 1)
            h, c = h * keep, c * keep
            xt = torch.from_numpy(x[t]).unsqueeze(1)   # (batch, seq = 1, 13)
            if flavour == "ref":
                a, (h, c) = model(xt, (h, c))
                mean = torch.full_like(a, float("nan"))
            else:
                out, (h, c) = model.lstm_actor(xt, (h, c))
                net = model.mlp_extractor_policy_net
                mean = model.action_net(torch.tanh(net[2](torch.tanh(net[0](out)))))
                a = torch.clamp(mean, -1.0, 1.0)
            acts.append(a[:, 0].numpy().copy())
            means.append(mean[:, 0].numpy().copy())
            hs.append(h[0].numpy().copy())
    return np.stack(acts), np.stack(means), np.stack(hs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CANTORRL_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "ag_lossabs_final.npz"))
    a = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(1)
    model, sd = load_reference_model(a.reference)
    with open(os.path.join(a.reference, "quantconnect", "model_files", "normalization_stats.pkl"), "rb") as f:
        ns = pickle.load(f)
    mean = np.asarray(ns["obs_mean"], np.float64)
    var = np.asarray(ns["obs_var"], np.float64)
    g = np.load(os.path.join(ROOT, "tests", "golden", "g1_v2_train.npz"))
    obs = np.concatenate([g["reset_obs"][None], g["obs"][:-1]]).astype(np.float32)
    start = np.concatenate([np.ones((1, obs.shape[1]), bool), g["terminated"][:-1]])
    z = (obs - mean) / np.sqrt(var + 1e-8)   # model_wrapper.py:131 (f64)
    out = {k.replace(".", "__"): sd[k].numpy() for k in ACTOR_KEYS}
    out.update(obs_mean=mean, obs_var=var, obs=obs, episode_start=start.astype(np.uint8))
    ra, _, rh = drive(model, z.astype(np.float32), start, "ref")
    sa, sm, sh = drive(model, np.clip(z, -10.0, 10.0).astype(np.float32), start, "sb3")
    out.update(ref_actions=np.clip(ra, -1, 1), ref_h=rh[list(H_STEPS)], sb3_actions=sa, sb3_mean=sm,
               sb3_h=sh[list(H_STEPS)], h_steps=np.array(H_STEPS, np.int64))
    out["doc"] = np.array(
        "ref_*: reference module (model_wrapper.py RecurrentPPOModel, relu MLP, tanh squash, obs not clipped); "
        "sb3_*: the same submodules composed as SB3 predict(deterministic=True) (tanh MLP, clip_obs 10, "
        "clip(mean)) -- RESTATED, SB3 is not installed; torch " + torch.__version__)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes; boundary steps:", np.nonzero(start.any(1))[0])


if __name__ == "__main__":
    main()
