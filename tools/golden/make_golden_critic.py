"""Record tests/golden/cr_lossabs_final.npz: the critic of the reference's RecurrentPPO checkpoint
driven over the sequence already in tests/golden/ag_lossabs_final.npz.

    python tools/golden/make_golden_critic.py --reference DIR

Run where the reference checkout is present (the build container); the tests only read the
file.  Numbers only: no reference source text is written anywhere.

  * src/results/lossabs_final/final_model.zip's policy.pth gives the critic's 10 tensors
    (lstm_critic.*, mlp_extractor.value_net.{0,2}.*, value_net.*) and log_std; its `data` gives
    gamma, gae_lambda and n_steps;
  * the fed obs and episode_start are ag_lossabs_final.npz's (300 steps x 16 envs, the boundary at
    step 252 inside), the obs normalised as SB3's VecNormalize does (f64, clipped at +-10, rounded
    to f32): the input of the sb3_* flavour of make_golden_actor.py.

Recorded as f32: values [300,16] and the critic's h [len(H_STEPS),16,128] after the steps H_STEPS
(the actor golden's).  They are computed by torch's own nn.LSTM + nn.Linear + torch.tanh loaded
with those tensors and composed as sb3_contrib's RecurrentActorCriticPolicy.predict_values composes
them (lstm_critic -> mlp_extractor.value_net (tanh) -> value_net), the hidden state zeroed where
episode_start is set as _process_sequence does.  SB3 / sb3_contrib are not installed here, so this
is RESTATED from their source, as the sb3_* flavour of the actor golden is.
"""
import argparse
import io
import json
import os
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CRITIC_KEYS = ("lstm_critic.weight_ih_l0", "lstm_critic.weight_hh_l0", "lstm_critic.bias_ih_l0",
               "lstm_critic.bias_hh_l0", "mlp_extractor.value_net.0.weight", "mlp_extractor.value_net.0.bias",
               "mlp_extractor.value_net.2.weight", "mlp_extractor.value_net.2.bias", "value_net.weight",
               "value_net.bias", "log_std")


def drive(sd, x, start):
    """x [T,N,13] f32 normalised obs, start [T,N] -> values [T,N], h [T,N,128] (f32)."""
    lstm = torch.nn.LSTM(13, 128, num_layers=1, batch_first=True)
    l1, l2, head = torch.nn.Linear(128, 64), torch.nn.Linear(64, 64), torch.nn.Linear(64, 1)
    with torch.no_grad():
        for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            getattr(lstm, name).copy_(sd["lstm_critic." + name])
        for lin, key in ((l1, "mlp_extractor.value_net.0"), (l2, "mlp_extractor.value_net.2"), (head, "value_net")):
            lin.weight.copy_(sd[key + ".weight"])
            lin.bias.copy_(sd[key + ".bias"])
    T, N = start.shape
    h = torch.zeros(1, N, 128)
    c = torch.zeros(1, N, 128)
    vals, hs = [], []
    with torch.no_grad():
        for t in range(T):
            keep = torch.from_numpy(1.0 - start[t].astype(np.float32)).view(1, N, 1)
            h, c = h * keep, c * keep
            out, (h, c) = lstm(torch.from_numpy(x[t]).unsqueeze(1), (h, c))   # (batch, seq = 1, 13)
            v = head(torch.tanh(l2(torch.tanh(l1(out)))))
            vals.append(v[:, 0, 0].numpy().copy())
            hs.append(h[0].numpy().copy())
    return np.stack(vals), np.stack(hs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.environ.get("CANTORRL_REFERENCE"), required="CANTORRL_REFERENCE" not in os.environ,
                    help="the reference checkout (or $CANTORRL_REFERENCE)")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "cr_lossabs_final.npz"))
    a = ap.parse_args()
    torch.manual_seed(0)
    torch.set_num_threads(1)
    with zipfile.ZipFile(os.path.join(a.reference, "src", "results", "lossabs_final", "final_model.zip")) as z:
        sd = torch.load(io.BytesIO(z.read("policy.pth")), map_location="cpu", weights_only=True)
        data = json.loads(z.read("data"))
    if data.get("use_sde"):
        raise SystemExit("the checkpoint uses gSDE: not the policy this golden is for")
    g = np.load(os.path.join(ROOT, "tests", "golden", "ag_lossabs_final.npz"))
    zn = (g["obs"].astype(np.float64) - g["obs_mean"]) / np.sqrt(g["obs_var"] + 1e-8)
    x = np.clip(zn, -10.0, 10.0).astype(np.float32)
    values, h = drive(sd, x, g["episode_start"])
    hsteps = g["h_steps"]
    out = {k.replace(".", "__"): sd[k].numpy() for k in CRITIC_KEYS}
    out.update(values=values.astype(np.float32), critic_h=h[hsteps].astype(np.float32), h_steps=hsteps,
               gamma=np.float64(data["gamma"]), gae_lambda=np.float64(data["gae_lambda"]),
               n_steps=np.int64(data["n_steps"]))
    out["doc"] = np.array(
        "values / critic_h: torch nn.LSTM + nn.Linear + torch.tanh loaded with the checkpoint's critic tensors, "
        "composed as sb3_contrib predict_values (lstm_critic -> value_net MLP (tanh) -> value_net) over "
        "ag_lossabs_final.npz's obs (VecNormalize, clip_obs 10) and episode_start -- RESTATED, SB3 is not "
        "installed; torch " + torch.__version__)
    np.savez_compressed(a.out, **out)
    print("wrote", a.out, os.path.getsize(a.out), "bytes; values", values.min(), values.max())


if __name__ == "__main__":
    main()
