"""The option cases of tests/test_rbergomi_replay_gpu.py, shared with the CPU test that
proves the GPU comparison is sensitive to a wrong draw layout for each of them
(tests/test_rbergomi_replay_cpu.py).  NumPy and the oracle only."""
import os

import numpy as np

from oracle import rbergomi_oracle as orc

import _rbergomi_replay as rep

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
R, DT = orc.R, orc.DT
OFF = 2 ** 32 - 2            # gid crosses the 32-bit word inside every launch
SEED = 2 ** 32 + 7           # hi(seed) != 0
KINDS = ("call", "put")      # sub = type: call 0, put 1

# Tolerances of the marks.  f64 normals: the file-wide tolerance of tests/test_rbergomi_gpu.py
# (same draws, different libm): mc_box_muller is within 1e-13 r_max = 8.6e-13 absolute of the
# f64 formula, which over n <= 63 steps moves log S by at most 63 sqrt(v dt) 8.6e-13 < 2e-12,
# and the payoff is 1-Lipschitz in S.
MARK_RTOL = 1e-10
MARK_ATOL_S0 = 1e-10         # atol = MARK_ATOL_S0 * max(S0)
# f32 normals: the device evaluates log2 / sqrt / sin / cos with the f32 hardware
# instructions, whose error the guides do not state, so the bound is measured: the largest
# |device - replay| / S0 over every f32 list-mode case below, on an MI355X, times 8.
F32_MEASURED_REL = 8.282e-9  # measured 8.28126e-09 (n = 30, n_mc = 1, put); the run is deterministic
F32_BOUND_REL = 8 * F32_MEASURED_REL
F32_CEILING_REL = 1e-4       # the bound may not exceed this

# n = int(T / dt) Euler steps -> option grid M_opt = next_pow2(n + 1):
#   1 -> 2; 2, 3 -> 4; 5, 6, 7 -> 8; 15 -> 16; 30 (the compile-time-guard variant), 31 -> 32;
#   32, 63 -> 64.  n = M - 1 at 1, 3, 7, 15, 31, 63; n < kXc = 6 at 1..5, n = kXc at 6, n not
#   a multiple of kXc everywhere but 6 and 30; odd n (the Im W pair of the last step half used).
MC_STEPS = (1, 2, 3, 5, 6, 7, 15, 30, 31, 32, 63)
# MC paths per option over 256 threads: one thread, a partial wave, thread 0 running two
# paths, an uneven tail
MC_PATHS = (1, 3, 257, 600)

# Four options: at, in and out of the money for both types.  Options 2 and 3 (gid >= 2^32)
# are in the money for a call and a put respectively, so a dropped hi(gid) shows in either type
# even with one MC path; xi of 0.04-0.16 keeps a one-step move well above every tolerance.
S0 = np.array([100.0, 80.0, 100.0, 496.48])
K = np.array([100.0, 82.0, 70.0, 700.0])
XI = np.array([0.09, 0.16, 0.09, 0.0625])
H = np.array([0.01, 0.49, 0.05, 0.1])
ETA = np.array([1.9, 1.0, 2.5, 2.2])
RHO = np.array([-0.7, -0.99, -0.01, -0.4])
# test_pricer_edge_inputs_follow_reference's rows (S0 <= 0, xi < 0, NaN, S0 below the floor,
# xi = 0); none of them depends on the draws, so they ride behind the four above
EDGE = dict(S0=np.array([0.0, -5.0, 100.0, np.nan, 1e-9, 50.0]), K=np.array([1.0, 1.0, 100.0, 100.0, 0.0, 50.0]),
            xi=np.array([0.04, 0.04, -0.01, 0.04, 0.04, 0.0]), H=np.full(6, 0.2), eta=np.full(6, 1.5),
            rho=np.full(6, -0.5))


def tenor(n):
    """(n + 1/2) dt: int(T / dt) = n without a rounding question."""
    return (n + 0.5) * DT


class Case:
    """One launch of the MC pricer per option type: inputs, draw coordinates, tolerance."""

    def __init__(self, name, n, n_mc, S0, K, xi, H, eta, rho, gid, sub0, T, n_draw_rows=None):
        self.name, self.n, self.n_mc, self.T = name, n, n_mc, T
        self.M = max(2, orc.next_pow2(n + 1))
        self.S0, self.K, self.xi, self.H, self.eta, self.rho = (np.asarray(x, np.float64) for x in
                                                                (S0, K, xi, H, eta, rho))
        self.gid = np.asarray(gid, np.uint64)
        self.sub0 = np.asarray(sub0, np.uint64)          # sub of a call; a put's is sub0 + 1
        self.rows = len(self.S0) if n_draw_rows is None else n_draw_rows   # rows held to the f32 bound

    def W(self, kind, normals, perturb=None):
        return rep.mc_W(SEED, self.gid, self.sub0 + np.uint64(KINDS.index(kind)), self.n_mc, self.M, normals,
                        n=self.n, perturb=perturb)

    def oracle(self, kind, W):
        with np.errstate(invalid="ignore"):
            return orc.price_options(self.S0, self.K, self.T, R, self.xi, self.H, self.eta, self.rho, kind,
                                     rep.w_to_z(W), DT)

    def tol(self, normals, ref):
        """Absolute tolerance per mark."""
        t = MARK_ATOL_S0 * np.nanmax(self.S0) + MARK_RTOL * np.abs(ref)
        if normals == "f32":
            t[:self.rows] = F32_BOUND_REL * self.S0[:self.rows]
        return t

    def check(self, kind, normals, got, ref):
        err = np.abs(got - ref)
        bad = ~(err <= self.tol(normals, ref)) & ~(np.isnan(got) & np.isnan(ref))
        assert not bad.any(), (self.name, kind, normals, got, ref, err)


def list_case(n, n_mc, edge=False):
    cols = [S0, K, XI, H, ETA, RHO]
    if edge:
        cols = [np.concatenate([a, EDGE[k]]) for a, k in zip(cols, ("S0", "K", "xi", "H", "eta", "rho"))]
    B = len(cols[0])
    return Case(f"list n={n} n_mc={n_mc}" + (" edge" if edge else ""), n, n_mc, *cols,
                gid=[OFF + i for i in range(B)], sub0=np.zeros(B, np.uint64), T=tenor(n), n_draw_rows=4)


def list_cases():
    return [list_case(n, n_mc) for n in MC_STEPS for n_mc in MC_PATHS] + [list_case(3, 3, edge=True)]


# ------------------------------------------------------------------ ATM marks
ATM_SMALL = dict(n_steps=5, n_mc=5, option_tenor=3.5 * DT)
ATM_DEFAULT = dict(n_steps=orc.N_STEPS, n_mc=2, option_tenor=orc.T_OPTION_TENOR)
ATM_PATHS = 3


def history():
    return np.load(os.path.join(GOLD, "rb_estimate.npz"))["hist__prices"]


def atm_case(name, params, paths, vol, n_steps, n_mc, option_tenor):
    """Day d of path p, flattened to option p n_steps + d: S0 = paths[p, d], xi = vol[p, d],
    K = round(S0), the path's H, eta, rho; gid = OFF + p, sub = 2 d + type."""
    P = paths.shape[0]
    p, d = np.divmod(np.arange(P * n_steps), n_steps)
    s = paths[p, d]
    return Case(name, int(option_tenor / DT), n_mc, s, np.round(s), vol[p, d], params[2][p], params[3][p],
                params[4][p], gid=[OFF + int(i) for i in p], sub0=(2 * d).astype(np.uint64), T=option_tenor)


def host_generate(base, n_steps):
    """params, paths, vol of ATM_PATHS paths from the replayed draws through the oracle."""
    unit = rep.unit_normals(SEED, OFF, ATM_PATHS)
    params = np.stack(orc.perturb_params(base, [s * u for s, u in zip(orc.PERTURB_STD, unit)]))
    M = orc.next_pow2(n_steps + 1)
    paths, vol = orc.simulate_paths(*params, rep.w_to_z(rep.main_W(SEED, OFF, ATM_PATHS, M)), R, DT, n_steps)
    return params, paths, vol
