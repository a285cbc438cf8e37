"""What tests/test_occmap_host.py and tests/test_occmap_gpu.py share: the hand-made columns, the rows, the values a row can hold, the
carries the stage must survive, the simulation and the bars."""
import numpy as np

import cfar_f64
import occmap_f64 as om

CHUNK = 64                                  # epochs of a stream that one workgroup of the chunk kernel takes (csrc/crn_segments.h)
LENGTHS = (1, 2, 63, 64, 65, 128, 129, 193)
CUTS = (1, 2, 61, 1, 64, 64)                # of a stream of 193 epochs: one epoch, inside a chunk, up to a chunk edge, whole chunks
N_PATTERNS = 16


def pattern(kind, T, rng):
    """Column pattern `kind` over T epochs, 0 / 1: the cases a join gets wrong when written carelessly sit around t = 64 and 128."""
    t = np.arange(T)
    if kind == 0:
        return 0 * t
    if kind == 1:
        return 0 * t + 1
    if kind == 2:
        return t % 2
    if kind == 3:
        return (t + 1) % 2
    if kind == 4:
        return ((t >= 60) & (t < 70)).astype(int)
    if kind == 5:
        return ((t >= 50) & (t <= 63)).astype(int)          # a busy run that ends exactly on the first chunk's last epoch
    if kind == 6:
        return ((t >= 64) & (t < 80)).astype(int)           # ... that begins exactly on the second chunk's first
    if kind == 7:
        return ((t >= 64) & (t < 128)).astype(int)          # a chunk that is one single run between two idle ones
    if kind == 8:
        return ((t >= 63) & (t < 129)).astype(int)
    if kind == 9:
        return (t % 3 == 0).astype(int)
    if kind == 10:
        return (t % 64 == 0).astype(int)
    if kind == 11:
        return (t % 65 == 0).astype(int)
    if kind in (12, 13, 14):
        return (rng.random(T) < (0.1, 0.5, 0.9)[kind - 12]).astype(int)
    return ((t == 0) | (t == T - 1)).astype(int)            # 15: busy only in the first and in the last epoch


def hand_made(n, S, T, seed=11):
    """det [S T][n] bool: the pattern of bin k in stream j is (k + j) mod 16, so every pattern meets every lane position and tile edge."""
    rng = np.random.default_rng(seed + n + 7 * T)
    det = np.zeros((S, T, n), bool)
    for j in range(S):
        for k in range(n):
            det[j, :, k] = pattern((k + j) % N_PATTERNS, T, rng)
    return det.reshape(S * T, n)


def rows(seed, epochs, n, quantised=False):
    """Gamma(10) rows of mean 1; quantised to quarters (0 included) so that equal values and zeros happen all the time."""
    rng = np.random.default_rng(seed)
    P = rng.gamma(10.0, 0.1, (epochs, n))
    if quantised:
        P = np.round(P * 4.0) / 4.0
    return P.astype(np.float32)


# values a row can hold, one constant column each (and the values in between are ordinary Gamma rows): max_hold and min_hold follow the
# unsigned order of the bit patterns, in which -1.0 (0xbf800000) lies above NaN (0x7fc00000) above +inf above every finite positive
SPECIAL = (0.0, 1e-45, 1e-39, np.inf, np.nan, -1.0)


def special_rows(n, T, seed=5):
    """(P [T][n], the special columns {bin: value}): columns 3, 40, 41, 255, 256 and n - 1 constant at the special values, one epoch of
    column 100 +inf, one of column 101 NaN, and columns 300 and 301 mixing 0.0 and a subnormal."""
    P = rows(seed, T, n)
    where = dict(zip((3, 40, 41, 255, 256, n - 1), SPECIAL))
    for k, v in where.items():
        P[:, k] = np.float32(v)
    P[T // 2, 100] = np.inf
    P[T // 3, 101] = np.nan
    P[::2, 300] = 0.0
    P[1::2, 300] = np.float32(1e-45)
    P[:, 301] = np.float32(1e-40)
    P[T - 1, 301] = 0.0
    return P, where


def carries(n):
    """Records [1][n] to start a call from with first = 0, all of them legal inputs: bins 0..63 all 0xFF bytes; 64..127 n_epochs = -5 and
    the other fields garbage; 128..191 run = -7; 192..255 state = 0x7ffffffe (bit 0 clear) and, odd bins, 0x7fffffff (bit 0 set);
    256..319 n_epochs = n_busy = run = 2^31 - 3 in a busy state; 320..383 the same in an idle state (n_busy 7); the rest all zero."""
    rec = np.zeros((1, n), om.BIN)
    raw = rec.view(np.uint8).reshape(1, n, 64)
    raw[0, :64] = 255
    rng = np.random.default_rng(3)
    raw[0, 64:128] = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    rec["n_epochs"][0, 64:128] = -5
    ok = rec[0, 128:384]
    ok["n_epochs"], ok["n_busy"], ok["n_rise"], ok["n_fall"], ok["run"], ok["state"] = 40, 13, 4, 3, 5, 1
    ok["run_max"] = (9, 6)
    ok["max_hold"], ok["min_hold"] = 3.0, 0.125
    ok["power"] = (20.0, 30.0)
    rec[0, 128:384] = ok
    rec["run"][0, 128:192] = -7
    rec["state"][0, 192:256] = 0x7ffffffe
    rec["state"][0, 193:256:2] = 0x7fffffff
    big = 2 ** 31 - 3
    rec["n_epochs"][0, 256:384] = big
    rec["run"][0, 256:384] = big
    rec["n_busy"][0, 256:320] = big
    rec["n_busy"][0, 320:384] = 7
    rec["state"][0, 320:384] = 0
    return rec


# ---- the simulation ---------------------------------------------------------------------------------------------------------------
# N = 1024 bins, K = 10 frames per epoch, 256 epochs.  The floor falls by 6 dB from the band's middle towards its edges (a receiver's
# pass band); three on-grid carriers 15 dB over the floor of their bin are switched on and off by two-state chains; the mask is the
# project's CA-CFAR twin (guard 2, 16 training cells a side) at Pfa 1e-2.
SIM = {"n": 1024, "k": 10, "rows": 256, "edge_db": 6.0, "carriers": {200: (0.05, 0.10), 512: (0.20, 0.20), 800: (0.02, 0.30)}, "snr_db": 15.0,
       "guard": 2, "train": 16, "pfa": 1e-2}

# Away from the carriers (more than guard + train bins from each) mean_idle is a mean of n_idle draws of floor x Gamma(K) / K: relative
# standard deviation 1 / sqrt(K n_idle).  The bar of the issue: every such bin within 5 / sqrt(K n_idle) of the true floor.  (The idle
# epochs are the ones the CFAR did not flag, so the mean is that of a distribution truncated near its 99th percentile: about 1 % low,
# 0.5 of a standard deviation at 256 rows; the largest of 900 bins lies near 3.4, which leaves a standard deviation of room.)
FLOOR_SIGMAS = 5.0

# The bars below are from the run of tests/test_occmap_host.py::test_simulation with seed 2051, each the run's figure widened by the
# run's own spread.
# duty of a carrier's bin against the on-fraction its chain realised: the run gives + 0.0039, + 0.0039 and + 0.0078, one or two epochs
# of 256 (the false alarms of the off epochs add, a carrier 15 dB up is never missed).  Rule: the three scatter by one epoch, 1 / 256;
# the bar is the largest plus three epochs, and one epoch below zero.
DUTY_RANGE = (-1 / 256, 5 / 256)
# mean_idle of the carriers' CFAR neighbourhood (within guard + train bins, the carrier's own bin left out) against the true floor, in
# standard deviations 1 / sqrt(K n_idle): the run's largest is 2.90 over 108 bins, their root mean square 1.16 (1 is what pure noise
# gives: the neighbourhood's threshold rises while the carrier is on, which lowers the false alarms there, not the idle mean).  Rule:
# the largest plus two of the run's root mean square.
NEIGH_SIGMAS = 5.2
# mean_idle of a carrier's own bin over the true floor of that bin: 0.992, 1.001, 0.970 in the run (the idle epochs are the off epochs,
# less their false alarms), a scatter of 0.016.  Rule: the run's range widened by three times its scatter on either side.
CARRIER_IDLE_RANGE = (0.92, 1.05)
# The busy power sum of a carrier's bin, power[1] / rows, over what the carrier put there, on-fraction x (1 + 10^1.5) x floor: 0.998,
# 0.987, 1.056 in the run (mean_busy itself is diluted by the false alarms of the off epochs, 27.6 x floor for the carrier that is on
# in 3 % of the rows against 31.9 for the one on in 47 %; the sum is not).  Rule: the range widened by three times its scatter, 0.03.
CARRIER_BUSY_RANGE = (0.90, 1.15)


def floor_shape(n, edge_db):
    x = (np.arange(n) - n / 2) / (n / 2)
    return 10.0 ** (-edge_db * x * x / 10.0)


def simulate(seed, alpha, sim=SIM):
    """(P [rows][n] float32, det [rows][n] bool, floor [n], on {bin: [rows] bool}): alpha is crn_cfar_alpha(pfa, k, train)."""
    n, k, R = sim["n"], sim["k"], sim["rows"]
    rng = np.random.default_rng(seed)
    floor = floor_shape(n, sim["edge_db"])
    P = floor[None, :] * rng.gamma(float(k), 1.0 / k, (R, n))
    on = {}
    for b, (p01, p10) in sim["carriers"].items():
        st = np.zeros(R, bool)
        cur = bool(rng.random() < p01 / (p01 + p10))
        for t in range(R):
            cur = (rng.random() >= p10) if cur else (rng.random() < p01)
            st[t] = cur
        noise = rng.normal(0, np.sqrt(0.5), (R, k)) + 1j * rng.normal(0, np.sqrt(0.5), (R, k))
        lit = floor[b] * (np.abs(10.0 ** (sim["snr_db"] / 20.0) + noise) ** 2).mean(axis=1)
        P[:, b] = np.where(st, lit, P[:, b])
        on[b] = st
    P = P.astype(np.float32)
    det = cfar_f64.ratio(P, sim["guard"], sim["train"], alpha) > 1.0
    return P, det, floor, on


def neighbourhood(sim=SIM):
    """(bins away from every carrier, the carriers' CFAR neighbourhoods without the carriers' own bins)."""
    n, reach = sim["n"], sim["guard"] + sim["train"]
    near = np.zeros(n, bool)
    for b in sim["carriers"]:
        near[(b + np.arange(-reach, reach + 1)) % n] = True
    own = np.zeros(n, bool)
    own[list(sim["carriers"])] = True
    return ~near, near & ~own


# ---- end to end with the generator (tests/test_occmap_gpu.py::test_end_to_end_with_the_generator) -----------------------------------
E2E = {"n": 1024, "k": 10, "epochs": 600, "seed": 2052, "noise_power": 1e-6, "signal_rms": 0.02, "pfa": 1e-2}
# duty of a channel's carrier bin less the fraction of the 600 epochs in which d_truth names the channel, from the GPU run recorded in
# profiles/r19_occmap.txt: + 0.0133, + 0.0133 and + 0.0100 for CH1, CH2 and CH3 (named in 0.1200, 0.3250 and 0.5550 of the epochs), that
# is 8, 8 and 6 epochs: the false alarms of the epochs in which the channel is off (Pfa 1e-2 of 270 to 530 of them), and no carrier missed.
# Rule: the three scatter by two epochs; the bar is the largest plus three times that, 14 epochs, and two epochs below zero.
E2E_DUTY_RANGE = (-2 / 600, 14 / 600)
