"""What the hop-count tests share (tests/test_hops_host.py, tests/test_hops_gpu.py): the constants of the end-to-end chain, which are
those of test_end_to_end_markov_chain in tests/test_channels_gpu.py (copied: a test file is not imported), the primary user's table, the
busy words of the grid, and the simulated users of the host test.  A plain module, not collected."""
import numpy as np

# N = 512, K = 10, 4 streams of 500 epochs, CRN_SIG_TONES with 8 tones per band, CA-CFAR guard 2 / train 16 at Pfa 1e-3, min_bins 3;
# channel c is band c of the energy plan as one circular interval (channel 0 is the reference band, which nobody drives)
E2E = {"n": 512, "k": 10, "n_streams": 4, "eps": 500, "pfa": 1e-3, "min_bins": 3, "seed": 2031, "noise_power": 1e-6, "signal_rms": 0.02,
       "tones": 8, "spans": [(300, 10), (496, 32), (55, 30), (189, 33)], "guard": 2, "train": 16}

# CRN_PU_MARKOV_INTENDED: row = the channel the user is on (CH1, CH2, CH3), column = the one it is on an epoch later
TABLE = np.array([[0.1, 0.3, 0.6], [0.1, 0.5, 0.4], [0.1, 0.3, 0.6]])

EPS = (1, 2, 63, 64, 65, 129, 193)
LAG_SETS = ((1,), (1, 2, 64), (1, 2, 3, 5, 8, 13, 63, 64))
CHANNELS = (1, 3, 63)
WORD_KINDS = ("chain", "d0.05", "d0.5", "d0.95", "zero", "high")


def jump_table(table):
    """A table without its diagonal, rows renormalised: where the user goes when it leaves."""
    t = np.array(table, float)
    np.fill_diagonal(t, 0.0)
    return t / t.sum(axis=1, keepdims=True)


def words(kind, E, C, rng):
    """E busy words of one kind for C channels, uint64: a chain with one bit per word that stays, moves or goes idle; random words at a
    bit density; all zero; random words with bits at and above C and bit 63 set as well (which the stage must ignore)."""
    if kind == "chain":
        pos = np.cumsum(rng.integers(-1, 2, E) * (rng.random(E) < 0.4)) % (C + 1)         # C: nothing busy
        return np.where(pos == C, np.uint64(0), np.uint64(1) << pos.astype(np.uint64)).astype(np.uint64)
    if kind == "zero":
        return np.zeros(E, np.uint64)
    dens = 0.3 if kind == "high" else float(kind[1:])
    w = np.zeros(E, np.uint64)
    for c in range(64 if kind == "high" else C):
        w |= (rng.random(E) < dens).astype(np.uint64) << np.uint64(c)
    if kind == "high":
        w |= np.uint64(1) << np.uint64(63)
        w[::3] &= ~np.uint64((1 << C) - 1)                                                  # ... and nothing below C in every third
    return w


def dwelling_user(rng, table, n_jumps, dwell, flicker):
    """The busy words of a user on len(table) channels that stays `dwell` epochs on a channel and then jumps by jump_table(table); a
    share `flicker` of the epochs shows nothing busy.  Returns (words, the number of jumps out of each channel)."""
    jt = jump_table(table)
    C = len(jt)
    at, seq, left = 0, [], np.zeros(C, int)
    for _ in range(n_jumps):
        seq += [at] * dwell
        left[at] += 1
        at = int(rng.choice(C, p=jt[at]))
    seq = np.array(seq + [at] * dwell, np.uint64)
    w = np.uint64(1) << seq
    w[rng.random(w.size) < flicker] = 0
    return w.astype(np.uint64), left


def sweep(n_channels, n_epochs):
    """The interferer's sweep over n_channels channels, one per epoch: 0, 1, .., n - 1, n - 2, .., 1, 0, 1, ..: the channel of each epoch."""
    period = list(range(n_channels)) + list(range(n_channels - 2, 0, -1))
    return np.array([period[t % len(period)] for t in range(n_epochs)])
