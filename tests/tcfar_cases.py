"""What tests/test_tcfar_host.py and tests/test_tcfar_gpu.py share: the receiver of the simulation (a floor that is not flat, a fixed spur,
a DC spike), its traffic, the bars both tests assert, and the rows the GPU test feeds the kernel."""
import numpy as np

N, K = 512, 10
CELLS, GUARD, RANK, PFA = 64, 1, 16, 1e-3
SPUR_BIN, SPUR_GAIN, DC_BIN, DC_GAIN = 100, 100.0, 0, 30.0
CHANNELS = ((150, 30), (250, 33), (350, 120))        # (lo, width): the widths of the reference's transmitters at N = 512, and a wide one

# the bars (DESIGN.md §5 quotes what the twin gives)
FA_LO, FA_HI = 1e-3 / 1.5, 1e-3 * 1.5                # noise only, over at least 4e5 decisions
SHARE_6DB, SHARE_10DB = 0.9, 0.99                    # share of the driven channel's bins set
SPUR_BAR = 0.01                                      # share of the epochs in which the spur bin is set
LAD_FALSE_BAR = 0.2                                  # LAD with one block: share of the idle bins it sets on the same rows


def gain(n=N):
    """The receiver's gain per bin: 1 + 0.75 cos(2 pi k / n) (8.5 dB across the row), x100 at the spur, x30 at DC."""
    g = 1.0 + 0.75 * np.cos(2.0 * np.pi * np.arange(n) / n)
    g[SPUR_BIN] *= SPUR_GAIN
    g[DC_BIN] *= DC_GAIN
    return g


def channel_bins(n=N):
    """[4, n] bool: row c the bins of channel c, row 0 (idle) empty."""
    chan = np.zeros((4, n), bool)
    for c, (lo, w) in enumerate(CHANNELS, start=1):
        chan[c, (lo + np.arange(w)) % n] = True
    return chan


def simulate(rng, epochs, db, n=N, k=K):
    """(rows [epochs, n] float32, pick [epochs] in 0..3): Gamma(k) noise of mean 1, in every epoch one of idle / channel 1 / 2 / 3 drawn
    uniformly, the driven channel's bins carrying an emitter `db` dB over the noise (db None: noise only); all of it through gain()."""
    P = rng.gamma(float(k), 1.0 / k, (epochs, n))
    pick = rng.integers(0, 4, epochs) if db is not None else np.zeros(epochs, np.int64)
    if db is not None:
        driven = channel_bins(n)[pick]
        P[driven] += 10.0 ** (db / 10.0) * rng.gamma(float(k), 1.0 / k, int(driven.sum()))
    return (P * gain(n)[None, :]).astype(np.float32), pick


def shares(mask, pick, n=N, skip=0):
    """(share of the driven channel's bins set, share of the bins outside every channel set, spur excluded and DC excluded, share of the
    epochs with the spur bin set, with the DC bin set) over the epochs from `skip` on."""
    chan = channel_bins(n)
    m, driven = mask[skip:], chan[pick[skip:]]
    idle = ~chan.any(axis=0)
    idle[[SPUR_BIN, DC_BIN]] = False
    hit = m[driven].mean() if driven.any() else float("nan")
    return hit, m[:, idle].mean(), m[:, SPUR_BIN].mean(), m[:, DC_BIN].mean()


def gamma_rows(seed, epochs, n, quantised=False):
    """Rows for the GPU test: Gamma(10) noise of mean 1; quantised to quarters (never 0) so that fl32(2 c) == P happens all the time."""
    rng = np.random.default_rng(seed)
    P = rng.gamma(10.0, 0.1, (epochs, n))
    if quantised:
        P = np.maximum(np.round(P * 4.0), 1.0) / 4.0
    return P.astype(np.float32)
