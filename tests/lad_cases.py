"""The synthetic rows that tests/test_lad_gpu.py feeds crn_lad_device, kept apart so that tests/test_lad_host.py can check on the CPU
what the GPU test relies on: that the twin (tests/lad_f64.py) calls every one of them decided.  Noise is Gamma(K) with mean 1e-4."""
import numpy as np

import lad_f64 as lf

SIZES = (512, 1024, 2048, 4096)
E_MAX = 65
INIT_PERCENTS = (1, 10, 50)
MEAN = 1e-4


def blocks_allowed(n):
    return [b for b in (1, 2, 4, 8) if n // b >= 256]


def params(k=10, pfa_cme=1e-2, pfa_lower=1e-2, pfa_upper=1e-4):
    """The factors of the issue's double threshold for K-frame noise, as the twin computes them."""
    t = lf.factor(pfa_cme, k)
    return {"t_cme": t, "t_lower": lf.factor(pfa_lower, k, t), "t_upper": lf.factor(pfa_upper, k, t)}


def _noise(rng, n, k):
    return rng.gamma(float(k), MEAN / k, n)


def _emitter(rng, n, bins, db, k=10):
    """Gamma(K) noise with a flat emitter `db` dB over it on `bins` (taken mod n)."""
    p = _noise(rng, n, k)
    idx = np.asarray(bins) % n
    p[idx] += MEAN * 10.0 ** (db / 10.0) * rng.gamma(float(k), 1.0 / k, idx.size)
    return p


# levels of the designed cluster rows over a quiet floor of 0.9 .. 1.1 MEAN: with params(10) the lower threshold lies near 1.9 MEAN and
# the upper one near 2.65 MEAN
LOW, HIGH = 2.2 * MEAN, 10.0 * MEAN


def _quiet(rng, n):
    return rng.uniform(0.9, 1.1, n) * MEAN


def _clusters_on_edges(rng, n, shift):
    """Runs of five bins over the lower threshold, one end bin of each over the upper one: that bin is the first or the last of a lane
    piece, of a mask word and of the row."""
    b = n // 64
    p = _quiet(rng, n)
    piece, word = (7 + shift) % 60 + 1, (3 + shift) % (n // 32 - 2) + 1
    for k, step in ((piece * b, 1), (piece * b + 3 * b - 1, -1), (word * 32 + n // 2, 1), (word * 32 + 31 + n // 4, -1), (0, 1), (n - 1, -1)):
        run = (k + step * np.arange(5)) % n
        if (p[run] > 1.5 * MEAN).any():                     # keep the runs apart: a run that would touch an earlier one is left out
            continue
        p[run] = LOW
        p[k % n] = HIGH
    return p


def _rejected_beside_kept(rng, n, shift):
    """A run without an upper bin one bin away from a run with one, inside a piece and across pieces; runs over three pieces whose only
    upper bin is in the first, the middle (a piece of ones) and the last of them, and one such run without any."""
    b = n // 64
    p = _quiet(rng, n)
    a = (5 + shift) % 8 * b + 1
    p[a: a + 3] = LOW                                         # rejected
    p[a + 4: a + 7] = LOW                                     # kept: one-bin gap at a + 3
    p[a + 5] = HIGH
    a = (12 + shift % 4) * b - 4                              # the same across a piece edge, the gap on the edge's last bin
    p[a: a + 3] = LOW
    p[a + 4: a + 9] = LOW
    p[a + 8] = HIGH
    for j, where in enumerate((0, 1, 2, None)):
        lo = (20 + 8 * j + shift % 3) * b + b // 2            # from the middle of a piece over the next one into the middle of the third
        p[lo: lo + 2 * b] = LOW
        if where is not None:
            p[lo + (0, b, 2 * b - 1)[where]] = HIGH
    lo = n - b - 2                                            # across the wrap, the upper bin beyond it
    p[lo:] = LOW
    p[:3] = LOW
    p[1] = HIGH
    return p


def batch(n, seed=0):
    """([E_MAX, n] float32, the kind of every row).  Every kind the issue lists comes up several times, at other places and seeds."""
    rng = np.random.default_rng(1000 * n + seed)
    b = n // 64
    kinds = [
        ("noise K=1", lambda i: _noise(rng, n, 1)),
        ("noise K=10", lambda i: _noise(rng, n, 10)),
        ("emitter inside a lane piece", lambda i: _emitter(rng, n, ((5 + i) % 64) * b + 1 + np.arange(b - 2), 10)),
        ("emitter on piece edges", lambda i: _emitter(rng, n, ((9 + i) % 60) * b + np.arange(2 * b), 10)),
        ("emitter over piece edges", lambda i: _emitter(rng, n, ((13 + i) % 60) * b - 1 + np.arange(b + 2), 6)),
        ("emitter across a block edge", lambda i: _emitter(rng, n, n // 2 - 20 - i % 7 + np.arange(37), 10)),
        ("emitter across the wrap", lambda i: _emitter(rng, n, n - 11 - i % 5 + np.arange(25), 10)),
        ("emitter over 90 % of the row", lambda i: _emitter(rng, n, i * 3 + np.arange(n * 9 // 10), 10)),
        ("all equal", lambda i: np.full(n, 3.0 * MEAN)),
        ("all zero", lambda i: np.zeros(n)),
        ("one bin 90 dB over the floor", lambda i: _emitter(rng, n, [((3 + i) % 64) * b], 90)),
        ("ties at the pivot", lambda i: rng.integers(1, 6, n) * MEAN),
        ("clusters on edges", lambda i: _clusters_on_edges(rng, n, i)),
        ("rejected beside kept", lambda i: _rejected_beside_kept(rng, n, i)),
    ]
    rows, names = [], []
    for i in range(E_MAX):
        name, make = kinds[i % len(kinds)]
        rows.append(make(i))
        names.append(name)
    return np.asarray(rows, np.float64).astype(np.float32), names
