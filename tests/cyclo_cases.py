"""Inputs the tests of crn_cyclo_device share (tests/test_cyclo_host.py, tests/test_cyclo_gpu.py): a root-raised-cosine QPSK carrier at an
off-grid symbol rate over white noise, cut into frames and transformed; the chain whose answer is known in closed form; the records a
kernel must survive; and the tolerances of the GPU comparison, derived here once.  A plain module, not collected."""
import numpy as np

import cyclo_f64 as cf

SEGMENT_DTYPE = [("lo", "<i4"), ("width", "<i4"), ("peak_bin", "<i4"), ("n_detected", "<i4"),
                 ("power", "<f4"), ("peak_power", "<f4"), ("centroid", "<f4"), ("reserved", "<f4")]
SEGMENT_EPOCH_DTYPE = [("n_found", "<i4"), ("n_stored", "<i4"), ("noise_bins", "<i4"), ("noise_mean", "<f4")]

ROLLOFF = 0.35


def rrc(t, beta=ROLLOFF):
    """The root-raised-cosine pulse at t symbols from its centre (unit symbol period)."""
    t = np.asarray(t, np.float64)
    at = np.abs(t)
    sing0, sing1 = at < 1e-9, np.abs(at - 1.0 / (4.0 * beta)) < 1e-9
    ts = np.where(sing0 | sing1, 0.3, t)                                   # any regular point; replaced below
    h = (np.sin(np.pi * ts * (1 - beta)) + 4 * beta * ts * np.cos(np.pi * ts * (1 + beta))) / (np.pi * ts * (1 - (4 * beta * ts) ** 2))
    h = np.where(sing0, 1 - beta + 4 * beta / np.pi, h)
    return np.where(sing1, beta / np.sqrt(2) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * beta)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * beta))), h)


def qpsk_spectra(rng, n, frames, epochs, rate_bins, centre_bin, snr_db, reach=8):
    """[epochs][frames][n] complex64: the DFTs of consecutive disjoint frames of unit white noise plus an RRC-QPSK carrier of rate_bins
    symbols per n samples around centre_bin, snr_db over the noise inside its band.  The pulse is summed over +- reach symbols."""
    L = epochs * frames * n
    sps = n / rate_bins
    t = np.arange(L) / sps
    m0 = np.floor(t).astype(np.int64)
    sym = (rng.integers(0, 2, (m0[-1] + 2 * reach + 2, 2)) * 2 - 1) @ np.array([1.0, 1j]) / np.sqrt(2)
    x = np.zeros(L, np.complex128)
    for d in range(-reach, reach + 1):
        x += sym[m0 + d + reach] * rrc(t - (m0 + d))
    x *= np.exp(2j * np.pi * centre_bin / n * np.arange(L))
    x *= np.sqrt(10 ** (snr_db / 10) * rate_bins / n / np.mean(np.abs(x) ** 2))        # in-band: the carrier's power lies in rate_bins of n bins
    x += (rng.standard_normal(L) + 1j * rng.standard_normal(L)) / np.sqrt(2)
    return np.fft.fft(x.reshape(epochs, frames, n), axis=2).astype(np.complex64)


def noise_spectra(rng, n, frames, epochs):
    x = (rng.standard_normal((epochs, frames, n)) + 1j * rng.standard_normal((epochs, frames, n))) / np.sqrt(2)
    return np.fft.fft(x, axis=2).astype(np.complex64)


def chain(rng, n, frames, lo, width, q0):
    """[frames][n] complex64 noise with X_f[lo + i] = u_i e^(j 2 pi q0 i f / F), |u_i| in 0.5 .. 2, on the span: S(a, q) = 1 where
    q = q0 a mod F and 0 elsewhere."""
    X = noise_spectra(rng, n, frames, 1)[0]
    u = rng.uniform(0.5, 2.0, width) * np.exp(2j * np.pi * rng.uniform(0, 1, width))
    f = np.arange(frames)[:, None]
    i = np.arange(width)[None, :]
    X[:, (lo + np.arange(width)) % n] = (u[None, :] * np.exp(2j * np.pi * q0 * i * f / frames)).astype(np.complex64)
    return X


def records(E, max_segments, segs):
    """(heads, recs) with segs = {epoch: [(lo, width), ...]}; slots beyond n_stored hold 0xFF bytes."""
    heads = np.zeros(E, np.dtype(SEGMENT_EPOCH_DTYPE))
    recs = np.frombuffer(b"\xff" * (E * max_segments * 32), np.dtype(SEGMENT_DTYPE)).reshape(E, max_segments).copy()
    for e, lst in segs.items():
        heads[e] = (len(lst), len(lst), 0, 1.0)
        for s, (lo, width) in enumerate(lst):
            recs[e, s] = (lo, width, lo, width, 1.0, 1.0, 0.0, 0.0)
    return heads, recs


def s_bound(frames):
    """|S - S_twin| allowed on the device, absolute: P and C are fp32 sums of F terms and rho <= 1."""
    return 8.0 * frames * 2.0 ** -24


def z_bound(frames, n_pairs):
    """... and of z: the same times F sqrt(n_pairs (F + 1) / (F - 1)), dz / dS."""
    return s_bound(frames) * frames * cf.z_scale(frames, n_pairs)
