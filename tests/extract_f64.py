"""crn_extract_device in float64, written from the definition in include/crn_sense.h ("extraction: a detected emitter as a baseband
sample stream") and from nothing else: kappa = centre mod N, the taper product rounded to fp32, the M-point inverse DFT as a plain sum,
the middle half of every block, the sign by the parity of kappa (t0 + t), zeros for a channel without a stream.  Also the bound of the
GPU comparison and the inputs the host and GPU tests share.  A plain module, not collected."""
import numpy as np

EXTRACT_CHANNEL_DTYPE = [("stream", "<i4"), ("centre", "<i4"), ("reserved", "<i4", (2,))]
OUT_LENS = (16, 32, 64, 128, 256)


def gamma(out_len):
    """The header's gamma: 5 u for each of the log2(M) butterfly levels and 4 u for the product between the two passes."""
    return 5 * int(np.log2(out_len)) + 4


def tapered(X, kappa, taper):
    """Z [frames][M] complex128 of step 1: both components of the fp32 product rounded to fp32; X [frames][N] complex64."""
    n, m = X.shape[1], taper.size
    k = (kappa + np.arange(m) - m // 2) % n
    x = np.ascontiguousarray(X[:, k], np.complex64)
    h = taper.astype(np.float32)[None, :]
    return (x.real * h).astype(np.float32).astype(np.float64) + 1j * (x.imag * h).astype(np.float32).astype(np.float64)


def run(X, channels, taper, out_len, frames_per_stream, t0=0, want_scale=False):
    """X [n_frames][N] complex64; channels EXTRACT_CHANNEL_DTYPE [n_chan]; taper float32 [M].  Returns out [n_chan][F M / 2] complex128
    and, if asked, scale [n_chan][F M / 2] = (sum over i of |Z[i]|) / N of the block each sample came from."""
    X = np.asarray(X)
    n_frames, n = X.shape
    m, F = int(out_len), int(frames_per_stream)
    assert X.dtype == np.complex64 and m in OUT_LENS and m <= n // 2 and taper.size == m and n_frames % F == 0
    S = n_frames // F
    out = np.zeros((len(channels), F * m // 2), np.complex128)
    scale = np.zeros((len(channels), F * m // 2), np.float64)
    i = np.arange(m) - m // 2
    nn = np.arange(m // 4, 3 * m // 4)
    E = np.exp(2j * np.pi * np.outer(i, nn) / m)                         # [M][M / 2]
    t = np.arange(F)
    for c, ch in enumerate(channels):
        stream = int(ch["stream"])
        if not 0 <= stream < S:
            continue
        kappa = int(ch["centre"]) % n
        Z = tapered(X[stream * F:(stream + 1) * F], kappa, taper)        # [F][M]
        y = (Z @ E) / n
        sign = np.where((kappa * (int(t0) + t)) % 2 == 1, -1.0, 1.0)
        out[c] = (y * sign[:, None]).reshape(-1)
        scale[c] = np.repeat(np.abs(Z).sum(axis=1) / n, m // 2)
    return (out, scale) if want_scale else out


def bound(scale, out_len):
    """|y - y_twin| allowed per sample on the device: gamma 2^-24 (sum |Z|) / N."""
    return gamma(out_len) * 2.0 ** -24 * scale


def taper(out_len, flat):
    """The definition of crnsense.extract_taper once more, for the tests that run the twin alone."""
    m = int(out_len)
    i = np.abs(np.arange(m, dtype=np.float64) - m // 2)
    h = np.where(i <= flat, 1.0, 0.5 * (1.0 + np.cos(np.pi * (i - flat) / (m // 2 - flat))))
    h[0] = 0.0
    return h.astype(np.float32)


def spectra(x, n):
    """[F][n] complex64: the unnormalised DFTs of the half-overlapped frames of the record x (F = len(x) / (n / 2) - 1), what
    crn_fft_forward_device writes for samples_per_frame = n, frame_stride = n / 2."""
    F = len(x) // (n // 2) - 1
    fr = np.stack([x[t * n // 2: t * n // 2 + n] for t in range(F)])
    return np.fft.fft(fr, axis=1).astype(np.complex64)


def sample_times(n_out, n, out_len):
    """The input sample at which output sample u sits: (u + M / 4) N / M."""
    return (np.arange(n_out) + out_len // 4) * (n // out_len)


def channel_records(pairs):
    """EXTRACT_CHANNEL_DTYPE records from (stream, centre) pairs; the reserved words hold 0xFF bytes: they are not looked at."""
    out = np.zeros(len(pairs), np.dtype(EXTRACT_CHANNEL_DTYPE))
    for c, (s, k) in enumerate(pairs):
        out[c] = (np.int64(s).astype(np.int32), np.int64(k).astype(np.int32), (-1, -1))
    return out


def noise_spectra(rng, n_frames, n):
    """Random fp32 spectra (not the DFT of anything half-overlapped: the stage does not care)."""
    return ((rng.standard_normal((n_frames, n)) + 1j * rng.standard_normal((n_frames, n))) * np.sqrt(n / 2)).astype(np.complex64)
