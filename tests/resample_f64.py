"""crn_resample_device in float64, written from the definition in include/crn_sense.h ("resampling: an extracted stream at k samples
per symbol") and from nothing else: the count, the positions and the carry in Python integers, the interpolated coefficient, the T-term
sum and the mixer in float64.  Also the bound of the GPU comparison and the helpers the host and GPU tests share.  A plain module, not
collected."""
import numpy as np

ROW_DTYPE = [("step", "<u8"), ("dphi", "<i4"), ("reserved", "<i4")]
STATE_DTYPE = [("pos", "<u8"), ("phase", "<u4"), ("taps", "<i4"), ("n_in", "<i8"), ("n_out", "<i8"), ("n_dropped", "<i8"),
               ("last_n_out", "<i4"), ("reserved", "<i4", (5,)), ("hist", "<c8", (32,))]
TAPS = (8, 16, 32)
PHASES = (32, 64, 128, 256)
STEP_MIN, STEP_MAX = 2 ** 30, 2 ** 34


def gamma(taps):
    """The header's gamma: 3 u for the coefficient, T u for the sum, 5.7 u for the mixer factor, 2.4 u for the complex product."""
    return int(taps) + 12


def count(pos, step, in_len):
    """Step 1 in Python integers."""
    L = int(in_len) << 32
    return 0 if pos >= L else (L - 1 - pos) // step + 1


def table(taps, phases, cutoff, beta):
    """The definition of crnsense.resample_taps once more, for the tests that run the twin alone.  Written from the same sentence of the
    header, so that the two agree byte for byte shows little; that the table is RIGHT shows in tests/test_resample_host.py: the multitone
    and alias figures it gives (within 1 % of an independent prototype's), row P being row 0 one tap on, the sum P and the peak at T / 2."""
    T, P = int(taps), int(phases)
    t = np.arange(T, dtype=np.float64)[None, :] - T // 2 + np.arange(P + 1, dtype=np.float64)[:, None] / P
    inside = np.abs(t) < T / 2
    w = np.i0(beta * np.sqrt(np.where(inside, 1 - (2 * t / T) ** 2, 0.0))) / np.i0(beta)
    g = np.where(inside, 2 * cutoff * np.sinc(2 * cutoff * t) * w, 0.0)
    return (g * (P / g[:P].sum())).astype(np.float32)


def rows(steps, dphis=0):
    """ROW_DTYPE records from steps (any 64-bit value) and increments (any int32 value); the reserved word holds 0xFF bytes."""
    steps = [int(s) for s in (steps if hasattr(steps, "__len__") else [steps])]      # not through numpy: 2^64 - 1 must stay an integer
    dphis = [int(d) for d in np.broadcast_to(np.atleast_1d(dphis), (len(steps),))]
    out = np.zeros(len(steps), np.dtype(ROW_DTYPE))
    for i, (s, d) in enumerate(zip(steps, dphis)):
        out[i] = (s, d, -1)
    return out


def states(n_rows, fill=0):
    """n_rows states, every byte `fill`."""
    return np.frombuffer(bytes([fill]) * (320 * n_rows), np.dtype(STATE_DTYPE)).copy()


def run(x, rws, h, state, out_cap, first=False, want_scale=False):
    """x [n_rows][in_len] complex64; rws ROW_DTYPE [n_rows]; h float32 [P + 1][T]; state STATE_DTYPE [n_rows], left as it is.  Returns
    (out [n_rows][out_cap] complex128, the new states) and, if asked, scale [n_rows][out_cap] = sum over k of max(|h[phi][k]|,
    |h[phi + 1][k]|) |x[j - k]| of every output (0 where none is)."""
    x = np.asarray(x)
    n_rows, in_len = x.shape
    T, P = h.shape[1], h.shape[0] - 1
    assert x.dtype == np.complex64 and h.dtype == np.float32 and T in TAPS and P in PHASES and len(rws) == n_rows == len(state)
    s = 32 - int(np.log2(P))
    h64 = h.astype(np.float64)
    L = in_len << 32
    out = np.zeros((n_rows, out_cap), np.complex128)
    scale = np.zeros((n_rows, out_cap), np.float64)
    new = state.copy()
    kk = np.arange(T)
    for r in range(n_rows):
        step, dphi = int(rws["step"][r]), int(rws["dphi"][r])
        if not STEP_MIN <= step <= STEP_MAX:
            new["last_n_out"][r] = 0
            continue
        st = state[r]
        empty = bool(first) or int(st["taps"]) != T
        pos = 0 if empty else int(st["pos"])
        phase = 0 if empty else int(st["phase"])
        hist = np.zeros(T - 1, np.complex128) if empty else st["hist"][: T - 1].astype(np.complex128)
        cnt = [0 if empty else max(int(st[name]), 0) for name in ("n_in", "n_out", "n_dropped")]
        n = count(pos, step, in_len)
        w = min(n, out_cap)
        xx = np.concatenate([hist, x[r].astype(np.complex128)])          # xx[T - 1 + i] = x[i]
        if w:
            p = [pos + u * step for u in range(w)]
            assert p[-1] < L
            j = np.array([q >> 32 for q in p], np.int64)
            f = [q & (2 ** 32 - 1) for q in p]
            phi = np.array([q >> s for q in f], np.int64)
            mu = np.array([(q & (2 ** s - 1)) >> max(s - 24, 0) for q in f], np.float64) * 2.0 ** -min(s, 24)
            X = xx[j[:, None] + (T - 1) - kk[None, :]]                   # [w][T]: x[j - k]
            h0, h1 = h64[phi], h64[phi + 1]
            y = (((1 - mu)[:, None] * h0 + mu[:, None] * h1) * X).sum(axis=1)
            theta = np.array([(phase + u * dphi) % 2 ** 32 for u in range(w)], np.float64)
            out[r, :w] = y * np.exp(2j * np.pi * theta / 2.0 ** 32)
            scale[r, :w] = (np.maximum(np.abs(h0), np.abs(h1)) * np.abs(X)).sum(axis=1)
        wrap = lambda v: (v + 2 ** 63) % 2 ** 64 - 2 ** 63      # noqa: E731
        new["pos"][r] = (pos + n * step - L) % 2 ** 64
        new["phase"][r] = (phase + n * dphi) % 2 ** 32
        new["taps"][r] = T
        new["n_in"][r], new["n_out"][r], new["n_dropped"][r] = wrap(cnt[0] + in_len), wrap(cnt[1] + w), wrap(cnt[2] + n - w)
        new["last_n_out"][r] = w
        new["reserved"][r] = 0
        new["hist"][r] = 0
        new["hist"][r][: T - 1] = xx[len(xx) - (T - 1):].astype(np.complex64)
    return (out, new, scale) if want_scale else (out, new)


def bound(scale, taps):
    """|z - z_twin| allowed per output on the device: gamma 2^-24 sum max(|h[phi][k]|, |h[phi + 1][k]|) |x[j - k]|."""
    return gamma(taps) * 2.0 ** -24 * scale


def tones(b, times, amps=(1, .5, .25, .5, 1)):
    """The five tones of the host test at the given times (in input samples): frequencies -b, -0.37 b, 0.011, 0.53 b, b cycles per
    sample, phases 0 .. 4 rad."""
    fr = (-b, -0.37 * b, 0.011, 0.53 * b, b)
    t = np.asarray(times, np.float64)
    return sum(a * np.exp(1j * (2 * np.pi * f * t + ph)) for a, f, ph in zip(amps, fr, range(5)))
