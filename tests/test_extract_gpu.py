"""crn_extract_device on the MI355X: the kernel against the twin (tests/extract_f64.py) fed the kernel's own fp32 spectra and taper,
every sample within gamma 2^-24 (sum |Z|) / N of it (gamma = 5 log2 M + 4, include/crn_sense.h); zero rows, the sign rule, cut
invariance, a repeated call and the 0xFF behind every array exact.  Then every refusal, the generator's RRC-QPSK carrier end to end, and
the cost next to the transform that feeds the stage."""
import ctypes as C

import numpy as np
import pytest

import crnsense as cs
import extract_f64 as xf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402


def _upload(a):
    """A structured array's bytes on the device."""
    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(DEV)


def _spectra(X):
    """[n_frames][N] complex64 -> interleaved float32 on the device."""
    return torch.from_numpy(np.ascontiguousarray(X, np.complex64).view(np.float32)).to(DEV)


def _extract(s, X, ch, h, m, F, t0=0):
    """One call on host arrays: ([n_chan][F M / 2] complex64 as the device wrote it, its bytes); the guard bytes are checked."""
    x_t, ch_t, h_t = _spectra(X), _upload(ch), torch.from_numpy(h).to(DEV)
    out = sgpu.Padded(out=len(ch) * F * (m // 2) * 8)
    s.extract_device(x_t.data_ptr(), X.shape[0], cs.extract_params(m, F, t0), ch_t.data_ptr(), len(ch), h_t.data_ptr(), out.out.data_ptr())
    out.host()
    assert out.pads_untouched(), "memory behind the output was written"
    return out.view("out", np.complex64, (len(ch), F * (m // 2))), out.raw["out"].tobytes()


def _channels(rng, n, m, S, n_chan):
    """The records of a case: centres 0, N - 1, N / 2, one whose window crosses the wrap, an even and an odd centre, two channels on one
    centre; streams -1, S and 2^31 - 1 (zero rows); centres -3, N + 17, 2^31 - 1, -2^31 next to their residues; then random ones."""
    st = lambda i: i % S      # noqa: E731
    fixed = [(0, 0), (st(1), n - 1), (st(2), n // 2), (0, n - m // 4), (st(1), 100), (st(2), 101), (0, 77), (0, 77),
             (-1, 5), (S, 5), (2 ** 31 - 1, 5),
             (st(1), -3), (st(1), n - 3), (st(2), n + 17), (st(2), 17), (0, 2 ** 31 - 1), (0, n - 1), (st(1), -2 ** 31), (st(1), 0)]
    pairs = fixed[:n_chan]
    while len(pairs) < n_chan:
        pairs.append((int(rng.integers(0, S)), int(rng.integers(0, n))))
    return xf.channel_records(pairs), pairs


SHARE = {}


def _against_twin(y, X, ch, h, m, F, t0, what):
    """Every sample within the bound; rows of channels without a stream are zero bytes.  Returns the largest share of the bound used."""
    want, scale = xf.run(X, ch, h, m, F, t0, want_scale=True)
    b = xf.bound(scale, m)
    err = np.abs(y.astype(np.complex128) - want)
    assert np.isfinite(y.view(np.float32)).all(), what
    assert (err <= b).all(), (what, float((err / np.where(b > 0, b, 1)).max()))
    S = X.shape[0] // F
    for c in range(len(ch)):
        if not 0 <= int(ch["stream"][c]) < S:
            assert not y[c].tobytes().strip(b"\0"), (what, c)
    return float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


@pytest.mark.parametrize("n,m", [(512, 16), (512, 64), (512, 256), (4096, 16), (4096, 64), (4096, 256), (512, 32), (4096, 128)])
def test_kernel_against_twin(built, n, m):
    """Per (fft_len, out_len): one stream of one frame with one channel, a taper of ones; three streams of two frames with 37 channels,
    extract_taper; three streams of seven frames with 37 channels under extract_taper, the spectra as they are, scaled by 1e12 and by
    1e-14, with the stream also cut 3 + 4, the call repeated, the other parity of t0 (odd centres negated bit for bit, even ones the
    same), a taper of ones and a taper of zeros; one stream of seven frames with one channel; the one-bin spectrum's closed form."""
    s = cs.Sensor(sgpu.cfg(n))
    rng = np.random.default_rng(n + m)
    flat = m // 4
    h, ones, zeros = cs.extract_taper(m, flat), np.ones(m, np.float32), np.zeros(m, np.float32)
    share = 0.0
    for S, F, n_chan, taper in ((1, 1, 1, ones), (3, 2, 37, h), (1, 7, 1, h)):
        X = xf.noise_spectra(rng, S * F, n)
        ch, _ = _channels(rng, n, m, S, n_chan)
        y, _ = _extract(s, X, ch, taper, m, F)
        share = max(share, _against_twin(y, X, ch, taper, m, F, 0, (n, m, S, F, n_chan)))
    S, F, n_chan = 3, 7, 37
    X0 = xf.noise_spectra(rng, S * F, n)
    ch, pairs = _channels(rng, n, m, S, n_chan)
    odd = np.array([0 <= st < S and (k % n) % 2 == 1 for st, k in pairs])
    live = np.array([0 <= st < S for st, _ in pairs])
    assert odd.sum() >= 5 and (live & ~odd).sum() >= 5 and (~live).sum() == 3
    for scale in (1.0, 1e12, 1e-14):
        what = (n, m, S, F, n_chan, scale)
        X = (X0 * np.float32(scale)).astype(np.complex64)
        y, raw = _extract(s, X, ch, h, m, F)
        share = max(share, _against_twin(y, X, ch, h, m, F, 0, what))
        assert np.abs(y[live]).min() > 0, what
        # hostile centres behave as their residues; two channels on one centre give one row twice
        for a, b in ((11, 12), (13, 14), (15, 16), (17, 18), (6, 7)):
            assert y[a].tobytes() == y[b].tobytes(), (what, a, b)
        # the same call again: the same bytes
        assert _extract(s, X, ch, h, m, F)[1] == raw, what
        # the stream cut 3 + 4: frames 0 .. 2 of every stream, then 3 .. 6 with t0 = 3
        Xs = X.reshape(S, F, n)
        ya, _ = _extract(s, Xs[:, :3].reshape(-1, n), ch, h, m, 3)
        yb, _ = _extract(s, Xs[:, 3:].reshape(-1, n), ch, h, m, 4, t0=3)
        assert np.concatenate([ya, yb], axis=1).tobytes() == raw, what
        # the other parity of t0: every odd centre negated bit for bit, every even one unchanged, zero rows still zero bytes
        y1, _ = _extract(s, X, ch, h, m, F, t0=1)
        assert (-y1[odd]).tobytes() == y[odd].tobytes() and y1[~odd].tobytes() == y[~odd].tobytes(), what
        y2, raw2 = _extract(s, X, ch, h, m, F, t0=2 ** 31 - 2)
        assert raw2 == raw, what
    y, _ = _extract(s, X0, ch, ones, m, F)
    share = max(share, _against_twin(y, X0, ch, ones, m, F, 0, (n, m, "ones")))
    y, _ = _extract(s, X0, ch, zeros, m, F)
    assert (y == 0).all(), (n, m, "a taper of zeros")
    # one bin: X_t[k0] = N comes out as H[k0 - kappa] e^(j 2 pi (k0 - kappa) n / M) (-1)^(kappa (t0 + t)), here for an even and an odd
    # kappa, both parities of t0, k0 on either side of the wrap
    X1 = np.zeros((2, n), np.complex64)
    X1[:, 2] = n
    cen = [n - 3, n - 2, 2, 7]
    for t0 in (0, 1):
        y, _ = _extract(s, X1, xf.channel_records([(0, k) for k in cen]), h, m, 2, t0=t0)
        for c, kappa in enumerate(cen):
            d = (2 - kappa + n // 2) % n - n // 2
            for t in range(2):
                want = h[d + m // 2] * np.exp(2j * np.pi * d * np.arange(m // 4, 3 * m // 4) / m) * (-1) ** (kappa * (t0 + t))
                got = y[c].reshape(2, m // 2)[t].astype(np.complex128)
                assert np.abs(got - want).max() <= xf.gamma(m) * 2.0 ** -24 * float(h[d + m // 2]), (n, m, kappa, t0, t)
    s.close()
    SHARE[(n, m)] = share
    print(f"N={n} M={m}: largest |y - y_twin| is {100 * share:.1f} % of the bound (gamma = {xf.gamma(m)})")


def test_refusals_with_a_live_handle(built):
    """Every refusal of the header's list; a refused call, n_frames = 0 and n_chan = 0 leave the output as it was."""
    n, m, S, F, n_chan = 512, 64, 2, 3, 4
    L = cs.lib()
    s = cs.Sensor(sgpu.cfg(n))
    rng = np.random.default_rng(1)
    X = xf.noise_spectra(rng, S * F, n)
    ch = xf.channel_records([(0, 10), (1, 100), (0, 301), (1, 511)])
    h = cs.extract_taper(m, 16)
    x_t, ch_t, h_t = _spectra(X), _upload(ch), torch.from_numpy(np.concatenate([h, h])).to(DEV)
    out = sgpu.Padded(out=n_chan * F * (m // 2) * 8)

    def rc(sp=x_t.data_ptr(), n_f=S * F, q=None, chp=ch_t.data_ptr(), nc=n_chan, tp=h_t.data_ptr(), op=out.out.data_ptr(), hd=s._h,
           out_len=m, fps=F, t0=0, reserved=(0, 0, 0, 0, 0)):
        if q is None:
            q = cs.extract_params(out_len, fps, t0)
            for i, x in enumerate(reserved):
                q.reserved[i] = x
        v = lambda p: C.c_void_p(p or None)      # noqa: E731
        return L.crn_extract_device(hd, v(sp), n_f, C.byref(q) if q != 0 else None, v(chp), nc, v(tp), v(op), None)
    assert rc() == 0
    before = out.host()["out"].copy()
    assert out.pads_untouched() and np.abs(out.view("out", np.complex64)).min() > 0
    out.out[: before.size] = 255
    for bad in ({"hd": None}, {"sp": 0}, {"q": 0}, {"chp": 0}, {"tp": 0}, {"op": 0},
                {"out_len": 0}, {"out_len": 8}, {"out_len": 48}, {"out_len": 512}, {"out_len": -64}, {"out_len": 65},
                {"fps": 0}, {"fps": -1}, {"fps": 4}, {"fps": 5}, {"fps": 7}, {"t0": -1}, {"t0": -2 ** 31},
                {"nc": -1}, {"nc": 65537}, {"n_f": -1}, {"n_f": -6},
                {"reserved": (1, 0, 0, 0, 0)}, {"reserved": (0, 0, 0, 0, -1)}, {"reserved": (0, 0, 7, 0, 0)},
                {"sp": x_t.data_ptr() + 8}, {"chp": ch_t.data_ptr() + 8}, {"tp": h_t.data_ptr() + 4}, {"tp": h_t.data_ptr() + 8},
                {"op": out.out.data_ptr() + 8}):
        assert rc(**bad) == cs.CRN_ERR_ARG, bad
        assert b"crn_extract_device" in L.crn_last_error(), bad
    # (out_len above fft_len / 2 has no case: the smallest plan has 512 points and the longest block 256)
    assert rc(n_f=0) == 0 and rc(nc=0) == 0 and rc(n_f=0, nc=0) == 0
    assert (out.host()["out"] == 255).all() and out.pads_untouched()
    # the ends of the ranges are accepted
    assert rc(t0=2 ** 31 - 1) == 0 and rc(fps=1) == 0 and rc(fps=2) == 0 and rc(out_len=16) == 0 and rc(tp=h_t.data_ptr() + 16) == 0
    assert rc() == 0
    assert out.host()["out"].tobytes() == before.tobytes() and out.pads_untouched()
    s.close()


# The generator's carrier end to end, as in tests/test_cyclo_gpu.py: RRC-QPSK at the default levels on the 60-bin channel.
E2E = {"n": 1024, "frames": 8, "epochs": 32, "seed": 2051, "noise_power": 1e-6, "signal_rms": 0.02, "channel": 2, "out_len": 128, "flat": 40}


def test_end_to_end_the_generators_carrier_as_a_stream(built):
    """crn_synth_fill_device_ex, RRC-QPSK at the default levels, a uniform pick among idle and the three channels per epoch of 8 frames,
    N = 1024; crn_fft_forward_device with stride N / 2 over the whole buffer, so that an epoch is a stream of 16 half-overlapped frames
    (the last reaches into the next epoch and is left out below); extraction at the centre of the 60-bin channel and at an idle place,
    M = 128, flat 40.  Both streams are within the bound of the twin.  In the epochs that drive the channel the carrier's stream must
    exceed the idle one in mean power by the generator's in-band SNR less a margin: the passband holds sum H^2 bins of noise, not the
    channel's 60, so the ratio falls short of the in-band SNR by 10 log10(sum H^2 / 60) = 2.4 dB; the margin is the twin's own shortfall
    on the same spectra (a reference value, not the kernel's) plus 0.05 dB, and that shortfall must itself be within 0.5 dB of 2.4."""
    n, K, E, m, flat = E2E["n"], E2E["frames"], E2E["epochs"], E2E["out_len"], E2E["flat"]
    cfg = sgpu.cfg(n, k=K)
    chan = {}
    for g in cfg.segs[: cfg.n_segs]:
        if g.band != 0:
            chan.setdefault(g.band, []).extend(range(g.lo, g.hi))
    bins = chan[E2E["channel"]]
    nb = len(bins)
    assert nb == 60 and cs.samples_per_epoch(cfg) == K * n
    centre = (bins[0] + bins[-1] + 1) // 2
    taken = np.zeros(n, bool)
    for b in chan.values():
        taken[np.array(b) % n] = True
    free = [k for k in range(m, n - m) if not taken[k - m // 2 - 8: k + m // 2 + 8].any()]
    idle = max(free, key=lambda k: min(abs(k - centre), n - abs(k - centre)))      # the free place farthest from the carrier
    F = 2 * K                                                      # frames of a stream
    iq_t = sgpu.zeros(((E * K * n + n // 2) * 2,), torch.float32)   # half a frame of zeros behind the last epoch
    truth_t = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    sc = cs.SynthCfg()
    sc.seed, sc.noise_power, sc.signal_rms = E2E["seed"], E2E["noise_power"], E2E["signal_rms"]
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = 0, cs.PU_UNIFORM, cs.SIG_RRC_QPSK, 1
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), E, K * n, sc, truth_ptr=truth_t.data_ptr())
    x_t = sgpu.zeros((E * F * n * 2,), torch.float32)
    s.fft_forward_device(iq_t.data_ptr(), E * F, n, x_t.data_ptr(), frame_stride=n // 2)
    ch = xf.channel_records([(e, k) for e in range(E) for k in (centre, idle)])
    h = cs.extract_taper(m, flat)
    ch_t, h_t = _upload(ch), torch.from_numpy(h).to(DEV)
    out = sgpu.Padded(out=len(ch) * F * (m // 2) * 8)
    s.extract_device(x_t.data_ptr(), E * F, cs.extract_params(m, F), ch_t.data_ptr(), len(ch), h_t.data_ptr(), out.out.data_ptr())
    out.host()
    assert out.pads_untouched()
    y = out.view("out", np.complex64, (E, 2, F, m // 2))
    X = x_t.cpu().numpy().view(np.complex64).reshape(E * F, n)
    truth = truth_t.cpu().numpy()
    s.close()
    want, scale = xf.run(X, ch, h, m, F, want_scale=True)
    err = np.abs(y.reshape(len(ch), -1).astype(np.complex128) - want)
    b = xf.bound(scale, m)
    assert (err <= b).all(), float((err / b).max())
    driven = np.flatnonzero(truth == E2E["channel"])
    assert len(driven) >= 4

    def power(a):
        """Mean power of the carrier's and of the idle stream over the driven epochs, the frame that reaches into the next epoch left out."""
        return np.mean(np.abs(a.astype(np.complex128)[driven][:, :, : F - 1]) ** 2, axis=(0, 2, 3))
    pc, pi = power(y)
    tc, ti = power(want.reshape(E, 2, F, m // 2))
    snr_db = 10 * np.log10(E2E["signal_rms"] ** 2 / (E2E["noise_power"] * nb / n))
    got_db, twin_db = 10 * np.log10(pc / pi), 10 * np.log10(tc / ti)
    short = 10 * np.log10(float((h.astype(np.float64) ** 2).sum()) / nb)
    margin = (snr_db - twin_db) + 0.05
    print(f"channel {E2E['channel']} centre {centre}, idle place {idle}; {len(driven)} driven epochs of {E}; in-band SNR {snr_db:.2f} dB; carrier / idle stream "
          f"{got_db:.3f} dB on the device, {twin_db:.3f} dB in the twin; shortfall {snr_db - twin_db:.3f} dB (sum H^2 / 60: {short:.3f} dB); margin {margin:.3f} dB; "
          f"largest share of the bound {100 * float((err / b).max()):.1f} %")
    assert abs((snr_db - twin_db) - short) <= 0.5, (snr_db - twin_db, short)
    assert got_db >= snr_db - margin, (got_db, snr_db, margin)
    assert got_db <= snr_db, (got_db, snr_db)


# crn_fft_forward_device + this stage against the transform alone, with the margin of the other stages: 1 + 1.5 x (the largest measured
# B / A - 1).  Measured on an MI355X in separate runs (profiles/r22_extract.txt): arm A 193.3, 193.1 and 183.7 us; with 2
# channels per stream B / A = 1.1742, 1.1712 and 1.1954, the stage alone 21.8 to 22.4 us; with 16 channels per stream 1.8957, 1.9020 and
# 1.9813, alone 166.7 to 172.0 us (the stage then reads every spectrum once and writes half as many bytes again: as much traffic as the
# transform's own, so B / A is close to 2).
SPEED_RATIO = {2: 1.293, 16: 2.472}


def test_cost_next_to_the_transform_that_feeds_it(built):
    """N = 1024, 64 streams of 1024 half-overlapped frames (537 MB of spectra), M = 64, flat 16; the method of tests/stage_gpu.py
    (best_of_windows).  Arm A is the transform of every frame; arm B the same followed by this stage, with 2 channels per stream and with
    16 (every bin of the band is extracted then).  The stage alone is measured the same way; all figures are printed."""
    n, S, F, m = 1024, 64, 1024, 64
    iq_t = sgpu.noise_batch(S * F + 1, 1, n // 2)
    s = cs.Sensor(sgpu.cfg(n))
    x_t = sgpu.zeros((S * F * n * 2,), torch.float32)
    h = cs.extract_taper(m, 16)
    h_t = torch.from_numpy(h).to(DEV)
    loads = {}
    for per in (2, 16):
        cen = [32 + 64 * i for i in range(16)] if per == 16 else [300, 801]
        ch = xf.channel_records([(st, k) for st in range(S) for k in cen])
        loads[per] = (ch, _upload(ch), sgpu.Padded(out=len(ch) * F * (m // 2) * 8))
    q = cs.extract_params(m, F)

    def arm_a():
        s.fft_forward_device(iq_t.data_ptr(), S * F, n, x_t.data_ptr(), frame_stride=n // 2)

    def stage(per):
        ch, ch_t, out = loads[per]
        s.extract_device(x_t.data_ptr(), S * F, q, ch_t.data_ptr(), len(ch), h_t.data_ptr(), out.out.data_ptr())
    arms = {"A": arm_a}
    for per in (2, 16):
        arms[f"B, {per} channels per stream"] = lambda per=per: (arm_a(), stage(per))
        arms[f"alone, {per} channels per stream"] = lambda per=per: stage(per)
    times = sgpu.best_of_windows(arms)
    best = {name: min(v) for name, v in times.items()}
    # the stage computed what the definition says: stream 5's first four frames once more on their own, the same bytes, and against the twin
    X = x_t.view(S, F, n, 2)[5, :4].cpu().numpy().view(np.complex64)[..., 0]
    for per in (2, 16):
        ch, _, out = loads[per]
        mine = np.flatnonzero(ch["stream"] == 5)
        rb = F * (m // 2) * 8                                              # bytes of a row
        big = b"".join(out.out[c * rb: c * rb + 4 * (m // 2) * 8].cpu().numpy().tobytes() for c in mine)
        sub = ch[mine].copy()
        sub["stream"] = 0
        y, _ = _extract(s, X, sub, h, m, 4)
        assert y.tobytes() == big, per
        _against_twin(y, X, sub, h, m, 4, 0, ("cost", per))
        assert bool((out.out[len(ch) * rb:] == 255).all()), "memory behind the output was written"
    s.close()
    for per in (2, 16):
        n_chan = S * per
        moved = n_chan * F * (m * 8 + m // 2 * 8)                          # bins read once per channel, samples written
        alone = best[f"alone, {per} channels per stream"]
        print(f"N=1024, {S} streams of {F} half-overlapped frames ({S * F * n * 8 / 1e6:.0f} MB), M={m}, {per} channels per stream: arm A (transform) "
              f"{best['A']:.4f} ms; B / A = {best[f'B, {per} channels per stream'] / best['A']:.4f}; crn_extract_device alone {alone * 1e3:.1f} us; "
              f"{moved / 1e6:.0f} MB to move: {moved / alone / 1e9:.2f} TB/s")
    for per in (2, 16):
        ratio = best[f"B, {per} channels per stream"] / best["A"]
        assert ratio <= SPEED_RATIO[per], (per, ratio, SPEED_RATIO[per])
