"""crn_segments_device on the MI355X: the kernel against the float64 twin (tests/segments_f64.py) fed the kernel's own inputs, so the
comparison is exact — every integer field equal, peak_power the same bits, unused slots zero, and power / centroid / noise_mean within
2^-22 relative (the twin's float64 value rounded to fp32 is within 2^-24 of it, the kernel's fp64 accumulation differs from the twin's
by at most width x 2^-53 before its own rounding; 2^-22 leaves room for a value on a rounding boundary going the other way and for the
centroid's divide).  Then hand-made and random masks uploaded from the host, cut independence, refusals, the wrap end to end, and the
cost next to the CFAR launch alone."""
import ctypes as C

import numpy as np
import pytest

import crnsense as cs
import segments_f64 as sg

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402

G_, W_ = 2, 16
SIZES = (512, 1024, 2048, 4096)
MERGE_GAPS, MIN_WIDTHS, MAX_SEGMENTS = (0, 1, 3, 40), (1, 2, 5), (1, 16, 256)


def _cfar(s, cfg, iq_t, E, outs=None):
    """One CFAR launch over E epochs without band_bins; returns the device tensors (mask [E][N / 32] int32, spectrum [E][N])."""
    return sgpu.cfar_launch(s, cfg, iq_t, E, outs=outs, band_bins=False)


class _Out:
    """The two output arrays of a batch on the device, filled with 0xFF first so that a slot the kernel skipped shows."""

    def __init__(self, E, max_segments):
        self.E, self.ms = E, max_segments
        self.epochs = torch.full((E, 16), 255, dtype=torch.uint8, device=DEV)
        self.segments = torch.full((E, max_segments, 32), 255, dtype=torch.uint8, device=DEV)

    def host(self):
        torch.cuda.synchronize()
        return (np.frombuffer(self.epochs.cpu().numpy().tobytes(), cs.SEGMENT_EPOCH_DTYPE),
                np.frombuffer(self.segments.cpu().numpy().tobytes(), cs.SEGMENT_DTYPE).reshape(self.E, self.ms))


def _segments(s, mask_t, spec_t, E, g, mw, ms, first=0, count=None, out=None, with_segments=True):
    out = _Out(E, ms) if out is None else out
    count = E - first if count is None else count
    s.segments_device(mask_t[first].data_ptr() if count else mask_t.data_ptr(), spec_t[first].data_ptr() if count else spec_t.data_ptr(),
                      count, out.epochs[first].data_ptr() if count else out.epochs.data_ptr(),
                      (out.segments[first].data_ptr() if count else out.segments.data_ptr()) if with_segments else 0,
                      merge_gap=g, min_width=mw, max_segments=ms)
    return out


def _check(s, mask_t, spec_t, n, combos, what):
    """The exact comparison over `combos` of (merge_gap, min_width, max_segments) on one pair of device arrays."""
    E = mask_t.shape[0]
    torch.cuda.synchronize()
    det = sg.unpack_mask(mask_t.cpu().numpy().view(np.uint32), n)
    P = spec_t.cpu().numpy()
    worst, found = 0.0, 0
    for g, mw, ms in combos:
        got_e, got_s = _segments(s, mask_t, spec_t, E, g, mw, ms).host()
        want_e, want_s = sg.run(det, P, g, mw, ms)
        worst = max(worst, sg.compare(got_e, got_s, want_e, want_s))
        found = max(found, int(want_e["n_found"].max()))
    print(f"{what}: {len(combos)} parameter sets x {E} epochs, most segments in an epoch {found}, widest relative error {worst:.2e} "
          f"(bound {sg.REL_TOL:.2e})")


ALL_COMBOS = [(g, mw, ms) for g in MERGE_GAPS for mw in MIN_WIDTHS for ms in MAX_SEGMENTS]


@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("window", [cs.WINDOW_RECT, cs.WINDOW_HANN])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_matches_twin_on_cfar_output(built, n, window, k):
    """tests/signals.make_epochs traffic through a CA-CFAR launch; the twin reads the mask and the rows that launch wrote."""
    import signals
    cfg = sgpu.cfg(n, window, k)
    E = 10
    iq, _ = signals.make_epochs(cfg, E, seed=n * 13 + window * 5 + k)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-2, k, W_), 1)     # Pfa 1e-2: more and closer runs for the closing to work on
    outs = _cfar(s, cfg, torch.from_numpy(iq).to(DEV), E)
    _check(s, outs["mask"], outs["spectrum"], n, ALL_COMBOS, f"make_epochs N={n} win={window} K={k}")
    s.close()


@pytest.mark.parametrize("kind", [cs.SIG_RRC_QPSK, cs.SIG_OFDM])
@pytest.mark.parametrize("n,window,k", [(512, cs.WINDOW_RECT, 10), (1024, cs.WINDOW_HANN, 10), (2048, cs.WINDOW_RECT, 1), (4096, cs.WINDOW_HANN, 10),
                                        (4096, cs.WINDOW_RECT, 10)])
def test_kernel_matches_twin_on_generated_carriers(built, n, window, k, kind):
    """The device generator's off-grid RRC-QPSK / OFDM carriers: wide segments, many lanes per segment."""
    cfg = sgpu.cfg(n, window, k)
    E = 10
    spe = cs.samples_per_epoch(cfg)
    iq_t = sgpu.zeros((cs.samples_needed(cfg, E) * 2,), torch.float32)
    sc = cs.SynthCfg()
    sc.seed, sc.noise_power, sc.signal_rms = 11 + n + kind, 1e-6, 0.02
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = 8, cs.PU_UNIFORM, kind, 1
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), E, spe, sc)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = _cfar(s, cfg, iq_t, E)
    torch.cuda.synchronize()
    det = sg.unpack_mask(outs["mask"].cpu().numpy().view(np.uint32), n)
    widest = {g: max(w for e in range(E) for _, w in (sg.runs_of(sg.close_mask(det[e], g)) if det[e].any() else [(0, 0)])) for g in (3, 40)}
    print(f"kind {kind} N={n}: widest segment {widest[3]} bins at merge_gap 3, {widest[40]} at 40")
    _check(s, outs["mask"], outs["spectrum"], n, ALL_COMBOS, f"generator kind={kind} N={n} win={window} K={k}")
    s.close()


def hand_made(n):
    """(name, set bins, merge_gap, min_width, max_segments): the cases of tests/test_segments_host.py at size n."""
    return [("empty", [], 0, 1, 16), ("empty, closing asked", [], 40, 1, 16), ("all ones", range(n), 0, 1, 16),
            ("across the wrap", [n - 2, n - 1, 0, 1], 0, 1, 16), ("joined across the wrap", [n - 3, 1], 3, 1, 16),
            ("not joined across the wrap", [n - 3, 1], 2, 1, 16), ("closing fills the circle", range(0, n, 2), 1, 1, 16),
            ("one bit, the widest closing", [n // 3], n - 1, 1, 16), ("one bit", [n // 3], n - 2, 1, 16),
            ("alternating, capped", range(0, n, 2), 0, 1, 8), ("alternating, 256 slots", range(0, n, 2), 0, 1, 256),
            ("min_width after merging", [3, 10, 12], 1, 2, 16), ("min_width drops all", [3, 10, 12], 0, 2, 16),
            ("a lane piece and its neighbours", list(range(n // 64 - 1, 3 * (n // 64) + 1)), 0, 1, 16),
            ("runs ending on piece edges", list(range(n // 64, 2 * (n // 64))) + list(range(4 * (n // 64), 6 * (n // 64))), 0, 1, 16),
            ("solid but one", [k for k in range(n) if k != n // 2], 0, 1, 16), ("solid but the first", range(1, n), 0, 1, 16),
            ("solid but the last", range(n - 1), 0, 1, 16), ("wide gap closed over empty pieces", [5, 5 + 3 * (n // 64) + 2], n // 16, 1, 16),
            ("wrap segment dropped by min_width", [n - 1, 0, 7, 8, 9], 0, 3, 16), ("wrap segment kept, capped", [n - 1, 0, 7, 20, 30], 0, 1, 2)]


@pytest.mark.parametrize("n", SIZES)
def test_hand_made_masks(built, n):
    rng = np.random.default_rng(n)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    for name, bits, g, mw, ms in hand_made(n):
        det = np.zeros((3, n), bool)
        det[:, list(bits)] = True
        P = rng.gamma(10.0, 1e-4, (3, n)).astype(np.float32)
        P[1] = 1.0                      # every comparison of the peak is a tie: the smallest offset wins
        P[2] = np.repeat(P[2, ::2], 2)                  # equal neighbours
        _check(s, sgpu.upload_mask(det), sgpu.upload_rows(P), n, [(g, mw, ms)], f"N={n} {name}")
    s.close()


@pytest.mark.parametrize("density", [0.001, 0.05, 0.5, 0.95])
@pytest.mark.parametrize("n", SIZES)
def test_random_masks(built, n, density):
    rng = np.random.default_rng(int(n + 1000 * density))
    E = 12
    det = rng.random((E, n)) < density
    P = (rng.gamma(10.0, 1e-4, (E, n)) * np.where(rng.random((E, n)) < 0.02, 1e4, 1.0)).astype(np.float32)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    combos = [(0, 1, 16), (1, 2, 256), (3, 1, 256), (40, 5, 16), (0, 1, 1), (3, 5, 1), (n - 1, 1, 16), (1, 1, 16), (40, 2, 256)]
    _check(s, sgpu.upload_mask(det), sgpu.upload_rows(P), n, combos, f"N={n} density {density}")
    s.close()


@pytest.mark.parametrize("n", [512, 4096])
def test_cut_independence_and_headers_only(built, n):
    rng = np.random.default_rng(n + 1)
    E, a = 37, 13
    det = rng.random((E, n)) < 0.05
    det[5] = False
    det[6] = True
    P = rng.gamma(10.0, 1e-4, (E, n)).astype(np.float32)
    mask_t, spec_t = sgpu.upload_mask(det), sgpu.upload_rows(P)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    for g, mw, ms in ((0, 1, 16), (3, 2, 4), (40, 1, 256)):
        whole = _segments(s, mask_t, spec_t, E, g, mw, ms)
        parts = _segments(s, mask_t, spec_t, E, g, mw, ms, first=0, count=a)
        parts = _segments(s, mask_t, spec_t, E, g, mw, ms, first=a, count=E - a, out=parts)
        heads = _segments(s, mask_t, spec_t, E, g, mw, ms, with_segments=False)
        torch.cuda.synchronize()
        assert whole.epochs.cpu().numpy().tobytes() == parts.epochs.cpu().numpy().tobytes()
        assert whole.segments.cpu().numpy().tobytes() == parts.segments.cpu().numpy().tobytes()
        assert whole.epochs.cpu().numpy().tobytes() == heads.epochs.cpu().numpy().tobytes()
        assert (heads.segments.cpu().numpy() == 255).all(), "d_segments = NULL must leave the segment array alone"
    # n_epochs = 0 launches nothing
    untouched = _segments(s, mask_t, spec_t, E, 0, 1, 16, first=0, count=0)
    torch.cuda.synchronize()
    assert (untouched.epochs.cpu().numpy() == 255).all() and (untouched.segments.cpu().numpy() == 255).all()
    s.close()


def test_refusals_and_any_handle(built):
    """The refusals that need a live handle; a REF_MAG handle with CFAR off extracts from an uploaded mask like any other."""
    n = 512
    L = cs.lib()
    s = cs.Sensor(cs.cfg_reference())        # REF_MAG, ANN decision: CFAR cannot even be switched on here
    assert s.get_cfar() is None
    det = np.zeros((2, n), bool)
    det[0, [n - 1, 0, 40, 41]] = True
    P = np.random.default_rng(0).gamma(10.0, 1e-4, (2, n)).astype(np.float32)
    mask_t, spec_t = sgpu.upload_mask(det), sgpu.upload_rows(P)
    _check(s, mask_t, spec_t, n, [(0, 1, 16)], "REF_MAG handle, uploaded mask")
    out = _Out(2, 16)

    def rc(h=None, m=mask_t.data_ptr(), sp=spec_t.data_ptr(), E=2, q=None, ep=out.epochs.data_ptr(), sgp=out.segments.data_ptr(), **kw):
        q = cs.SegmentParams(merge_gap=kw.get("g", 0), min_width=kw.get("mw", 1), max_segments=kw.get("ms", 16), reserved=kw.get("r", 0)) if q is None else q
        return L.crn_segments_device(s._h if h is None else h, C.c_void_p(m or None), C.c_void_p(sp or None), E,
                                     C.byref(q) if q != 0 else None, C.c_void_p(ep or None), C.c_void_p(sgp or None), None)
    assert rc() == 0
    for bad in ({"g": -1}, {"g": n}, {"mw": 0}, {"mw": -3}, {"ms": 0}, {"ms": 257}, {"r": 1}, {"E": -1}, {"m": 0}, {"sp": 0}, {"ep": 0}, {"q": 0},
                {"sp": spec_t.data_ptr() + 4}, {"m": mask_t.data_ptr() + 4}):
        assert rc(**bad) == cs.CRN_ERR_ARG, bad
        assert b"crn_segments_device" in L.crn_last_error()
    assert rc(g=n - 1) == 0 and rc(ms=256, sgp=0) == 0 and rc(ms=1) == 0 and rc(E=0) == 0
    torch.cuda.synchronize()
    s.close()


def _wrap_pair(n, k, E, seed):
    """White noise of power 1e-6 per sample plus, in every frame, on-grid tones at bins N - 1 and 0, each 40 dB over the floor in its
    bin (rect: |X|^2 = a^2 N^2 against N 1e-6), phases redrawn per frame."""
    rng = np.random.default_rng(seed)
    F = E * k
    x = (rng.normal(0, np.sqrt(0.5e-6), (F, n)) + 1j * rng.normal(0, np.sqrt(0.5e-6), (F, n)))
    a = np.sqrt(1e-6 * 1e4 / n)
    m = np.arange(n)
    x += a * np.exp(2j * np.pi * ((n - 1) * m % n) / n + 2j * np.pi * rng.uniform(size=(F, 1)))
    x += a * np.exp(2j * np.pi * rng.uniform(size=(F, 1))) * np.ones(n)
    return x.astype(np.complex64).view(np.float32).reshape(-1).copy()


@pytest.mark.parametrize("n", [512, 4096])
def test_end_to_end_pair_across_the_wrap(built, n):
    """Rect, K = 10, guard 2, train 16, CA at Pfa 1e-3, 40 epochs: the pair at bins N - 1 and 0 is one stored segment, lo = N - 1,
    width 2, n_detected 2, and the last one stored.  An epoch whose mask has bin N - 2 or bin 1 set (a false alarm beside the pair) is
    left out; at most 4 of the 40 may be."""
    k, E = 10, 40
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = _cfar(s, cfg, torch.from_numpy(_wrap_pair(n, k, E, seed=n)).to(DEV), E)
    got_e, got_s = _segments(s, outs["mask"], outs["spectrum"], E, 0, 1, 64).host()
    det = sg.unpack_mask(outs["mask"].cpu().numpy().view(np.uint32), n)
    s.close()
    left_out = det[:, n - 2] | det[:, 1]
    print(f"N={n}: {int(left_out.sum())} of {E} epochs left out; n_found max {int(got_e['n_found'].max())}, mean {got_e['n_found'].mean():.2f}")
    assert left_out.sum() <= 4
    assert (got_e["n_found"] <= 64).all()
    for e in np.flatnonzero(~left_out):
        last = got_s[e, got_e["n_stored"][e] - 1]
        assert got_e["n_stored"][e] >= 1 and (last["lo"], last["width"], last["n_detected"]) == (n - 1, 2, 2), (e, last)
        assert last["peak_bin"] in (n - 1, 0) and 0.0 <= last["centroid"] < 2.0
        assert not ((got_s[e, : got_e["n_stored"][e] - 1]["lo"] == n - 1).any())


def test_noise_only_segment_load(built):
    """Recorded, not asserted beyond the twin's agreement: on noise only (N = 4096, K = 10, Pfa 1e-3) the mean n_found per epoch at
    min_width 1 and 2, i.e. how much of the false-alarm load a two-bin minimum removes."""
    n, k, E = 4096, 10, 512
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k)
    iq_t = sgpu.noise_batch(E, k, n, seed=77)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = _cfar(s, cfg, iq_t, E)
    means = {mw: float(_segments(s, outs["mask"], outs["spectrum"], E, 0, mw, 16).host()[0]["n_found"].mean()) for mw in (1, 2, 3)}
    print(f"noise only, N=4096 K=10 Pfa 1e-3: mean n_found per epoch {means[1]:.3f} at min_width 1, {means[2]:.4f} at 2, {means[3]:.5f} at 3")
    _check(s, outs["mask"][:16], outs["spectrum"][:16], n, [(0, 1, 16), (0, 2, 16)], "noise only")
    s.close()


# CFAR launch + crn_segments_device against the CFAR launch alone, `spectrum` written in both arms.  Measured on the MI355X on real
# traffic: 1.086 on one box and 1.097 on another, SPEED_MEASURED is their mean; asserted with the relative margin the
# CA speed test carries over its own measurement (1.084 measured, 1.15 asserted), because boxes of the pool differ by a few per cent.
SPEED_MEASURED = 1.0915
SPEED_RATIO = 1.158                      # 1.0915 x 1.15 / 1.084


def test_cost_next_to_the_cfar_launch(built):
    """N = 4096, K = 10, rect, 64 bands, the 2.18 GB batch; the method of tests/stage_gpu.py (best_of_windows): each timed window holds
    8 launches issued back to back behind one already queued, the arms alternate, 5 windows each after a warm-up, the best counts.
    Arm A is the CFAR launch alone, arm B the same launch followed by crn_segments_device (max_segments 16) on the same stream.  The
    uploaded all-zero, alternating and solid masks and the kernel alone are measured the same way and printed."""
    n, k = 4096, 10
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k, bands=64)
    E = 6656                                  # 6656 x 10 x 4096 x 8 B = 2.18 GB
    iq_t = sgpu.add_tones(sgpu.noise_batch(E, k, n), E, k, n)      # real traffic: epochs carry segments as well as false alarms
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = _cfar(s, cfg, iq_t, E)
    out = _Out(E, 16)
    words = {"all-zero": 0, "alternating": 0x55555555, "solid": 0xFFFFFFFF}
    masks = {name: torch.full((E, n // 32), w - (1 << 32) if w >> 31 else w, dtype=torch.int32, device=DEV) for name, w in words.items()}
    torch.cuda.synchronize()

    def arm_a():
        _cfar(s, cfg, iq_t, E, outs=outs)

    def arm_b(mask_t=None):
        _cfar(s, cfg, iq_t, E, outs=outs)
        _segments(s, outs["mask"] if mask_t is None else mask_t, outs["spectrum"], E, 0, 1, 16, out=out)

    def alone(mask_t=None):
        _segments(s, outs["mask"] if mask_t is None else mask_t, outs["spectrum"], E, 0, 1, 16, out=out)
    arms = {"A": arm_a, "B real": arm_b, "alone real": alone}
    for name, m in masks.items():
        arms["B " + name] = (lambda m=m: arm_b(m))
        arms["alone " + name] = (lambda m=m: alone(m))
    times = sgpu.best_of_windows(arms)
    got_e = out.host()[0]
    arm_b()
    real_e = out.host()[0]
    s.close()
    best = {name: min(v) for name, v in times.items()}
    nbytes = E * k * n * 8
    moved = E * (n * 4 + n // 8 + 16 + 16 * 32)
    print(f"N=4096 K=10 rect 64 bands, {E} epochs ({nbytes / 1e9:.2f} GB), spectrum written: arm A (CFAR launch alone) {best['A']:.4f} ms "
          f"({nbytes / best['A'] / 1e6:.0f} GB/s of input); real traffic: mean n_found {real_e['n_found'].mean():.2f}")
    for name in ("real", "all-zero", "alternating", "solid"):
        print(f"  {name:12s} B / A = {best['B ' + name] / best['A']:.4f}   kernel alone {best['alone ' + name] * 1e3:.1f} us "
              f"({moved / best['alone ' + name] / 1e6:.0f} GB/s of its own {moved / 1e6:.0f} MB)")
    assert got_e["n_found"].min() == 1 and got_e["n_found"].max() == 1          # the last mask measured was the solid one
    assert best["B real"] <= SPEED_RATIO * best["A"], (best["B real"] / best["A"], SPEED_RATIO)
