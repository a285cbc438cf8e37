"""crn_measure_device on the MI355X: the kernel against the twin (tests/measure_f64.py) fed the kernel's own inputs, byte for byte: the
powers of a segment become integers once and every sum is an integer sum, so there is no rounding freedom, net_power and crest
included (crest is one fp64 division rounded to fp32 on both sides).  The output array has 256 bytes of 0xFF behind it that must stay.
Then the records the stage must survive, the chain behind the CFAR launch with its cuts, the refusals that need a live handle, the
generator's band noise and carrier end to end against the bars of tests/measure_cases.py, and the cost next to the CFAR launch with
the segment stage."""
import ctypes as C

import numpy as np
import pytest

import crnsense as cs
import measure_cases as mc
import measure_f64 as mf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402

G_, W_ = 2, 16
SIZES = (512, 1024, 2048, 4096)


def _upload(a):
    """A structured array's bytes on the device."""
    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(DEV)


def _params(ms, params):
    sub, ppm, ratio = params
    q = cs.measure_params(ms, subtract_noise=bool(sub))
    q.tail_ppm, q.xdb_ratio = int(ppm), float(ratio)
    return q


def _launch(s, spec_t, E, q, heads_t, recs_t, out, first=0, count=None):
    """Epochs first .. first + count - 1 of the batch; spec_t [E][n] float32, heads_t, recs_t and out.measures flat uint8."""
    count = E - first if count is None else count
    ms = q.max_segments
    s.measure_device(spec_t.data_ptr() + first * spec_t.shape[1] * 4, count, q, heads_t.data_ptr() + first * 16,
                     recs_t.data_ptr() + first * ms * 32, out.measures.data_ptr() + first * ms * 32)


def _got(out, E, ms):
    out.host()
    assert out.pads_untouched(), "memory behind the array was written"
    return out.view("measures", cs.MEASURE_DTYPE, (E, ms))


def _same(got, want, what):
    for f in ("obw_lo", "obw_width", "xdb_lo", "xdb_width", "n_above"):
        assert (got[f] == want[f]).all(), (what, f, np.argwhere(got[f] != want[f])[:8])
    for f in ("net_power", "crest", "reserved"):
        a, b = got[f].view(np.uint32), want[f].view(np.uint32)
        assert (a == b).all(), (what, f, np.argwhere(a != b)[:8], got[f][a != b][:4], want[f][a != b][:4])
    assert got.tobytes() == want.tobytes(), what


def _check(s, P, heads, recs, ms, param_sets, what):
    """One launch per parameter set over 0xFF-filled outputs, every byte against the twin.  Returns the last result."""
    E = P.shape[0]
    spec_t, heads_t, recs_t = sgpu.upload_rows(P), _upload(heads), _upload(recs)
    for params in param_sets:
        out = sgpu.Padded(measures=E * ms * 32)
        _launch(s, spec_t, E, _params(ms, params), heads_t, recs_t, out)
        got = _got(out, E, ms)
        _same(got, mc.measure(P, heads, recs, ms, params), (what, params))
    return got


@pytest.mark.parametrize("ms", [1, 16, 256])
@pytest.mark.parametrize("n", SIZES)
def test_hand_made_records_against_twin(built, n, ms):
    """tests/measure_cases.hand_made: widths 1, 2, 63, 64, 65, 127, 128, 129, N - 1 and N (lo = 0), spans across the wrap, the peak where
    the row has it, at the first and at the last bin, n_stored 0, 1 and max_segments, a span whose every bin is <= noise_mean, a NaN
    inside a span, a row of subnormals; Gamma(10) rows and rows quantised to quarters; every set of measure_cases.PARAMS
    (subtract_noise 0 and 1, tail_ppm 0, 5000 and 499999, xdb_ratio 0, 0.5 and 10^-2.6).  Records beyond n_stored hold 0xFF bytes and must
    come out as zeros."""
    s = cs.Sensor(sgpu.cfg(n))
    measured = 0
    for quantised in (False, True):
        P, heads, recs = mc.hand_made(n, ms, quantised)
        got = _check(s, P, heads, recs, ms, mc.PARAMS, f"N={n} max_segments={ms} quantised={quantised}")
        measured += int((got["obw_width"] > 0).sum())
        stored = np.arange(ms)[None, :] < heads["n_stored"][:, None]
        assert not got[~stored].tobytes().strip(b"\0")
    s.close()
    assert measured > 0


@pytest.mark.parametrize("n", [512, 4096])
def test_records_the_stage_must_survive(built, n):
    """lo = N + 5 and - 1, width 0 and N + 1, peak_power + inf, - inf and NaN, n_stored = max_segments + 3 and - 2, a NaN, an infinite and
    a negative noise_mean: zero records, the clamped count, the noise left alone; pads untouched.  Every row index of the kernel is masked
    with N - 1 and every count clamped before it is used (csrc/crn_measure.hip): this states the defined output."""
    ms = 4
    rng = np.random.default_rng(n)
    P = mc.rows(n, 12, n)
    heads = np.zeros(12, np.dtype(mc.SEGMENT_EPOCH_DTYPE))
    recs = np.zeros((12, ms), np.dtype(mc.SEGMENT_DTYPE))
    for e in range(12):
        heads[e] = (ms, ms, n, 1.0)
        for sl in range(ms):
            recs[e, sl] = mc.record(P[e], int(rng.integers(0, n)), int(rng.integers(1, 200)))
    zero = []                                                      # (epoch, slot) that must come out as zero bytes
    for e, (field, value) in enumerate((("lo", n + 5), ("lo", -1), ("width", 0), ("width", n + 1), ("peak_power", np.inf),
                                        ("peak_power", -np.inf), ("peak_power", np.nan))):
        recs[field][e, 1] = value
        zero.append((e, 1))
    recs["lo"][7, 2], recs["width"][7, 3] = 2 ** 31 - 1, -2 ** 31
    zero += [(7, 2), (7, 3)]
    heads["n_stored"][8], heads["n_stored"][9] = ms + 3, -2
    zero += [(9, sl) for sl in range(ms)]
    heads["noise_mean"][9], heads["noise_mean"][10], heads["noise_mean"][11], heads["noise_mean"][8] = np.nan, np.nan, np.inf, -1.0
    s = cs.Sensor(sgpu.cfg(n))
    got = _check(s, P, heads, recs, ms, mc.PARAMS[:1], f"N={n}")
    s.close()
    for e, sl in zero:
        assert not got[e, sl].tobytes().strip(b"\0"), (e, sl)
    assert (got["obw_width"][8] > 0).all() and (got["obw_width"][10] > 0).all() and (got["obw_width"][11] > 0).all()
    # a noise_mean that cannot be used is no noise_mean
    want = mc.measure(P[10:], heads[10:], recs[10:], ms, (0,) + mc.PARAMS[0][1:])
    assert got[10:].tobytes() == want.tobytes()


@pytest.mark.parametrize("n", [512, 4096])
def test_chain_behind_the_cfar_launch_and_cuts(built, n):
    """tests/signals.make_epochs traffic, CA-CFAR at Pfa 1e-2, crn_segments_device (merge_gap 3, max_segments 16), this stage: the twin is
    fed the arrays the device wrote.  The batch cut into launches of [1, 2, the rest] gives the same bytes."""
    import signals
    k, E, ms = 10, 10, 16
    cfg = sgpu.cfg(n, k=k)
    iq, _ = signals.make_epochs(cfg, E, seed=n + 3)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-2, k, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, torch.from_numpy(iq).to(DEV), E, band_bins=False)
    heads_t, recs_t = sgpu.zeros((E * 16,), torch.uint8), sgpu.zeros((E * ms * 32,), torch.uint8)
    s.segments_device(outs["mask"].data_ptr(), outs["spectrum"].data_ptr(), E, heads_t.data_ptr(), recs_t.data_ptr(), merge_gap=3, max_segments=ms)
    whole = {}
    for params in (mc.PARAMS[0], mc.PARAMS[3]):
        q = _params(ms, params)
        out = sgpu.Padded(measures=E * ms * 32)
        _launch(s, outs["spectrum"], E, q, heads_t, recs_t, out)
        whole[params] = _got(out, E, ms)
        cut = sgpu.Padded(measures=E * ms * 32)
        for first, count in ((0, 1), (1, 2), (3, E - 3)):
            _launch(s, outs["spectrum"], E, q, heads_t, recs_t, cut, first, count)
        assert _got(cut, E, ms).tobytes() == whole[params].tobytes(), params
    P = outs["spectrum"].cpu().numpy()
    heads = np.frombuffer(heads_t.cpu().numpy().tobytes(), cs.SEGMENT_EPOCH_DTYPE)
    recs = np.frombuffer(recs_t.cpu().numpy().tobytes(), cs.SEGMENT_DTYPE).reshape(E, ms)
    s.close()
    for params, got in whole.items():
        _same(got, mc.measure(P, heads, recs, ms, params), (n, params))
    stored = np.arange(ms)[None, :] < heads["n_stored"][:, None]
    got = whole[mc.PARAMS[0]]
    print(f"N={n}: {int(stored.sum())} stored segments in {E} epochs, {int((got['obw_width'] > 0).sum())} measured; widest segment "
          f"{int(recs['width'].max())} bins, widest occupied span {int(got['obw_width'].max())}")
    assert stored.sum() > E // 2 and (got["obw_width"][stored] >= 1).all() and (got["obw_width"] <= recs["width"]).all()


def test_refusals_with_a_live_handle(built):
    """Every refusal of the header's list with a live handle; a refused call and n_epochs = 0 leave the output as it was."""
    n, E, ms = 512, 8, 4
    L = cs.lib()
    s = cs.Sensor(sgpu.cfg(n))
    P, heads, recs = mc.simulate(3, "flat", dict(mc.SIM, n=n, rows=E, lo=100, emitter=(110, 64)))
    recs = np.repeat(recs, ms, axis=1)
    heads["n_stored"] = ms
    spec_t, heads_t, recs_t = sgpu.upload_rows(P), _upload(heads), _upload(recs)
    out = sgpu.Padded(measures=E * ms * 32)
    inf, nan = float("inf"), float("nan")

    def rc(sp=spec_t.data_ptr(), n_e=E, q=None, he=heads_t.data_ptr(), re=recs_t.data_ptr(), me=out.measures.data_ptr(), h=s._h, reserved=(0, 0, 0, 0),
           **kw):
        if q is None:
            q = cs.MeasureParams(**{"max_segments": ms, "tail_ppm": 5000, "xdb_ratio": 0.25, "subtract_noise": 1, **kw})
            for i, x in enumerate(reserved):
                q.reserved[i] = x
        v = lambda p: C.c_void_p(p or None)      # noqa: E731
        return L.crn_measure_device(h, v(sp), n_e, C.byref(q) if q != 0 else None, v(he), v(re), v(me), None)
    assert rc() == 0
    before = out.host()["measures"].copy()
    assert before.tobytes().strip(b"\0") and (out.view("measures", cs.MEASURE_DTYPE)["obw_width"] > 0).all()
    out.measures[: E * ms * 32] = 255
    for bad in ({"h": None}, {"sp": 0}, {"q": 0}, {"he": 0}, {"re": 0}, {"me": 0}, {"n_e": -1},
                {"max_segments": 0}, {"max_segments": 257}, {"max_segments": -1}, {"tail_ppm": -1}, {"tail_ppm": 500000},
                {"xdb_ratio": -0.5}, {"xdb_ratio": 1.0}, {"xdb_ratio": 2.0}, {"xdb_ratio": inf}, {"xdb_ratio": -inf}, {"xdb_ratio": nan},
                {"subtract_noise": 2}, {"subtract_noise": -1},
                {"reserved": (1, 0, 0, 0)}, {"reserved": (0, 1, 0, 0)}, {"reserved": (0, 0, 1, 0)}, {"reserved": (0, 0, 0, -1)},
                {"sp": spec_t.data_ptr() + 4}, {"sp": spec_t.data_ptr() + 8}, {"he": heads_t.data_ptr() + 8}, {"re": recs_t.data_ptr() + 8},
                {"me": out.measures.data_ptr() + 4}, {"me": out.measures.data_ptr() + 8}):
        assert rc(**bad) == cs.CRN_ERR_ARG, bad
        assert b"crn_measure_device" in L.crn_last_error(), bad
    assert rc(n_e=0) == 0
    assert (out.host()["measures"] == 255).all() and out.pads_untouched()
    assert rc(xdb_ratio=0.0, tail_ppm=0, subtract_noise=0, max_segments=ms) == 0 and rc(tail_ppm=499999, xdb_ratio=0.99999994) == 0
    assert rc() == 0
    assert out.host()["measures"].tobytes() == before.tobytes() and out.pads_untouched()
    s.close()


# merge_gap: a smallest-of CFAR with 16 training cells a side behind 2 guard cells sees the outer 8 bins or so of a flat emitter at + 10 dB
# (further in, the quieter side's cells hold too much of the emitter), so the closing has to bridge up to 66 - 16 bins; a carrier needs
# none, and a wide closing would only pull false alarms into its segment
E2E = {"n": 1024, "k": 10, "epochs": 64, "seed": 2044, "noise_power": 1e-6, "merge_gap": {cs.SIG_BAND_NOISE: 64, cs.SIG_CW: 3}, "max_segments": 16,
       "margin": (mc.SIM["width"] - mc.SIM["emitter"][1]) // 2}      # the bars were taken on a span that reaches 10 bins beyond the emitter on either side


def _span(bins, n):
    """(first bin, bins from the first to the last) of a channel, around the circle: the channel across the wrap leaves two bins out at
    its middle."""
    b = np.sort(np.asarray(bins))
    gaps = np.diff(np.concatenate([b, b[:1] + n]))
    return int(b[(int(np.argmax(gaps)) + 1) % b.size]), n - int(gaps.max()) + 1


def _end_to_end(kind):
    """(records of the strongest segment of every driven epoch, for band noise where it holds the whole driven channel and at most
    E2E["margin"] bins more on either side, those segments, the channels' widths, how many epochs were driven): the generator's traffic
    through a smallest-of CFAR launch (a cell-averaging one does not see the inside of a flat emitter 60 bins wide, and at + 10 dB not
    its edges either), crn_segments_device with the closing of E2E, and this stage; every record equals the twin.  A channel's width
    is its extent in bins."""
    n, k, E, ms = E2E["n"], E2E["k"], E2E["epochs"], E2E["max_segments"]
    cfg = sgpu.cfg(n, k=k)
    chan = {}
    for g in cfg.segs[: cfg.n_segs]:
        if g.band != 0:
            chan.setdefault(g.band, []).extend(range(g.lo, g.hi))
    widest = max(len(b) for b in chan.values())
    iq_t = sgpu.zeros((cs.samples_needed(cfg, E) * 2,), torch.float32)
    truth_t = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    sc = cs.SynthCfg()
    # band noise of total power signal_rms^2 over w bins against noise_power over N bins: + 10 dB per bin on the widest channel
    sc.seed, sc.noise_power, sc.signal_rms = E2E["seed"], E2E["noise_power"], float(np.sqrt(10.0 * widest / n * E2E["noise_power"]))
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = 0, cs.PU_UNIFORM, kind, 1
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), E, cs.samples_per_epoch(cfg), sc, truth_ptr=truth_t.data_ptr())
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_, method="so"), 1, method="so")
    outs = sgpu.cfar_launch(s, cfg, iq_t, E, band_bins=False)
    heads_t, recs_t = sgpu.zeros((E * 16,), torch.uint8), sgpu.zeros((E * ms * 32,), torch.uint8)
    s.segments_device(outs["mask"].data_ptr(), outs["spectrum"].data_ptr(), E, heads_t.data_ptr(), recs_t.data_ptr(), merge_gap=E2E["merge_gap"][kind],
                      max_segments=ms)
    q = cs.measure_params(ms)
    out = sgpu.Padded(measures=E * ms * 32)
    _launch(s, outs["spectrum"], E, q, heads_t, recs_t, out)
    got = _got(out, E, ms)
    P = outs["spectrum"].cpu().numpy()
    heads = np.frombuffer(heads_t.cpu().numpy().tobytes(), cs.SEGMENT_EPOCH_DTYPE)
    recs = np.frombuffer(recs_t.cpu().numpy().tobytes(), cs.SEGMENT_DTYPE).reshape(E, ms)
    truth = truth_t.cpu().numpy()
    s.close()
    _same(got, mf.run(P, heads, recs, ms, q.tail_ppm, q.xdb_ratio, q.subtract_noise), ("end to end", kind))
    picked, segs, widths = [], [], []
    for e in np.flatnonzero(truth > 0):
        if heads["n_stored"][e] < 1:
            continue
        sl = int(np.argmax(recs["power"][e, : heads["n_stored"][e]]))
        g = recs[e, sl]
        first, extent = _span(chan[int(truth[e])], n)
        before = (first - int(g["lo"])) % n                       # bins of the segment in front of the channel
        after = int(g["width"]) - before - extent
        if kind == cs.SIG_BAND_NOISE and not (0 <= before <= E2E["margin"] and 0 <= after <= E2E["margin"]):
            continue
        picked.append(got[e, sl])
        segs.append(g)
        widths.append(extent)
    return np.array(picked), np.array(segs), np.array(widths, float), int((truth > 0).sum())


def test_end_to_end_band_noise_and_carrier(built):
    """crn_synth_fill_device_ex at N = 1024, K = 10, rect, 64 epochs, a uniform pick among idle and the three channels (one of them across
    the wrap): band noise 10 dB over the noise in every bin of the widest channel, and a carrier of the same total power at the channel's
    centre bin.  The bars of tests/measure_cases.py: the occupied width of the flat emitter against the channel's true width in bins,
    in the mean and row by row; its fill; the carrier's - 26 dB width.  The strongest stored segment of a driven epoch counts where it
    holds the whole channel (the closing bridged the inside) and no more than 10 bins beyond it on either side, the span the bars were
    taken on (a closing this wide pulls false alarms in, and the half of the noise that survives the subtraction over 60 bins outweighs
    the 0.5 % tail: include/crn_sense.h, Limits); at least half of the driven epochs must give one."""
    m, segs, widths, driven = _end_to_end(cs.SIG_BAND_NOISE)
    assert driven >= 32 and len(m) >= driven / 2, (driven, len(m))
    off = m["obw_width"] - widths
    fill = m["n_above"] / np.maximum(m["xdb_width"], 1)
    print(f"band noise: {len(m)} of {driven} driven epochs; segment width - channel width {np.mean(segs['width'] - widths):.2f} bins (max "
          f"{int((segs['width'] - widths).max())}); occupied width - channel width: mean {off.mean():.2f} ({int(off.min())} .. {int(off.max())}; bars "
          f"{mc.OBW_MEAN_WITHIN}, {mc.OBW_ROW_RANGE}); fill {fill.mean():.3f} (bar {mc.FILL_FLAT_MIN}); crest {m['crest'].mean():.2f}")
    assert abs(off.mean()) <= mc.OBW_MEAN_WITHIN
    assert mc.OBW_ROW_RANGE[0] <= off.min() and off.max() <= mc.OBW_ROW_RANGE[1]
    assert fill.mean() >= mc.FILL_FLAT_MIN
    assert m["crest"].mean() <= mc.CREST_FLAT_MAX
    m, segs, widths, driven = _end_to_end(cs.SIG_CW)
    assert driven >= 32 and len(m) >= driven / 2, (driven, len(m))
    print(f"carrier: {len(m)} of {driven} driven epochs; segment width {segs['width'].mean():.2f} bins (max {int(segs['width'].max())}); - 26 dB width "
          f"{m['xdb_width'].mean():.2f} (max {int(m['xdb_width'].max())}; bar {mc.CARRIER_XDB_MEAN}); occupied width {m['obw_width'].mean():.2f}")
    assert m["xdb_width"].mean() <= mc.CARRIER_XDB_MEAN
    assert ((m["xdb_lo"] + segs["lo"]) % E2E["n"] == segs["peak_bin"]).mean() >= 0.9      # the line sits on the carrier


# CFAR launch + crn_segments_device + crn_measure_device against the first two alone, `spectrum` written in both arms, with the margin of
# tests/test_lad_gpu.py: 1 + 1.5 x (the larger measured B / A - 1).  Measured on an MI355X in two separate runs (profiles/r18_measure.txt,
# DESIGN.md §5): arm A 461.8 us, B / A = 1.0577, the stage alone 25.6 us; arm A 458.7 us, B / A = 1.0521, alone 25.2 us.
SPEED_RATIO = 1.087


def test_cost_next_to_the_segment_stage(built):
    """N = 4096, K = 10, rect, 64 bands, 6656 epochs, add_tones traffic, max_segments 16; the method of tests/stage_gpu.py
    (best_of_windows): each timed window holds 8 launches issued back to back behind one already queued, the arms alternate, 5 windows
    each after a warm-up, the best counts.  Arm A is the CFAR launch followed by crn_segments_device, arm B the same followed by
    crn_measure_device on the same stream.  The stage alone is measured the same way and printed."""
    n, k, ms = 4096, 10, 16
    cfg = sgpu.cfg(n, k=k, bands=64)
    E = 6656                                  # 6656 x 10 x 4096 x 8 B = 2.18 GB
    iq_t = sgpu.add_tones(sgpu.noise_batch(E, k, n), E, k, n)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = sgpu.cfar_outs(cfg, E)
    heads_t, recs_t = sgpu.zeros((E * 16,), torch.uint8), sgpu.zeros((E * ms * 32,), torch.uint8)
    out = sgpu.Padded(measures=E * ms * 32)
    q = cs.measure_params(ms)

    def arm_a():
        sgpu.cfar_launch(s, cfg, iq_t, E, outs=outs)
        s.segments_device(outs["mask"].data_ptr(), outs["spectrum"].data_ptr(), E, heads_t.data_ptr(), recs_t.data_ptr(), max_segments=ms)

    def stage():
        _launch(s, outs["spectrum"], E, q, heads_t, recs_t, out)

    def arm_b():
        arm_a()
        stage()
    times = sgpu.best_of_windows({"A": arm_a, "B": arm_b, "alone": stage})
    got = _got(out, E, ms)
    # the stage computed what the definition says: every 64th epoch against the twin
    pick = np.arange(0, E, 64)
    P = outs["spectrum"][pick].cpu().numpy()
    heads = np.frombuffer(heads_t.cpu().numpy().tobytes(), cs.SEGMENT_EPOCH_DTYPE)
    recs = np.frombuffer(recs_t.cpu().numpy().tobytes(), cs.SEGMENT_DTYPE).reshape(E, ms)
    s.close()
    _same(got[pick], mf.run(P, heads[pick], recs[pick], ms, q.tail_ppm, q.xdb_ratio, q.subtract_noise), "cost batch")
    best = {name: min(v) for name, v in times.items()}
    nbytes = E * k * n * 8
    moved = E * (n * 4 + 16 + 2 * ms * 32)
    print(f"N=4096 K=10 rect 64 bands, {E} epochs ({nbytes / 1e9:.2f} GB), spectrum written: arm A (CFAR launch + crn_segments_device) {best['A']:.4f} ms; "
          f"B / A = {best['B'] / best['A']:.4f}; crn_measure_device alone {best['alone'] * 1e3:.1f} us ({moved / best['alone'] / 1e6:.0f} GB/s of its own "
          f"{moved / 1e6:.0f} MB); mean n_stored {heads['n_stored'].mean():.2f}, measured {int((got['obw_width'] > 0).sum())}")
    assert (got["obw_width"] > 0).sum() > E
    assert best["B"] <= SPEED_RATIO * best["A"], (best["B"] / best["A"], SPEED_RATIO)
