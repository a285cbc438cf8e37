"""crn_channels_device on the MI355X: the kernels against the twin (tests/channels_f64.py) fed the kernels' own inputs, so the comparison
is exact: every integer field of every record equal, d_busy equal, memory past the arrays still the 0xFF fill; d_power within 2^-22
relative of the twin's float64 sum (the bound of tests/test_segments_gpu.py, for the same reason: the twin's value rounded to fp32 is within
2^-24 of it, the kernel's fp64 accumulation differs by at most width x 2^-53 before its own rounding, and 2^-22 leaves room for a value on a
rounding boundary going the other way); power[] within 1e-9 relative of the twin summing the kernel's own d_power (an fp64 sum of the same
fp32 values in another order: at most epochs x 2^-53).  Then the strong neighbour, cut independence, the fused kernel's occupancy, a known
Markov chain end to end, the refusals that need a live handle, and the cost next to the CFAR launch alone."""
import ctypes as C

import numpy as np
import pytest

import channels_f64 as ch
import crnsense as cs

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402

G_, W_ = 2, 16
SIZES = (512, 1024, 2048, 4096)


def _spans(spans):
    return [(sp.lo, sp.width) if isinstance(sp, cs.ChannelSpan) else tuple(sp) for sp in spans]


class _Out(sgpu.Padded):
    """The records, d_busy and d_power of a batch on the device, each with 0xFF bytes behind it (stage_gpu.Padded).  The workspace is
    exactly the size the library asks for."""

    def __init__(self, E, n_streams, nch, spans, eps, min_bins=1):
        self.E, self.S, self.C = E, n_streams, nch
        super().__init__(stats=n_streams * nch * 192, busy=E * 8, power=E * nch * 4)
        self.ws_bytes = cs.channels_workspace_bytes(E, spans, eps, min_bins)
        self.ws = torch.full((self.ws_bytes,), 255, dtype=torch.uint8, device=DEV)

    def host(self):
        super().host()
        return self.view("stats", cs.CHANNEL_STATS_DTYPE, (self.S, self.C)), self.view("busy", np.uint64), self.view("power", np.float32, (self.E, self.C))


def _run(s, mask_t, spec_t, E, spans, eps, min_bins=1, first=True, out=None, busy=True, power=True):
    spans = _spans(spans)
    out = _Out(E, E // eps if eps else 0, len(spans), spans, eps, min_bins) if out is None else out
    s.channels_device(mask_t.data_ptr(), spec_t.data_ptr() if spec_t is not None else 0, E, out.stats.data_ptr(), out.ws.data_ptr(), out.ws_bytes,
                      spans, epochs_per_stream=eps, min_bins=min_bins, first=first, busy_ptr=out.busy.data_ptr() if busy else 0,
                      power_ptr=out.power.data_ptr() if power and spec_t is not None else 0)
    return out


def _upload(det, P):
    return sgpu.upload_mask(det), None if P is None else sgpu.upload_rows(P)


def _check(s, det, P, spans, eps, min_bins, what):
    """The exact comparison on one uploaded batch, from zeroed records (first = 1).  Returns (records, largest relative error of d_power)."""
    E = det.shape[0]
    spans = _spans(spans)
    mask_t, spec_t = _upload(det, P)
    out = _run(s, mask_t, spec_t, E, spans, eps, min_bins)
    st, busy, power = out.host()
    assert out.pads_untouched(), (what, "memory behind an output array was written")
    n_det, want_busy, want_power = ch.epochs(det, None if P is None else np.asarray(P, np.float32), spans, min_bins)
    assert (busy == want_busy).all(), (what, "d_busy", np.flatnonzero(busy != want_busy)[:8])
    if P is None:
        assert (power.view(np.uint32) == 0xFFFFFFFF).all(), (what, "d_power was written without a spectrum")
        worst = 0.0
    else:
        worst = ch.compare_power(power, want_power)
    want = ch.update(None, busy, None if P is None else power, eps, True, len(spans))
    ch.compare(st, want, what)
    assert (st["n_trans"].sum(axis=(2, 3)) == st["n_epochs"] - 1).all() and (st["run_sum"].sum(axis=2) + st["run"] == st["n_epochs"]).all()
    return st, worst


def span_sets(n, rng):
    """{n_channels: spans} at size n: width 1, width N (from bin 0 and from inside a lane piece), across the wrap, overlapping, edges on
    and one off a lane-piece edge (a piece is B = N / 64 bins), inside one piece, and random ones."""
    B = n // 64
    fixed = [(n // 3, 1), (0, n), (5, n), (n - 3, 7), (n - B - 1, 2 * B + 2), (3 * B, B), (3 * B, 2 * B), (3 * B - 1, B + 2), (3 * B + 1, B - 1),
             (3 * B + 1, 2 * B - 1), (5 * B + 2, 3), (5 * B, 1), (6 * B - 1, 1), (6 * B - 1, 2), (n - 1, 1), (n - 1, n), (n - B, B), (n - B, B + 1),
             (0, B), (0, 1), (B - 1, n - B + 2), (10 * B, 30 * B), (20 * B + 3, 30 * B), (n // 2, n // 2), (n // 2 + 1, n // 2)]
    rand = [(int(rng.integers(0, n)), int(rng.integers(1, n + 1))) for _ in range(20)] + \
           [(int(rng.integers(0, n)), int(rng.integers(1, 3 * B))) for _ in range(64 - 20 - len(fixed))]
    return {1: [(n - 3, 7)], 3: [(5, n), (n // 3, 1), (n - B - 1, 2 * B + 2)], 64: fixed + rand}


@pytest.mark.parametrize("n", SIZES)
def test_spans_against_twin(built, n):
    """Random masks (sparse and dense rows) and random rows with outliers; 1, 3 and 64 channels; min_bins 1, 3 and one larger than any
    width; with and without the spectrum."""
    rng = np.random.default_rng(n)
    E = 6
    det = rng.random((E, n)) < np.array([0.0, 0.002, 0.05, 0.5, 0.95, 1.0])[:, None]
    P = (rng.gamma(10.0, 1e-4, (E, n)) * np.where(rng.random((E, n)) < 0.02, 1e4, 1.0)).astype(np.float32)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    worst = 0.0
    for nch, spans in span_sets(n, rng).items():
        assert len(spans) == nch
        for mb in (1, 3, n + 1):
            for eps in (E, 1, 3):
                worst = max(worst, _check(s, det, P, spans, eps, mb, f"N={n} {nch} channels min_bins {mb} eps {eps}")[1])
        st, _ = _check(s, det, None, spans, E, 1, f"N={n} {nch} channels, no spectrum")
        assert not st["power"].any()
    s.close()
    print(f"N={n}: widest relative error of d_power {worst:.2e} (bound {ch.REL_TOL:.2e})")


def _chain(rng, T, p, start):
    """A two-state chain that flips with probability p per epoch."""
    return (start + np.cumsum(rng.random(T) < p)) % 2


def _det_from_bits(bits, n, nch):
    """bits [E][nch] -> a mask in which channel c, the span (c B', B') with B' = n / nch, has its first two bins set where bits says so."""
    E = bits.shape[0]
    det = np.zeros((E, n), bool)
    det[:, (n // nch) * np.arange(nch)] = bits.astype(bool)
    det[:, (n // nch) * np.arange(nch) + 1] = bits.astype(bool)
    return det, [(c * (n // nch), n // nch) for c in range(nch)]


@pytest.mark.parametrize("n_streams", [1, 3])
@pytest.mark.parametrize("eps", [1, 63, 64, 65, 129, 576, 1000, 1087])
def test_time_sequences_against_twin(built, eps, n_streams):
    """64 channels over time, one kind of sequence per channel: all idle, all busy, alternating (both phases), and random two-state
    chains that flip with p = 0.02, 0.5 and 0.98; stream lengths around the 64-epoch chunks of the time kernel and one of many chunks.
    576 and 1087 epochs are 9 and 17 chunks: the join's 8 waves take 2 and 3 chunks each, so its last three and its last two waves
    get none and hand on an empty summary (every other length here gives every wave of the join some chunk)."""
    n, nch = 512, 64
    rng = np.random.default_rng(eps * 7 + n_streams)
    E = eps * n_streams
    bits = np.zeros((n_streams, eps, nch), int)
    t = np.arange(eps)
    for st in range(n_streams):
        for c in range(nch):
            kind = c % 8
            bits[st, :, c] = (0 * t if kind == 0 else 0 * t + 1 if kind == 1 else t % 2 if kind == 2 else (t + 1) % 2 if kind == 3 else
                              _chain(rng, eps, (0.02, 0.5, 0.98, 0.02)[kind - 4], c & 1 if kind != 7 else 1 - (c >> 3 & 1)))
    det, spans = _det_from_bits(bits.reshape(E, nch), n, nch)
    P = rng.gamma(10.0, 1e-4, (E, n)).astype(np.float32)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    st, worst = _check(s, det, P, spans, eps, 1, f"eps {eps} x {n_streams} streams")
    s.close()
    assert (st["n_busy"] == bits.sum(axis=1)).all()
    print(f"eps {eps} x {n_streams}: most completed runs of a channel {int(st['n_runs'].sum(axis=2).max())}, longest run {int(st['run_max'].max())}")


def test_one_flip_at_every_position(built):
    """Three streams of 130 epochs, 64 channels each: channel c of stream s flips once, before epoch 64 s + c + 1 (every position 1 .. 129
    of the stream, across both chunk edges; even channels go idle -> busy, odd ones busy -> idle), the channels left over never flip."""
    n, nch, eps, n_streams = 512, 64, 130, 3
    t = np.arange(eps)
    bits = np.zeros((n_streams, eps, nch), int)
    for st in range(n_streams):
        for c in range(nch):
            pos = 64 * st + c + 1
            bits[st, :, c] = ((t >= pos) if c % 2 == 0 else (t < pos)) if pos < eps else c % 2
    det, spans = _det_from_bits(bits.reshape(-1, nch), n, nch)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    got, _ = _check(s, det, None, spans, eps, 1, "one flip")
    s.close()
    for st in range(n_streams):
        for c in range(nch):
            pos = 64 * st + c + 1
            if pos < eps:
                a = c % 2                                      # the state before the flip
                assert got[st, c]["n_runs"][a] == 1 and got[st, c]["n_runs"][1 - a] == 0 and got[st, c]["run_sum"][a] == pos
                assert got[st, c]["run"] == eps - pos and got[st, c]["state"] == 1 - a and got[st, c]["n_trans"][a][1 - a] == 1
            else:
                assert got[st, c]["n_runs"].sum() == 0 and got[st, c]["run"] == eps


@pytest.mark.parametrize("n", [512, 4096])
def test_strong_neighbour(built, n):
    """One bin 90 dB over the floor directly outside a channel at both edges: nothing of it may reach the channel's power.  Channels on
    and off the lane-piece edges, inside one piece, and across the wrap; the neighbours of one channel lie inside another, wider one."""
    rng = np.random.default_rng(n + 90)
    B, E = n // 64, 4
    inner = [(3 * B, B), (7 * B + 1, B - 2), (9 * B - 2, 2 * B + 5), (12 * B + 2, 3), (n - 4, 8), (20 * B, 10 * B), (40 * B + B // 2, 1)]
    P = rng.gamma(10.0, 1e-4, (E, n)).astype(np.float64)
    for lo, w in inner:
        P[:, (lo - 1) % n] = 1e-3 * 1e9 * rng.uniform(0.5, 2.0, E)
        P[:, (lo + w) % n] = 1e-3 * 1e9 * rng.uniform(0.5, 2.0, E)
    spans = inner + [(0, n), (3 * B - 1, B + 2)]
    det = rng.random((E, n)) < 0.05
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    _, worst = _check(s, det, P.astype(np.float32), spans, E, 1, f"strong neighbour N={n}")
    s.close()
    ratio = P.astype(np.float32)[:, [(lo - 1) % n for lo, _ in inner]].min() / P[:, 3 * B: 4 * B].sum(axis=1).max()
    print(f"N={n}: neighbours at least {10 * np.log10(ratio):.0f} dB over a channel's whole power; widest relative error {worst:.2e} (bound {ch.REL_TOL:.2e})")


def _ints(st):
    return b"".join(np.ascontiguousarray(st[f]).tobytes() for f in ch.INT_FIELDS)


@pytest.mark.parametrize("n,n_streams", [(512, 1), (4096, 1), (512, 3)])
def test_cut_independence(built, n, n_streams):
    """One batch against the same epochs in several calls (first = 1, then 0), cut at 1 epoch, in the middle of runs and chunks, and on a
    chunk edge: integers, d_busy and d_power byte for byte; power[] within 1e-9 (another order of the same fp64 sum)."""
    rng = np.random.default_rng(n + n_streams)
    T, nch = 300, 64
    bits = np.stack([np.stack([_chain(rng, T, (0.02, 0.3, 0.9)[c % 3], c & 1) for c in range(nch)], axis=1) for _ in range(n_streams)])
    det, spans = _det_from_bits(bits.reshape(-1, nch), n, nch)
    det |= rng.random(det.shape) < 0.01
    P = rng.gamma(10.0, 1e-4, det.shape).astype(np.float32)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    mask_t, spec_t = _upload(det, P)
    whole = _run(s, mask_t, spec_t, n_streams * T, spans, T, 2)
    w_st, w_busy, w_power = whole.host()
    for cuts in ([1], [77], [128], [1, 2, 66, 131, 299], [64, 192]):
        edges = [0] + cuts + [T]
        out, busy, power = None, [], []
        for a, b in zip(edges[:-1], edges[1:]):
            m_t = mask_t.view(n_streams, T, -1)[:, a:b].contiguous()
            p_t = spec_t.view(n_streams, T, -1)[:, a:b].contiguous()
            part = _Out(n_streams * (b - a), n_streams, nch, spans, b - a, 2)
            if out is not None:
                part.stats = out.stats
            out = _run(s, m_t, p_t, n_streams * (b - a), spans, b - a, 2, first=(a == 0), out=part)
            st, bu, pw = out.host()
            assert out.pads_untouched()
            busy.append(bu.reshape(n_streams, b - a))
            power.append(pw.reshape(n_streams, b - a, nch))
        assert _ints(st) == _ints(w_st), cuts
        ch.compare(st, w_st, f"cuts {cuts}")
        assert np.concatenate(busy, axis=1).tobytes() == w_busy.tobytes() and np.concatenate(power, axis=1).tobytes() == w_power.tobytes(), cuts
    # first != 0 after garbage equals a call on zeroed records
    zeroed = _Out(n_streams * T, n_streams, nch, spans, T, 2)
    zeroed.stats.zero_()
    z_st = _run(s, mask_t, spec_t, n_streams * T, spans, T, 2, first=False, out=zeroed).host()[0]
    assert z_st.tobytes() == w_st.tobytes()
    # NULL d_busy / d_power: the same records, and the two arrays are left alone
    quiet = _run(s, mask_t, spec_t, n_streams * T, spans, T, 2, busy=False, power=False)
    q_st, q_busy, q_power = quiet.host()
    assert q_st.tobytes() == w_st.tobytes()
    assert (q_busy == 2 ** 64 - 1).all() and (q_power.view(np.uint32) == 0xFFFFFFFF).all() and quiet.pads_untouched()
    # n_epochs = 0 touches nothing, with first != 0 too
    for first in (True, False):
        nothing = _Out(0, n_streams, nch, spans, T, 2)
        s.channels_device(mask_t.data_ptr(), spec_t.data_ptr(), 0, nothing.stats.data_ptr(), nothing.ws.data_ptr(), nothing.ws_bytes, spans,
                          epochs_per_stream=T, min_bins=2, first=first, busy_ptr=nothing.busy.data_ptr(), power_ptr=nothing.power.data_ptr())
        torch.cuda.synchronize()
        assert all((x.cpu().numpy() == 255).all() for x in (nothing.stats, nothing.busy, nothing.power, nothing.ws))
    s.close()


@pytest.mark.parametrize("n", [512, 4096])
def test_agreement_with_the_fused_kernel(built, n):
    """A 64-band Welch plan with CFAR on, channels = its bands, the same min_bins: bit c of d_busy[e] is occupancy[e][c] and the twin's
    n_det on the kernel's mask is band_bins, exactly, on tests/signals.make_epochs traffic."""
    import signals
    k, E, mb = 10, 24, 2
    cfg = cs.cfg_welch(n, k, 64)
    iq, _ = signals.make_epochs(cfg, E, seed=n + 64)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-2, k, W_), mb)
    outs = sgpu.cfar_launch(s, cfg, torch.from_numpy(iq).to(DEV), E)
    spans = cs.channel_spans_from_bands(cfg)
    out = _run(s, outs["mask"], outs["spectrum"], E, spans, E, mb)
    st, busy, power = out.host()
    occ, band_bins = outs["occupancy"].cpu().numpy(), outs["band_bins"].cpu().numpy()
    det = ch.unpack_mask(outs["mask"].cpu().numpy().view(np.uint32), n)
    s.close()
    n_det, want_busy, _ = ch.epochs(det, None, _spans(spans), mb)
    assert (n_det == band_bins).all()
    got_bits = (busy[:, None] >> np.arange(64, dtype=np.uint64)[None, :]) & np.uint64(1)
    assert (got_bits == occ).all() and (busy == want_busy).all()
    print(f"N={n}: {int(occ.sum())} occupied (epoch, band) pairs of {occ.size}, {int(det.sum())} detected bins")
    assert 0 < occ.sum() < occ.size
    assert (st["n_busy"][0] == occ.sum(axis=0)).all()


E2E = {"n": 512, "k": 10, "n_streams": 4, "eps": 500, "pfa": 1e-3, "min_bins": 3, "seed": 2031, "noise_power": 1e-6, "signal_rms": 0.02,
       "tones": 8, "spans": [(300, 10), (496, 32), (55, 30), (189, 33)], "stay": {1: 0.1, 2: 0.5, 3: 0.6}}


def test_end_to_end_markov_chain(built):
    """The intended Markov chain of crn_synth_fill_device_ex (never idle; CH1, CH2 and CH3 are left with probability 0.9, 0.5 and 0.4),
    4 streams x 500 epochs, N = 512, K = 10, rect, CRN_SIG_TONES with 8 tones per band, CA-CFAR guard 2 / train 16 at Pfa 1e-3,
    min_bins 3.  Channel c is band c of the energy plan as one circular interval (CH1 crosses the wrap; channel 0 is the reference band,
    which nobody drives).  A driven band shows 8 detected bins and an idle one at most a false alarm or two (32 bins at Pfa 1e-3: three
    of them in one epoch is a 5e-6 event), so the busy bits are the truth with room to spare: the count of (epoch, channel) pairs that
    differ is printed and capped at 1 %.  The records equal the twin on the kernel's own mask, and the stay probabilities estimated from
    them lie within 4 binomial standard deviations, sqrt(p (1 - p) / n) with n the observed transitions out of busy, of 0.1, 0.5, 0.6."""
    n, k, S, T = E2E["n"], E2E["k"], E2E["n_streams"], E2E["eps"]
    E = S * T
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k)
    iq_t = sgpu.zeros((cs.samples_needed(cfg, E) * 2,), torch.float32)
    truth_t = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    sc = cs.SynthCfg()
    sc.seed, sc.noise_power, sc.signal_rms = E2E["seed"], E2E["noise_power"], E2E["signal_rms"]
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = E2E["tones"], cs.PU_MARKOV_INTENDED, cs.SIG_TONES, S
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), E, cs.samples_per_epoch(cfg), sc, truth_ptr=truth_t.data_ptr())
    s.set_cfar(G_, W_, cs.cfar_alpha(E2E["pfa"], k, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, iq_t, E)
    out = _run(s, outs["mask"], outs["spectrum"], E, E2E["spans"], T, E2E["min_bins"])
    st, busy, power = out.host()
    truth = truth_t.cpu().numpy()
    det = ch.unpack_mask(outs["mask"].cpu().numpy().view(np.uint32), n)
    P = outs["spectrum"].cpu().numpy()
    s.close()
    differ = sum(int((((busy >> np.uint64(c)) & np.uint64(1)).astype(bool) != (truth == c)).sum()) for c in (1, 2, 3))
    print(f"end to end: {differ} of {3 * E} (epoch, channel) pairs differ from the truth (cap {3 * E // 100})")
    assert differ <= 3 * E // 100
    n_det, want_busy, want_power = ch.epochs(det, P, E2E["spans"], E2E["min_bins"])
    assert (busy == want_busy).all()
    ch.compare_power(power, want_power)
    ch.compare(st, ch.update(None, busy, power, T, True), "end to end")
    for c, p in E2E["stay"].items():
        for rows, who in [(st[:, c], "pooled")] + [(st[i: i + 1, c], f"stream {i}") for i in range(S)]:
            n11, n10 = int(rows["n_trans"][:, 1, 1].sum()), int(rows["n_trans"][:, 1, 0].sum())
            est, sd = n11 / (n11 + n10), np.sqrt(p * (1 - p) / (n11 + n10))
            print(f"CH{c} {who}: stays busy {n11} of {n11 + n10}: {est:.4f} against {p} ({abs(est - p) / sd:.2f} standard deviations)")
            assert abs(est - p) <= 4 * sd, (c, who, est, p, sd)
    # what the records are for: the forecast of every channel of stream 0, and the channel to pick
    pick = cs.best_channel(st[0], 5, widths=[w for _, w in E2E["spans"]])
    print("p_idle over 5 epochs, stream 0:", [f"{cs.channel_forecast(st[0, c], 5)[2]:.3f}" for c in range(4)], "best", pick)
    assert pick == 0                                                    # the reference band is never driven


def test_refusals_and_any_handle(built):
    """The refusals that need a live handle; a REF_MAG handle with CFAR off works on an uploaded mask like any other."""
    n, E = 512, 4
    L = cs.lib()
    s = cs.Sensor(cs.cfg_reference())        # REF_MAG, ANN decision: CFAR cannot even be switched on here
    assert s.get_cfar() is None
    rng = np.random.default_rng(0)
    det = rng.random((E, n)) < 0.1
    P = rng.gamma(10.0, 1e-4, (E, n)).astype(np.float32)
    spans = [(n - 3, 7), (40, 8), (0, n)]
    _check(s, det, P, spans, 2, 1, "REF_MAG handle, uploaded mask")
    mask_t, spec_t = _upload(det, P)
    out = _Out(E, 2, 3, spans, 2)

    def rc(m=mask_t.data_ptr(), sp=spec_t.data_ptr(), n_e=E, q=None, stp=out.stats.data_ptr(), bu=out.busy.data_ptr(), pw=out.power.data_ptr(),
           ws=out.ws.data_ptr(), wb=out.ws_bytes, spans=spans, eps=2, mb=1, r=None, nch=None):
        if q is None:
            q = cs.channel_params(spans, eps, mb, True)
            if r is not None:
                q.reserved[r] = 1
            if nch is not None:
                q.n_channels = nch
        v = lambda p: C.c_void_p(p or None)      # noqa: E731
        return L.crn_channels_device(s._h, v(m), v(sp), n_e, C.byref(q) if q != 0 else None, v(stp), v(bu), v(pw), v(ws), wb, None)
    assert rc() == 0
    for bad in ({"m": 0}, {"q": 0}, {"stp": 0}, {"ws": 0}, {"n_e": -1}, {"nch": 0}, {"nch": 65}, {"mb": 0}, {"eps": 0}, {"eps": 3}, {"r": 0}, {"r": 3},
                {"spans": [(-1, 4)]}, {"spans": [(n, 4)]}, {"spans": [(0, 0)]}, {"spans": [(0, n + 1)]}, {"spans": [(0, 8), (0, 8), (511, 513)]},
                {"sp": 0},                                                               # d_power without d_spectrum
                {"m": mask_t.data_ptr() + 4}, {"bu": out.busy.data_ptr() + 4}, {"sp": spec_t.data_ptr() + 8}, {"sp": spec_t.data_ptr() + 4},
                {"stp": out.stats.data_ptr() + 8}, {"pw": out.power.data_ptr() + 8}, {"pw": out.power.data_ptr() + 4},
                {"wb": out.ws_bytes - 1}, {"wb": 0}):
        assert rc(**bad) == cs.CRN_ERR_ARG, bad
        assert b"crn_channels_device" in L.crn_last_error()
    assert rc(sp=0, pw=0) == 0 and rc(bu=0, pw=0) == 0 and rc(n_e=0) == 0 and rc(mb=n + 1) == 0 and rc(spans=[(n - 1, n)]) == 0
    torch.cuda.synchronize()
    s.close()


# CFAR launch + crn_channels_device against the CFAR launch alone, `spectrum` written in both arms: the bar crn_segments_device is held
# to (tests/test_segments_gpu.py: its measured ratio with the relative margin the CA speed test carries, because boxes of the pool
# differ by a few per cent).  Measured on an MI355X (profiles/r11_channels.txt): arm A 392.3 us; one stream of 6656 epochs
# B / A = 1.1555, the three kernels alone 54.7 us; 64 streams of 104 epochs B / A = 1.0993, alone 36.1 us.  The one-stream case meets
# the bar with 0.2 % to spare: what it pays over the 64-stream one is the single join workgroup, 8 waves of 13 dependent summaries each.
SPEED_RATIO = 1.158


def test_cost_next_to_the_cfar_launch(built):
    """N = 4096, K = 10, rect, 64 bands, the 2.18 GB batch; the method of tests/stage_gpu.py (best_of_windows): each timed window holds
    8 launches issued back to back behind one already queued, the arms alternate, 5 windows each after a warm-up, the best counts.  Arm A
    is the CFAR launch alone, arm B the same launch followed by crn_channels_device on the same stream: 64 channels (the plan's bands),
    one stream of 6656 epochs, the hardest case for the time stage, d_busy and d_power NULL.  64 streams of 104 epochs, and the stage
    alone in both layouts, are measured the same way and printed."""
    n, k = 4096, 10
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k, bands=64)
    E = 6656                                  # 6656 x 10 x 4096 x 8 B = 2.18 GB
    # the traffic of every cost test here: tones over unit noise in two epochs of three, so that channels go busy and idle
    iq_t = sgpu.add_tones(sgpu.noise_batch(E, k, n), E, k, n)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, iq_t, E)
    spans = _spans(cs.channel_spans_from_bands(cfg))
    one, many = _Out(E, 1, 64, spans, E), _Out(E, 64, 64, spans, 104)
    torch.cuda.synchronize()

    def arm_a():
        sgpu.cfar_launch(s, cfg, iq_t, E, outs=outs)

    def stage(out, eps):
        _run(s, outs["mask"], outs["spectrum"], E, spans, eps, 1, first=True, out=out, busy=False, power=False)

    def arm_b(out=one, eps=E):
        arm_a()
        stage(out, eps)
    arms = {"A": arm_a, "B one stream": arm_b, "B 64 streams": lambda: arm_b(many, 104), "alone one stream": lambda: stage(one, E),
            "alone 64 streams": lambda: stage(many, 104)}
    times = sgpu.best_of_windows(arms)
    st_one, st_many = one.host()[0], many.host()[0]
    s.close()
    best = {name: min(v) for name, v in times.items()}
    nbytes = E * k * n * 8
    moved = E * (n * 4 + n // 8 + 2 * (8 + 64 * 4))
    print(f"N=4096 K=10 rect 64 bands, {E} epochs ({nbytes / 1e9:.2f} GB), spectrum written: arm A (CFAR launch alone) {best['A']:.4f} ms "
          f"({nbytes / best['A'] / 1e6:.0f} GB/s of input)")
    for name in ("one stream", "64 streams"):
        print(f"  {name:12s} B / A = {best['B ' + name] / best['A']:.4f}   the three kernels alone {best['alone ' + name] * 1e3:.1f} us "
              f"({moved / best['alone ' + name] / 1e6:.0f} GB/s of their own {moved / 1e6:.0f} MB)")
    # the two layouts saw the same epochs
    assert st_one["n_epochs"][0, 0] == E and (st_many["n_epochs"] == 104).all() and (st_one["n_busy"][0] == st_many["n_busy"].sum(axis=0)).all()
    assert st_one["n_busy"][0].max() == E and st_one["n_busy"][0].min() < E // 4       # the band of the steady tones, and one without any
    assert best["B one stream"] <= SPEED_RATIO * best["A"], (best["B one stream"] / best["A"], SPEED_RATIO)
