"""crn_holes_device on the MI355X: the kernels against the twin (tests/holes_f64.py) fed the kernels' own inputs, so the comparison is
exact: d_age, d_free_mask, every integer field, peak_bin and peak_power byte for byte, the slots beyond n_stored zero, memory past every
array still the 0xFF fill; power and floor_mean within 2^-22 relative of the twin's float64 sums (the bound of tests/test_segments_gpu.py,
for the same reason: the twin's value rounded to fp32 is within 2^-24 of it, the kernel's fp64 accumulation in another order differs by
at most width x 2^-53 before its own rounding, and 2^-22 leaves room for a value on a rounding boundary going the other way).  Then the
carry and the NULL outputs, the strong neighbour, cut independence, the free mask fed to crn_channels_device, a known Markov chain end to
end, the refusals that need a live handle, and the cost next to the CFAR launch alone."""
import ctypes as C

import numpy as np
import pytest

import channels_f64 as ch
import crnsense as cs
import holes_f64 as hf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402

G_, W_ = 2, 16
SIZES = (512, 1024, 2048, 4096)
DEFAULTS = {"guard": 0, "min_age": 1, "min_width": 1, "max_holes": 16, "avg_epochs": 1}


class _Out(sgpu.Padded):
    """d_age, the headers, the holes and d_free_mask of a batch on the device, each with 0xFF bytes behind it (stage_gpu.Padded).  The
    workspace is exactly the size the library asks for."""

    def __init__(self, E, n_streams, n, eps, q):
        self.S, self.n, self.mh = n_streams, n, q["max_holes"]
        super().__init__(age=n_streams * n * 4, streams=n_streams * 32, holes=n_streams * self.mh * 32, free=n_streams * n // 8)
        self.ws_bytes = cs.holes_workspace_bytes(E, eps, **q)
        self.ws = torch.full((self.ws_bytes,), 255, dtype=torch.uint8, device=DEV)

    def set_age(self, age):
        raw = np.ascontiguousarray(age, np.int32).view(np.uint8).reshape(-1)
        self.age[: raw.size] = torch.from_numpy(raw.copy()).to(DEV)

    def host(self):
        super().host()
        return (self.view("age", np.int32, (self.S, self.n)), self.view("free", np.uint32, (self.S, self.n // 32)),
                self.view("streams", cs.HOLE_STREAM_DTYPE), self.view("holes", cs.HOLE_DTYPE, (self.S, self.mh)))


def _run(s, mask_t, spec_t, E, eps, q, first=True, out=None, holes=True, free=True):
    n = s.cfg.fft_len
    out = _Out(E, E // eps, n, eps, q) if out is None else out
    s.holes_device(mask_t.data_ptr(), spec_t.data_ptr() if spec_t is not None else 0, E, out.age.data_ptr(), out.streams.data_ptr(),
                   out.ws.data_ptr(), out.ws_bytes, cs.hole_params(eps, first=first, **q), holes_ptr=out.holes.data_ptr() if holes else 0,
                   free_mask_ptr=out.free.data_ptr() if free else 0)
    return out


def _upload(det, P):
    return sgpu.upload_mask(det), None if P is None else sgpu.upload_rows(P)


def _check(s, det, P, eps, what, age0=None, holes=True, free=True, uploaded=None, **kw):
    """The exact comparison on one batch; age0 None: first = 1 on a 0xFF-filled d_age.  Returns ((age, free, streams, holes), worst error)."""
    E, n = det.shape
    q = {**DEFAULTS, **kw}
    mask_t, spec_t = _upload(det, P) if uploaded is None else uploaded
    out = _Out(E, E // eps, n, eps, q)
    if age0 is not None:
        out.set_age(age0)
    _run(s, mask_t, spec_t, E, eps, q, first=age0 is None, out=out, holes=holes, free=free)
    got = out.host()
    assert out.pads_untouched(), (what, "memory behind an output array was written")
    w_age, w_free, w_st, w_holes = hf.run(det, P, eps, age=age0, **q)
    assert got[0].tobytes() == w_age.tobytes(), (what, "d_age", np.argwhere(got[0] != w_age)[:8])
    if free:
        assert got[1].tobytes() == hf.pack_mask(w_free).tobytes(), (what, "d_free_mask")
    else:
        assert (out.raw["free"] == 255).all(), (what, "a NULL d_free_mask was written")
    if not holes:
        assert (out.raw["holes"] == 255).all(), (what, "a NULL d_holes was written")
    worst = hf.compare(got[2], got[3] if holes else None, w_st, w_holes, what)
    return got, worst


def _rows(rng, E, n):
    return (rng.gamma(10.0, 1e-4, (E, n)) * np.where(rng.random((E, n)) < 0.02, 1e4, 1.0)).astype(np.float32)


def _edge_mask(E, n):
    """One blocked bin per epoch and edge: the first and the last bin of a lane piece (N / 64 bins) and of a mask word, a different piece
    and word in every epoch, the row's own two ends among them."""
    B = n // 64
    det = np.zeros((E, n), bool)
    for e in range(E):
        for k in (((e * 5) % 64) * B, ((e * 7 + 3) % 64) * B + B - 1, ((e * 3 + 1) % (n // 32)) * 32, ((e * 11 + 2) % (n // 32)) * 32 + 31,
                  0 if e % 4 == 1 else n - 1 if e % 4 == 3 else n // 2):
            det[e, k] = True
    return det


# every value of the issue's parameter lists in some set; `late` stands for T + 1 (no bin can be that old after a first call)
PARAM_SETS = [{"guard": 0, "min_age": 1, "min_width": 1, "max_holes": 256, "avg_epochs": 1},
              {"guard": 1, "min_age": 8, "min_width": 8, "max_holes": 4, "avg_epochs": 8},
              {"guard": 2, "min_age": 1, "min_width": 8, "max_holes": 1, "avg_epochs": 64},
              {"guard": 31, "min_age": 8, "min_width": 1, "max_holes": 4, "avg_epochs": 8},
              {"guard": 32, "min_age": 1, "min_width": 1, "max_holes": 256, "avg_epochs": 64},
              {"guard": 2, "min_age": "late", "min_width": 1, "max_holes": 4, "avg_epochs": 1},
              {"guard": 0, "min_age": 1, "min_width": "n", "max_holes": 1, "avg_epochs": 8}]


@pytest.mark.parametrize("S,T", [(1, 1), (1, 63), (1, 64), (3, 65), (1, 129), (2, 200)])
@pytest.mark.parametrize("n", SIZES)
def test_shapes_against_twin(built, n, S, T):
    """Random masks of density 0, 0.002, 0.5 and 1 and the edge mask; every parameter set; stream lengths on, under and over the chunk
    edges of the last-blocked kernel.  Density 0.002 leaves bins that only an earlier chunk row resolves, and some that none does."""
    rng = np.random.default_rng(n + 31 * S + T)
    E = S * T
    P = _rows(rng, E, n)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    worst, most = 0.0, 0
    masks = [(f"density {d}", rng.random((E, n)) < d) for d in (0.0, 0.002, 0.5, 1.0)] + [("edges", _edge_mask(E, n))]
    for name, det in masks:
        up = _upload(det, P)
        for q in PARAM_SETS:
            q = {k: (T + 1 if v == "late" else n if v == "n" else v) for k, v in q.items()}
            got, w = _check(s, det, P, T, f"N={n} {S}x{T} {name} {q}", uploaded=up, **q)
            worst, most = max(worst, w), max(most, int(got[2]["n_found"].max()))
    s.close()
    print(f"N={n} {S}x{T}: most holes found in a stream {most}; widest relative error of power / floor_mean {worst:.2e} (bound {hf.REL_TOL:.2e})")


@pytest.mark.parametrize("n", [512, 4096])
def test_carry_and_null_outputs(built, n):
    rng = np.random.default_rng(n + 5)
    S, T = 2, 70
    det = rng.random((S * T, n)) < 0.004
    det[:, 100:140] = False                                   # bins no epoch of the batch blocks: their age is the carry's + T
    P = _rows(rng, S * T, n)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    q = {"guard": 1, "min_age": 8, "min_width": 4, "max_holes": 8, "avg_epochs": 8}
    fresh, _ = _check(s, det, P, T, "first after 0xFF garbage", **q)
    zeroed, _ = _check(s, det, P, T, "a zeroed d_age", age0=np.zeros((S, n), np.int32), **q)
    for a, b in zip(fresh, zeroed):
        assert a.tobytes() == b.tobytes()
    # a fabricated carry: close to 2^31 - 1 (saturates), negative (counts as 0), ordinary
    age0 = rng.integers(0, 1000, (S, n)).astype(np.int32)
    age0[:, 100:110] = 2 ** 31 - 1 - np.arange(10) * 10
    age0[:, 110:120] = -1 - np.arange(10) * 1000
    age0[:, 120] = -2 ** 31
    got, _ = _check(s, det, P, T, "fabricated carry", age0=age0, **q)
    assert (got[0][:, 100:107] == 2 ** 31 - 1).all() and (got[0][:, 107:110] == 2 ** 31 - 1 - np.arange(7, 10) * 10 + T).all()
    assert (got[0][:, 110:121] == T).all()
    # NULL d_spectrum, d_holes, d_free_mask: the other outputs do not change
    for kw in ({"holes": False}, {"free": False}, {"holes": False, "free": False}):
        quiet, _ = _check(s, det, P, T, f"NULL outputs {kw}", **kw, **q)
        assert quiet[0].tobytes() == fresh[0].tobytes() and quiet[2].tobytes() == fresh[2].tobytes()
        if "holes" not in kw:
            assert quiet[3].tobytes() == fresh[3].tobytes()
        if "free" not in kw:
            assert quiet[1].tobytes() == fresh[1].tobytes()
    dark, _ = _check(s, det, None, T, "NULL d_spectrum", **q)
    assert dark[0].tobytes() == fresh[0].tobytes() and dark[1].tobytes() == fresh[1].tobytes()
    for f in hf.STREAM_INTS:
        assert (dark[2][f] == fresh[2][f]).all()
    for f in ("lo", "width", "age", "age_max"):
        assert (dark[3][f] == fresh[3][f]).all()
    assert (dark[3]["peak_bin"] == dark[3]["lo"]).all() and not dark[3]["power"].any() and not dark[3]["peak_power"].any() and not dark[2]["floor_mean"].any()
    # n_epochs = 0 touches nothing, with first != 0 too
    mask_t, spec_t = _upload(det, P)
    for first in (True, False):
        nothing = _Out(0, S, n, T, {**DEFAULTS, **q})
        s.holes_device(mask_t.data_ptr(), spec_t.data_ptr(), 0, nothing.age.data_ptr(), nothing.streams.data_ptr(), nothing.ws.data_ptr(),
                       nothing.ws_bytes, cs.hole_params(T, first=first, **q), holes_ptr=nothing.holes.data_ptr(), free_mask_ptr=nothing.free.data_ptr())
        torch.cuda.synchronize()
        assert all((x.cpu().numpy() == 255).all() for x in (nothing.age, nothing.streams, nothing.holes, nothing.free, nothing.ws))
    s.close()


@pytest.mark.parametrize("n", [512, 4096])
def test_strong_neighbour(built, n):
    """A row value 90 dB over the floor one bin outside a hole leaves the hole's power within the bound; the same value one bin inside
    becomes its peak_power.  Holes on and off the lane-piece edges, inside one piece, and across the wrap (the hole that contains bin 0)."""
    rng = np.random.default_rng(n + 90)
    B, T = n // 64, 4
    spans = [(3 * B, B), (7 * B + 1, B - 2), (9 * B - 2, 2 * B + 5), (20 * B, 10 * B), (n - 4, 8)]       # the holes
    det = np.ones((T, n), bool)
    for lo, w in spans:
        det[:, (lo + np.arange(w)) % n] = False
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    for inside in (False, True):
        P = rng.gamma(10.0, 1e-4, (T, n))
        loud = {}
        for lo, w in spans:
            for k in ((lo, lo + w - 1) if inside else (lo - 1, lo + w)):
                P[:, k % n] = 1e-3 * 1e9 * rng.uniform(0.5, 2.0, T)
            loud[lo] = [k % n for k in ((lo, lo + w - 1) if inside else (lo - 1, lo + w))]
        P = P.astype(np.float32)
        got, worst = _check(s, det, P, T, f"strong neighbour N={n} inside={inside}", avg_epochs=4)
        st, holes = got[2][0], got[3][0]
        assert st["n_found"] == len(spans) and sorted((int(h["lo"]), int(h["width"])) for h in holes[: len(spans)]) == sorted(spans)
        pb = hf.pbar(P, 4)
        for h in holes[: len(spans)]:
            if inside:
                assert h["peak_bin"] in loud[int(h["lo"])] and h["peak_power"] == pb[loud[int(h["lo"])]].max() > 1e5
            else:
                assert h["peak_power"] < 1.0 and h["power"] < 1.0       # nothing of a 1e6 neighbour reached the sum
        print(f"N={n} loud bins {'inside' if inside else 'outside'}: widest relative error {worst:.2e} (bound {hf.REL_TOL:.2e})")
    s.close()


def _ints(got):
    """d_age, d_free_mask and every integer field that does not come from Pbar (peak_bin does: it goes with the floats)."""
    return got[0].tobytes() + got[1].tobytes() + b"".join(np.ascontiguousarray(got[2][f]).tobytes() for f in hf.STREAM_INTS) + \
        b"".join(np.ascontiguousarray(got[3][f]).tobytes() for f in hf.HOLE_INTS if f != "peak_bin")


@pytest.mark.parametrize("n", [512, 4096])
def test_cut_independence(built, n):
    """(S = 3, T = 200) in one call against the same epochs in several calls (first = 1, then 0): cut at 1 epoch, inside a chunk, on the
    chunk edges, and into its streams.  d_age, d_free_mask and the integers byte for byte; the floats, and peak_bin with them, where the
    last piece has T >= avg_epochs (every cut but the last two, whose last pieces of 7 and 1 epochs average other rows)."""
    rng = np.random.default_rng(n + 3)
    S, T = 3, 200
    det = rng.random((S * T, n)) < 0.003
    det[:, 50:90] = rng.random((S * T, 1)) < 0.05                # a channel that comes and goes
    P = _rows(rng, S * T, n)
    q = {"guard": 2, "min_age": 8, "min_width": 8, "max_holes": 16, "avg_epochs": 8}
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    mask_t, spec_t = _upload(det, P)
    whole, _ = _check(s, det, P, T, "whole", uploaded=(mask_t, spec_t), **q)
    for cuts in ([1], [37], [64], [128], [64, 128], [1, 37, 64, 128, 193], [199]):
        edges = [0] + cuts + [T]
        out = None
        for a, b in zip(edges[:-1], edges[1:]):
            m_t = mask_t.view(S, T, -1)[:, a:b].contiguous()
            p_t = spec_t.view(S, T, -1)[:, a:b].contiguous()
            part = _Out(S * (b - a), S, n, b - a, q)
            if out is not None:
                part.age = out.age
            out = _run(s, m_t, p_t, S * (b - a), b - a, q, first=(a == 0), out=part)
            got = out.host()
            assert out.pads_untouched()
        assert _ints(got) == _ints(whole), cuts
        if edges[-1] - edges[-2] >= q["avg_epochs"]:
            assert got[2].tobytes() == whole[2].tobytes() and got[3].tobytes() == whole[3].tobytes(), cuts
    # into its streams: each stream alone gives its own rows of the batch
    for i in range(S):
        one, _ = _check(s, det[i * T: (i + 1) * T], P[i * T: (i + 1) * T], T, f"stream {i} alone", **q)
        assert one[0].tobytes() == whole[0][i: i + 1].tobytes() and one[1].tobytes() == whole[1][i: i + 1].tobytes()
        assert one[2].tobytes() == whole[2][i: i + 1].tobytes() and one[3].tobytes() == whole[3][i: i + 1].tobytes()
    s.close()


def test_free_mask_feeds_the_channel_stage(built):
    """A real CFAR launch (Welch 64-band plan, N = 512), 6 streams of 4 epochs: d_free_mask, one row per stream, goes to
    crn_channels_device as a batch of 6 epochs and gives what that stage gives on the twin's free mask."""
    import signals
    n, k, S, T = 512, 10, 6, 4
    E = S * T
    cfg = cs.cfg_welch(n, k, 64)
    iq, _ = signals.make_epochs(cfg, E, seed=n + 14)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-2, k, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, torch.from_numpy(iq).to(DEV), E)
    q = {**DEFAULTS, "guard": 1, "min_age": 2}
    out = _run(s, outs["mask"], outs["spectrum"], E, T, q)
    age, free, st, holes = out.host()
    det = hf.unpack_mask(outs["mask"].cpu().numpy().view(np.uint32), n)
    w_age, w_free, w_st, w_holes = hf.run(det, outs["spectrum"].cpu().numpy(), T, **q)
    assert age.tobytes() == w_age.tobytes() and free.tobytes() == hf.pack_mask(w_free).tobytes()
    hf.compare(st, holes, w_st, w_holes, "on a CFAR launch")
    assert 0 < st["free_bins"].sum() < S * n
    spans = [(sp.lo, sp.width) for sp in cs.channel_spans_from_bands(cfg)]

    def channels(mask_ptr):
        nb = cs.channels_workspace_bytes(S, spans, S, 4)
        stats = torch.full((64 * 192,), 255, dtype=torch.uint8, device=DEV)
        busy = torch.full((S * 8,), 255, dtype=torch.uint8, device=DEV)
        ws = torch.full((nb,), 255, dtype=torch.uint8, device=DEV)
        s.channels_device(mask_ptr, 0, S, stats.data_ptr(), ws.data_ptr(), nb, spans, epochs_per_stream=S, min_bins=4, first=True, busy_ptr=busy.data_ptr())
        torch.cuda.synchronize()
        return stats.cpu().numpy().tobytes(), busy.cpu().numpy().tobytes()
    twin_t = torch.from_numpy(hf.pack_mask(w_free).view(np.int32)).to(DEV)
    assert channels(out.free.data_ptr()) == channels(twin_t.data_ptr())
    _, want_busy, _ = ch.epochs(w_free, None, spans, 4)
    assert channels(out.free.data_ptr())[1] == want_busy.tobytes()
    s.close()


# the traffic of tests/test_channels_gpu.py's end-to-end test
E2E = {"n": 512, "k": 10, "n_streams": 4, "eps": 500, "pfa": 1e-3, "seed": 2031, "noise_power": 1e-6, "signal_rms": 0.02, "tones": 8,
       "spans": [(300, 10), (496, 32), (55, 30), (189, 33)], "guard": 2, "min_age": 8, "min_width": 8, "piece": 20}
COVERAGE_BAR = 0.85              # tests/test_holes_host.py::test_coverage_simulation


def test_end_to_end_markov_chain(built):
    """The intended Markov chain of crn_synth_fill_device_ex (never idle; one of CH1, CH2, CH3 is driven in every epoch), 4 streams x 500
    epochs, N = 512, K = 10, rect, 8 tones per band, CA-CFAR guard 2 / train 16 at Pfa 1e-3; holes with guard 2, min_age 8, min_width 8.
    The stage is called on pieces of 20 epochs (first = 1, then 0), so the holes are looked at 25 times per stream.  A bin is truly idle
    when it lies in no channel whose truth was busy in the last 8 epochs.  At most 1 % of all stored hole bins may lie in such a channel
    (the cap of the channels test, whose traffic gave 0 of 6000), and the stored holes must cover at least 0.85 of the truly idle bins,
    pooled (the bar the host simulation justifies).  Every piece equals the twin on the kernel's own mask."""
    n, k, S, T, piece = E2E["n"], E2E["k"], E2E["n_streams"], E2E["eps"], E2E["piece"]
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
    truth = truth_t.cpu().numpy().reshape(S, T)
    det = hf.unpack_mask(outs["mask"].cpu().numpy().view(np.uint32), n).reshape(S, T, n)
    q = {"guard": E2E["guard"], "min_age": E2E["min_age"], "min_width": E2E["min_width"], "max_holes": 16, "avg_epochs": 8}
    out, w_age = None, None
    stored = wrong = idle_bins = covered = 0
    for a in range(0, T, piece):
        m_t = outs["mask"].view(S, T, -1)[:, a: a + piece].contiguous()
        p_t = outs["spectrum"].view(S, T, -1)[:, a: a + piece].contiguous()
        part = _Out(S * piece, S, n, piece, q)
        if out is not None:
            part.age = out.age
        out = _run(s, m_t, p_t, S * piece, piece, q, first=(a == 0), out=part)
        age, free, st, holes = out.host()
        assert out.pads_untouched()
        w_age, w_free, w_st, w_holes = hf.run(det[:, a: a + piece].reshape(-1, n), p_t.cpu().numpy().reshape(-1, n), piece, age=w_age, **q)
        assert age.tobytes() == w_age.tobytes() and free.tobytes() == hf.pack_mask(w_free).tobytes()
        hf.compare(st, holes, w_st, w_holes, f"end to end, epochs {a}..{a + piece - 1}")
        assert (st["n_found"] == st["n_stored"]).all()
        for i in range(S):
            truly_idle = np.ones(n, bool)
            for c in (1, 2, 3):
                if (truth[i, a + piece - E2E["min_age"]: a + piece] == c).any():
                    lo, w = E2E["spans"][c]
                    truly_idle[(lo + np.arange(w)) % n] = False
            inside = np.zeros(n, bool)
            for h in holes[i, : st[i]["n_stored"]]:
                inside[(h["lo"] + np.arange(h["width"])) % n] = True
            stored += int(inside.sum())
            wrong += int((inside & ~truly_idle).sum())
            idle_bins += int(truly_idle.sum())
            covered += int((inside & truly_idle).sum())
    s.close()
    print(f"end to end: {wrong} of {stored} stored hole bins lie in a channel busy in the last {E2E['min_age']} epochs (cap {stored // 100}); "
          f"{covered} of {idle_bins} truly idle bins covered: {covered / idle_bins:.4f} (bar {COVERAGE_BAR})")
    assert wrong <= stored // 100
    assert covered / idle_bins >= COVERAGE_BAR


def test_refusals_with_a_live_handle(built):
    """The refusals that need a live handle; a REF_MAG handle with CFAR off works on an uploaded mask like any other."""
    n, S, T = 512, 2, 3
    E = S * T
    L = cs.lib()
    s = cs.Sensor(cs.cfg_reference())
    rng = np.random.default_rng(0)
    det = rng.random((E, n)) < 0.01
    P = _rows(rng, E, n)
    _check(s, det, P, T, "REF_MAG handle, uploaded mask", guard=1, min_age=2)
    mask_t, spec_t = _upload(det, P)
    out = _Out(E, S, n, T, DEFAULTS)

    def rc(m=mask_t.data_ptr(), sp=spec_t.data_ptr(), n_e=E, q=None, ag=out.age.data_ptr(), stp=out.streams.data_ptr(), ho=out.holes.data_ptr(),
           fr=out.free.data_ptr(), ws=out.ws.data_ptr(), wb=out.ws_bytes, eps=T, reserved=0, **kw):
        if q is None:
            q = cs.hole_params(eps, **{**DEFAULTS, **kw})
            q.reserved = reserved
        v = lambda p: C.c_void_p(p or None)      # noqa: E731
        return L.crn_holes_device(s._h, v(m), v(sp), n_e, C.byref(q) if q != 0 else None, v(ag), v(stp), v(ho), v(fr), v(ws), wb, None)
    assert rc() == 0
    for bad in ({"m": 0}, {"q": 0}, {"ag": 0}, {"stp": 0}, {"ws": 0}, {"n_e": -1}, {"eps": 0}, {"eps": 4}, {"guard": -1}, {"guard": 33},
                {"min_age": 0}, {"min_width": 0}, {"min_width": n + 1}, {"max_holes": 0}, {"max_holes": 257}, {"avg_epochs": 0}, {"avg_epochs": 65},
                {"reserved": 1},
                {"m": mask_t.data_ptr() + 4}, {"fr": out.free.data_ptr() + 4}, {"ws": out.ws.data_ptr() + 4}, {"sp": spec_t.data_ptr() + 8},
                {"sp": spec_t.data_ptr() + 4}, {"ag": out.age.data_ptr() + 8}, {"stp": out.streams.data_ptr() + 8}, {"ho": out.holes.data_ptr() + 8},
                {"wb": S * n - 1}, {"wb": 0}):
        assert rc(**bad) == cs.CRN_ERR_ARG, bad
        assert b"crn_holes_device" in L.crn_last_error()
    # the workspace the handle's own fft_len needs is enough: one byte per bin and (stream, chunk)
    assert rc(wb=S * n) == 0 and rc(sp=0) == 0 and rc(ho=0, fr=0) == 0 and rc(n_e=0) == 0 and rc(min_width=n, min_age=2 ** 31 - 1) == 0
    torch.cuda.synchronize()
    s.close()


# CFAR launch + crn_holes_device against the CFAR launch alone, `spectrum` written in both arms: the bar the project holds its post-CFAR
# stages to (tests/test_channels_gpu.py, tests/test_segments_gpu.py).  Measured on an MI355X (profiles/r14_holes.txt): arm A
# 424.1 us; one stream of 6656 epochs B / A = 1.1061, the two kernels alone 40.7 us; 64 streams of 104 epochs B / A = 1.0739, alone 27.5 us.
SPEED_RATIO = 1.158


def test_cost_next_to_the_cfar_launch(built):
    """N = 4096, K = 10, rect, 64 bands, the 2.18 GB batch; the method of tests/stage_gpu.py (best_of_windows): each timed window holds
    8 launches issued back to back behind one already queued, the arms alternate, 5 windows each after a warm-up, the best counts.  Arm A
    is the CFAR launch alone, arm B the same launch followed by crn_holes_device on the same stream with all outputs, guard 2, min_age 8,
    min_width 8, max_holes 16, avg_epochs 8: one stream of 6656 epochs, and 64 streams of 104.  Both layouts are held to the bar; the
    stage alone is measured the same way and printed."""
    n, k = 4096, 10
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k, bands=64)
    E = 6656                                  # 6656 x 10 x 4096 x 8 B = 2.18 GB
    # the traffic of every cost test here: tones over unit noise in two epochs of three
    iq_t = sgpu.add_tones(sgpu.noise_batch(E, k, n), E, k, n)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, iq_t, E)
    q = {"guard": 2, "min_age": 8, "min_width": 8, "max_holes": 16, "avg_epochs": 8}
    one, many = _Out(E, 1, n, E, q), _Out(E, 64, n, 104, q)
    torch.cuda.synchronize()

    def arm_a():
        sgpu.cfar_launch(s, cfg, iq_t, E, outs=outs)

    def stage(out, eps):
        _run(s, outs["mask"], outs["spectrum"], E, eps, q, first=True, out=out)

    def arm_b(out=one, eps=E):
        arm_a()
        stage(out, eps)
    arms = {"A": arm_a, "B one stream": arm_b, "B 64 streams": lambda: arm_b(many, 104), "alone one stream": lambda: stage(one, E),
            "alone 64 streams": lambda: stage(many, 104)}
    times = sgpu.best_of_windows(arms)
    g_one, g_many = one.host(), many.host()
    assert one.pads_untouched() and many.pads_untouched()
    det = hf.unpack_mask(outs["mask"].cpu().numpy().view(np.uint32), n)
    s.close()
    best = {name: min(v) for name, v in times.items()}
    nbytes = E * k * n * 8
    print(f"N=4096 K=10 rect 64 bands, {E} epochs ({nbytes / 1e9:.2f} GB), spectrum written: arm A (CFAR launch alone) {best['A']:.4f} ms "
          f"({nbytes / best['A'] / 1e6:.0f} GB/s of input)")
    for name in ("one stream", "64 streams"):
        print(f"  {name:12s} B / A = {best['B ' + name] / best['A']:.4f}   the two kernels alone {best['alone ' + name] * 1e3:.1f} us")
    # both layouts computed what the definition says: the ages against the twin's closed form on the kernel's own mask
    assert g_one[0].tobytes() == hf.ages(det, 2)[None, :].tobytes()
    assert g_many[0].tobytes() == np.stack([hf.ages(det[i * 104: (i + 1) * 104], 2) for i in range(64)]).tobytes()
    assert g_one[2]["n_found"][0] > 0 and (g_many[2]["free_bins"] > 0).all()
    assert best["B 64 streams"] <= SPEED_RATIO * best["A"], (best["B 64 streams"] / best["A"], SPEED_RATIO)
    assert best["B one stream"] <= SPEED_RATIO * best["A"], (best["B one stream"] / best["A"], SPEED_RATIO)
