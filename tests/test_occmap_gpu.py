"""crn_occmap_device on the MI355X: the kernels against the twin (tests/occmap_f64.py) fed the kernels' own inputs, so the comparison is
exact: every integer field of every record, state, max_hold and min_hold, the usual mask and the headers equal byte for byte, memory
past the arrays still the 0xFF fill; power[] within n_epochs x 2^-52 relative of the twin's exactly rounded sum (the bound of an fp64 sum
of n non-negative terms in any order).  Hand-made columns around the 64-epoch chunks, the values a row can hold, cuts, the carries the
stage must survive, the stage behind the CFAR launch and in front of crn_segments_device, determinism, the refusals that need a live
handle, the generator end to end, and the cost next to the CFAR launch alone."""
import ctypes as C

import numpy as np
import pytest

import crnsense as cs
import occmap_cases as oc
import occmap_f64 as om

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402

G_, W_ = 2, 16
SIZES = (512, 1024, 2048, 4096)


class _Out(sgpu.Padded):
    """The records, headers and usual mask of a batch on the device, each with 0xFF bytes behind it (stage_gpu.Padded).  The workspace is
    exactly the size the library asks for."""

    def __init__(self, E, S, n, eps):
        self.E, self.S, self.n = E, S, n
        super().__init__(bins=S * n * 64, streams=S * 32, usual=S * n // 8)
        self.ws_bytes = cs.occmap_workspace_bytes(E, eps)
        self.ws = torch.full((self.ws_bytes,), 255, dtype=torch.uint8, device=DEV)

    def carry(self, bins):
        raw = np.ascontiguousarray(bins).view(np.uint8).reshape(-1)
        self.bins[: raw.size] = torch.from_numpy(raw.copy()).to(DEV)

    def host(self):
        super().host()
        return (self.view("bins", cs.OCCMAP_BIN_DTYPE, (self.S, self.n)), self.view("streams", cs.OCCMAP_STREAM_DTYPE),
                self.view("usual", np.uint32, (self.S, self.n // 32)))


def _run(s, mask_t, spec_t, E, eps, duty_ppm=500000, first=True, out=None, n=None, usual=True):
    out = _Out(E, E // eps, n, eps) if out is None else out
    s.occmap_device(mask_t.data_ptr(), spec_t.data_ptr() if spec_t is not None else 0, E, out.bins.data_ptr(), out.streams.data_ptr(),
                    out.ws.data_ptr(), out.ws_bytes, epochs_per_stream=eps, duty=duty_ppm / 1e6, first=first,
                    usual_mask_ptr=out.usual.data_ptr() if usual else 0)
    return out


def _same(out, want, duty_ppm, what):
    """The device's outputs against the twin's records `want`: returns (records, the largest power error in units of the bound)."""
    bins, streams, usual = out.host()
    assert out.pads_untouched(), (what, "memory behind an output array was written")
    worst = om.compare(bins, want, what)
    w_streams, w_usual = om.headers(want, duty_ppm)
    assert streams.tobytes() == w_streams.tobytes(), (what, "headers", streams, w_streams)
    assert usual.tobytes() == w_usual.tobytes(), (what, "usual mask", np.argwhere(usual != w_usual)[:6].tolist())
    return bins, worst


# ---- 1. hand-made columns ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", oc.LENGTHS)
@pytest.mark.parametrize("n", SIZES)
def test_hand_made_columns_against_twin(built, n, T):
    """tests/occmap_cases.py, hand_made: sixteen column patterns by bin index mod 16, shifted by one bin from stream to stream (S = 3);
    stream lengths on and around the 64-epoch chunks.  Gamma(10) rows and rows quantised to quarters, and no rows at all; duty_ppm 1,
    500000 and 1000000."""
    S = 3
    E = S * T
    det = oc.hand_made(n, S, T)
    mask_t = sgpu.upload_mask(det)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    worst = 0.0
    for kind in ("gamma", "quarters", None):
        P = None if kind is None else oc.rows(n + T, E, n, quantised=kind == "quarters")
        spec_t = None if P is None else sgpu.upload_rows(P)
        want = om.update(None, det, P, T, True)
        for duty_ppm in (1, 500000, 1000000):
            out = _run(s, mask_t, spec_t, E, T, duty_ppm, n=n)
            bins, w = _same(out, want, duty_ppm, f"N={n} T={T} {kind} duty {duty_ppm}")
            worst = max(worst, w)
        if P is None:
            assert not bins["power"].any() and not bins["max_hold"].any() and not bins["min_hold"].any()
    s.close()
    assert (bins["n_epochs"] == T).all() and (bins["n_busy"] == det.reshape(S, T, n).sum(axis=1)).all()
    print(f"N={n} T={T}: largest power error {worst:.3f} of the bound; most rises of a bin {int(bins['n_rise'].max())}, longest completed run "
          f"{int(bins['run_max'].max())}")


# ---- 2. values a row can hold -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 4096])
def test_values_a_row_can_hold(built, n):
    """Columns of 0.0, subnormals, +inf, NaN and -1.0 (tests/occmap_cases.py, special_rows): max_hold and min_hold follow the bit-pattern
    rule exactly, power[] is NaN or inf exactly where the twin's is, and the neighbouring columns are unaffected (om.compare holds every
    column)."""
    T, S = 70, 2
    rng = np.random.default_rng(n)
    det = rng.random((S * T, n)) < 0.3
    P = np.concatenate([oc.special_rows(n, T, seed=j)[0] for j in range(S)])
    where = oc.special_rows(n, T)[1]
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    out = _run(s, sgpu.upload_mask(det), sgpu.upload_rows(P), S * T, T, n=n)
    bins, _ = _same(out, om.update(None, det, P, T, True), 500000, f"special values N={n}")
    s.close()
    for k, v in where.items():
        bits = int(np.float32(v).view(np.uint32))
        assert (om.bits_of(bins["max_hold"][:, k]) == bits).all() and (om.bits_of(bins["min_hold"][:, k]) == bits).all(), (k, v)
    assert np.isinf(bins["max_hold"][:, 100]).all() and np.isnan(bins["max_hold"][:, 101]).all()
    assert np.isnan(bins["power"][:, 101]).sum() == S and np.isinf(bins["power"][:, 100]).sum() == S        # one of the two sums each
    assert np.isfinite(bins["power"][:, [99, 102]]).all() and (bins["min_hold"][:, 300] == 0).all()


# ---- 3. cuts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 4096])
def test_cut_independence(built, n):
    """T = 193 in one call against calls of 1, 2, 61, 1, 64 and 64 epochs per stream (first = 1, then 0): everything but power[] the same
    bytes, the usual mask and the headers too; power[] within the bound of the twin's sum."""
    S, T = 3, 193
    det = oc.hand_made(n, S, T, seed=12)
    P = oc.rows(n, S * T, n)
    mask_t, spec_t = sgpu.upload_mask(det), sgpu.upload_rows(P)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    want = om.update(None, det, P, T, True)
    whole = _run(s, mask_t, spec_t, S * T, T, 300000, n=n)
    w_bins, _ = _same(whole, want, 300000, "whole")
    out, a = None, 0
    for c in oc.CUTS:
        m_t = mask_t.view(S, T, -1)[:, a: a + c].contiguous()
        p_t = spec_t.view(S, T, -1)[:, a: a + c].contiguous()
        part = _Out(S * c, S, n, c)
        if out is not None:
            part.bins = out.bins
        out = _run(s, m_t, p_t, S * c, c, 300000, first=(a == 0), out=part)
        a += c
    bins, _ = _same(out, want, 300000, f"cuts {oc.CUTS}")
    s.close()
    assert om.exact_bytes(bins) == om.exact_bytes(w_bins)
    assert whole.raw["streams"].tobytes() == out.raw["streams"].tobytes() and whole.raw["usual"].tobytes() == out.raw["usual"].tobytes()


# ---- 4. carries -------------------------------------------------------------------------------------------------------------------
def test_carries_the_stage_must_survive(built):
    """tests/occmap_cases.py, carries: 0xFF bytes and n_epochs = -5 with garbage around it (both taken as empty), run = -7 (taken as 0),
    state = 0x7ffffffe (only bit 0 is read), and n_epochs = n_busy = run = 2^31 - 3 followed by five busy epochs (all three saturate at
    2^31 - 1, run_max unchanged).  The output is exactly the twin's, the pads are untouched."""
    n, T = 512, 5
    carry = oc.carries(n)
    rng = np.random.default_rng(4)
    det = rng.random((T, n)) < 0.5
    det[:, 256:320] = True                                        # five busy epochs behind the saturating busy carry
    det[:, 320:384] = False
    P = oc.rows(4, T, n)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    for spec in (P, None):
        out = _Out(T, 1, n, T)
        out.carry(carry)
        _run(s, sgpu.upload_mask(det), None if spec is None else sgpu.upload_rows(spec), T, T, first=False, out=out)
        bins, _ = _same(out, om.update(carry, det, spec, T, False), 500000, "carries")
    s.close()
    fresh = om.update(None, det, None, T, True)
    assert om.exact_bytes(bins[:, :128]) == om.exact_bytes(fresh[:, :128])
    sat = bins[0, 256:320]
    assert (sat["n_epochs"] == om.SAT).all() and (sat["n_busy"] == om.SAT).all() and (sat["run"] == om.SAT).all() and (sat["run_max"] == (9, 6)).all()
    assert (bins["n_epochs"][0, 320:384] == om.SAT).all() and (bins["n_busy"][0, 320:384] == 7).all() and (bins["run"][0, 320:384] == om.SAT).all()
    assert (bins["n_epochs"][0, 128:256] == 45).all() and (bins["state"][0, 128:256] == det[-1, 128:256]).all()


# ---- 5. behind the CFAR launch ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [512, 4096])
def test_behind_the_cfar_launch(built, n):
    """tests/signals.make_epochs traffic, CA-CFAR at Pfa 1e-2, then this stage on the launch's own mask and `spectrum` (the twin is fed
    the device's arrays); the usual mask then goes through crn_segments_device with the streams' last rows, and the segments equal the
    segment twin's for that mask."""
    import segments_f64 as sf
    import signals
    k, S, T = 10, 2, 40
    E = S * T
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k)
    iq, _ = signals.make_epochs(cfg, E, seed=n + 19)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-2, k, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, torch.from_numpy(iq).to(DEV), E)
    out = _run(s, outs["mask"], outs["spectrum"], E, T, 150000, n=n)
    det = om.unpack_mask(outs["mask"].cpu().numpy(), n)
    P = outs["spectrum"].cpu().numpy()
    bins, _ = _same(out, om.update(None, det, P, T, True), 150000, f"behind the CFAR launch N={n}")
    usual = om.unpack_mask(out.raw["usual"].view(np.uint32), n)
    print(f"N={n}: {int(det.sum())} detected bins in {E} epochs; usual bins per stream {usual.sum(axis=1).tolist()}, clear bins "
          f"{out.view('streams', cs.OCCMAP_STREAM_DTYPE)['clear_bins'].tolist()}")
    assert 0 < usual.sum() < usual.size
    last = outs["spectrum"].view(S, T, n)[:, T - 1].contiguous()
    seg = sgpu.Padded(epochs=S * 16, segments=S * 16 * 32)
    s.segments_device(out.usual.data_ptr(), last.data_ptr(), S, seg.epochs.data_ptr(), seg.segments.data_ptr(), merge_gap=2, max_segments=16)
    seg.host()
    s.close()
    assert seg.pads_untouched()
    w_epochs, w_segments = sf.run(usual, last.cpu().numpy(), 2, 1, 16)
    sf.compare(seg.view("epochs", cs.SEGMENT_EPOCH_DTYPE), seg.view("segments", cs.SEGMENT_DTYPE, (S, 16)), w_epochs, w_segments)
    assert seg.view("epochs", cs.SEGMENT_EPOCH_DTYPE)["n_found"].min() >= 1


# ---- 6. determinism ---------------------------------------------------------------------------------------------------------------
def test_the_same_call_twice_gives_the_same_bytes(built):
    """Two streams of 1100 epochs, 18 chunks: the join folds them as three shares of six in three waves that meet in LDS (the lengths of
    the hand-made test are one share).  The same call twice into fresh outputs gives identical bytes, power[] included, and they are
    the twin's."""
    n, S, T = 1024, 2, 1100
    rng = np.random.default_rng(6)
    det, P = rng.random((S * T, n)) < rng.random(n)[None, :], oc.rows(6, S * T, n)
    mask_t, spec_t = sgpu.upload_mask(det), sgpu.upload_rows(P)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    outs = [_run(s, mask_t, spec_t, S * T, T, n=n) for _ in range(2)]
    a, b = (out.host() for out in outs)
    s.close()
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert a[0]["power"].any() and (a[0]["n_epochs"] == T).all()
    _same(outs[0], om.update(None, det, P, T, True), 500000, "three shares")


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------
def test_refusals_with_a_live_handle(built):
    """Every refusal of the header's list; the message names the function; a refused call and n_epochs = 0 leave every output as it
    was.  A REF_MAG handle with CFAR off serves an uploaded mask like any other."""
    n, E = 512, 4
    L = cs.lib()
    s = cs.Sensor(cs.cfg_reference())
    rng = np.random.default_rng(0)
    det = rng.random((E, n)) < 0.2
    P = oc.rows(0, E, n)
    mask_t, spec_t = sgpu.upload_mask(det), sgpu.upload_rows(P)
    _same(_run(s, mask_t, spec_t, E, 2, n=n), om.update(None, det, P, 2, True), 500000, "REF_MAG handle, uploaded mask")
    out = _Out(E, 2, n, 2)

    def rc(h=0, m=mask_t.data_ptr(), sp=spec_t.data_ptr(), n_e=E, q=None, b=out.bins.data_ptr(), st=out.streams.data_ptr(), u=out.usual.data_ptr(),
           ws=out.ws.data_ptr(), wb=out.ws_bytes, eps=2, duty=500000, first=1, r=None):
        if q is None:
            q = cs.OccmapParams(epochs_per_stream=eps, first=first, duty_ppm=duty)
            if r is not None:
                q.reserved[r] = 1
        v = lambda p: C.c_void_p(p or None)      # noqa: E731
        return L.crn_occmap_device(s._h if h == 0 else h, v(m), v(sp), n_e, C.byref(q) if q != 0 else None, v(b), v(st), v(u), v(ws), wb, None)
    for bad in ({"h": None}, {"m": 0}, {"q": 0}, {"b": 0}, {"st": 0}, {"ws": 0}, {"n_e": -1}, {"eps": 0}, {"eps": -2}, {"eps": 3}, {"duty": 0},
                {"duty": -5}, {"duty": 1000001}, {"r": 0}, {"r": 4},
                {"m": mask_t.data_ptr() + 4}, {"sp": spec_t.data_ptr() + 8}, {"sp": spec_t.data_ptr() + 4}, {"b": out.bins.data_ptr() + 8},
                {"st": out.streams.data_ptr() + 8}, {"u": out.usual.data_ptr() + 4}, {"ws": out.ws.data_ptr() + 8},
                {"wb": out.ws_bytes - 1}, {"wb": 0}, {"wb": -1}):
        assert rc(**bad) == cs.CRN_ERR_ARG, bad
        assert b"crn_occmap_device" in L.crn_last_error(), bad
    assert rc(n_e=0) == 0 and rc(n_e=0, first=0) == 0 and rc(n_e=0, eps=7) == 0
    torch.cuda.synchronize()
    out.host()
    assert all((x == 255).all() for x in out.raw.values()) and out.pads_untouched() and (out.ws.cpu().numpy() == 255).all()
    assert rc() == 0 and rc(sp=0, u=0) == 0 and rc(duty=1) == 0 and rc(duty=1000000) == 0 and rc(first=5) == 0
    torch.cuda.synchronize()
    s.close()


# ---- 8. end to end with the generator ---------------------------------------------------------------------------------------------
def test_end_to_end_with_the_generator(built):
    """crn_synth_fill_device_ex at N = 1024, K = 10, rect, one stream of 600 epochs, CRN_SIG_CW under the intended Markov chain (CH1, CH2
    and CH3 are left with probability 0.9, 0.5 and 0.4, so they are on the air for very different shares of the time), CA-CFAR at Pfa
    1e-2, this stage.  Every record equals the twin.  A channel's carrier sits in one bin (the strongest of the epochs that d_truth
    gives to the channel): its duty against the fraction of epochs d_truth names the channel, held to occmap_cases.E2E_DUTY_RANGE; and the
    usual mask at a duty_ppm midway between two channels' realised fractions holds the carriers of the channels above it, not the ones
    below."""
    e2e = oc.E2E
    n, k, E = e2e["n"], e2e["k"], e2e["epochs"]
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k)
    iq_t = sgpu.zeros((cs.samples_needed(cfg, E) * 2,), torch.float32)
    truth_t = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    sc = cs.SynthCfg()
    sc.seed, sc.noise_power, sc.signal_rms = e2e["seed"], e2e["noise_power"], e2e["signal_rms"]
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = 0, cs.PU_MARKOV_INTENDED, cs.SIG_CW, 1
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), E, cs.samples_per_epoch(cfg), sc, truth_ptr=truth_t.data_ptr())
    s.set_cfar(G_, W_, cs.cfar_alpha(e2e["pfa"], k, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, iq_t, E)
    truth = truth_t.cpu().numpy()
    det = om.unpack_mask(outs["mask"].cpu().numpy(), n)
    P = outs["spectrum"].cpu().numpy()
    want = om.update(None, det, P, E, True)
    frac = {c: float((truth == c).mean()) for c in (1, 2, 3)}
    carrier = {c: int(np.argmax(P[truth == c].mean(axis=0))) for c in (1, 2, 3)}
    order = sorted(frac, key=frac.get)
    cutoff = 0.5 * (frac[order[1]] + frac[order[2]])              # between the two channels most on the air
    out = _run(s, outs["mask"], outs["spectrum"], E, E, int(round(cutoff * 1e6)), n=n)
    bins, _ = _same(out, want, int(round(cutoff * 1e6)), "end to end")
    s.close()
    m = cs.occupancy_map(bins[0])
    usual = om.unpack_mask(out.raw["usual"].view(np.uint32), n)[0]
    for c in (1, 2, 3):
        b = carrier[c]
        print(f"CH{c}: carrier at bin {b}, named by d_truth in {frac[c]:.4f} of the epochs, duty {m['duty'][b]:.4f} ({m['duty'][b] - frac[c]:+.4f}); "
              f"rises {int(bins['n_rise'][0, b])}, longest busy run {int(bins['run_max'][0, b, 1])}, mean_busy / mean_idle "
              f"{m['mean_busy'][b] / m['mean_idle'][b]:.1f}; in the usual mask at {cutoff:.4f}: {bool(usual[b])}")
    print(f"usual bins {int(usual.sum())}: {np.flatnonzero(usual).tolist()[:8]}; floor_db over the band {np.nanmin(cs.floor_db(bins[0])):.2f} .. "
          f"{np.nanmax(cs.floor_db(bins[0])):.2f} dB")
    for c in (1, 2, 3):
        assert oc.E2E_DUTY_RANGE[0] <= m["duty"][carrier[c]] - frac[c] <= oc.E2E_DUTY_RANGE[1], c
    assert np.flatnonzero(usual).tolist() == sorted(carrier[c] for c in (1, 2, 3) if frac[c] >= cutoff) == [carrier[order[2]]]


# ---- 9. cost ----------------------------------------------------------------------------------------------------------------------
# CFAR launch + crn_occmap_device against the CFAR launch alone, `spectrum` written in both arms, with the project's rule for a stage
# nobody has measured before: 1 + 1.5 x (the larger measured B / A - 1).  Measured on an MI355X in two separate runs
# (profiles/r19_occmap.txt): arm A 429.8 us, B / A = 1.1227, the stage alone 48.0 us; arm A 427.1 us, B / A = 1.1248, alone
# 48.3 us.
SPEED_RATIO = 1.188


def test_cost_next_to_the_cfar_launch(built):
    """N = 4096, K = 10, rect, 64 bands, the 2.18 GB batch, 6656 epochs as 13 streams of 512, add_tones traffic; the method of
    tests/stage_gpu.py (best_of_windows): each timed window holds 8 launches issued back to back behind one already queued, the arms
    alternate, 5 windows each after a warm-up, the best counts.  Arm A is the CFAR launch alone, arm B the same launch followed by
    crn_occmap_device on the same stream, usual mask written.  The stage alone, and the same epochs as one stream of 6656, are measured
    the same way and printed.  Every 64th stream-bin is compared with the twin."""
    n, k = 4096, 10
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k, bands=64)
    E, T = 6656, 512                          # 6656 x 10 x 4096 x 8 B = 2.18 GB
    iq_t = sgpu.add_tones(sgpu.noise_batch(E, k, n), E, k, n)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, iq_t, E)
    many, one = _Out(E, E // T, n, T), _Out(E, 1, n, E)
    torch.cuda.synchronize()

    def arm_a():
        sgpu.cfar_launch(s, cfg, iq_t, E, outs=outs)

    def stage(out, eps):
        _run(s, outs["mask"], outs["spectrum"], E, eps, first=True, out=out)

    def arm_b(out=many, eps=T):
        arm_a()
        stage(out, eps)
    arms = {"A": arm_a, "B": arm_b, "B one stream": lambda: arm_b(one, E), "alone": lambda: stage(many, T), "alone one stream": lambda: stage(one, E)}
    times = sgpu.best_of_windows(arms)
    b_many, b_one = many.host()[0], one.host()[0]
    det = om.unpack_mask(outs["mask"].cpu().numpy(), n)[:, ::64]
    P = outs["spectrum"][:, ::64].cpu().numpy()
    s.close()
    best = {name: min(v) for name, v in times.items()}
    nbytes = E * k * n * 8
    moved = E * (n * 4 + n // 8)
    print(f"N=4096 K=10 rect 64 bands, {E} epochs ({nbytes / 1e9:.2f} GB), spectrum written: arm A (CFAR launch alone) {best['A']:.4f} ms "
          f"({nbytes / best['A'] / 1e6:.0f} GB/s of input)")
    for name, label in (("", "13 streams of 512"), (" one stream", "one stream of 6656")):
        print(f"  {label:20s} B / A = {best['B' + name] / best['A']:.4f}   the three kernels alone {best['alone' + name] * 1e3:.1f} us "
              f"({moved / best['alone' + name] / 1e6:.0f} GB/s of the {moved / 1e6:.0f} MB of rows and mask)")
    assert many.pads_untouched() and one.pads_untouched()
    om.compare(b_many[:, ::64], om.update(None, det, P, T, True), "every 64th bin, 13 streams")
    om.compare(b_one[:, ::64], om.update(None, det, P, E, True), "every 64th bin, one stream")
    # the two layouts saw the same epochs: a tone's bin is busy in its third of them, a noise bin in a false alarm's share
    assert (b_one["n_busy"][0] == b_many["n_busy"].sum(axis=0)).all() and b_one["n_busy"][0].max() >= E // 3 and b_one["n_busy"][0].min() < E // 100
    assert best["B"] <= SPEED_RATIO * best["A"], (best["B"] / best["A"], SPEED_RATIO)
