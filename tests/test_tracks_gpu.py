"""crn_tracks_device on the MI355X: the kernels against the float64 twin (tests/tracks_f64.py) fed the kernels' own input arrays, so
the comparison is exact — headers, every integer field, flags, peak_power (the same bits), the zero fill and the whole of d_track_of
equal; power_sum within 2^-22 relative (fp64 accumulation in whatever order the atomics landed, one rounding to fp32: the bound and
the reason of tests/segments_f64.py); centre within N x 2^-23 bins on the circle (the fp32 spacing of a value below N is at most
N x 2^-24, the fp64 sums add far less; derived, not measured).  Output buffers are filled with 0xFF bytes before every call so that a
slot the kernels skipped shows (d_track_of with 0x7F bytes: 0xFF would read as the legitimate label -1), and so is the workspace."""
import ctypes as C

import numpy as np
import pytest

import crnsense as cs
import tracks_f64 as tk
from tracks_cases import E2E, check_end_to_end, e2e_cfg, e2e_synth, runs_of_truth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402
import tracks_gpu_util as tu    # noqa: E402

G_, W_ = 2, 16
SLACKS, MAX_MISS, MIN_EPOCHS, MAX_TRACKS, MAX_SEGMENTS = (0, 2, 40), (0, 1, 3), (1, 2, 5), (1, 64, 1024), (1, 16, 256)


def _cfar(s, cfg, iq_t, E, outs=None):
    return sgpu.cfar_launch(s, cfg, iq_t, E, outs=outs, band_bins=False)


def _check(s, segs, n, eps, combos, what):
    """The exact comparison over `combos` of (slack_bins, max_miss, min_epochs, max_tracks) on one pair of device arrays."""
    ep, sgm = segs.host()
    roots, worst_p, worst_c, found = {}, 0.0, 0.0, 0
    for slack, miss, mine, mt in combos:
        got = tu.tracks(s, segs, eps, slack, miss, mine, mt).host()
        if (slack, miss) not in roots:
            ns = np.clip(ep["n_stored"].astype(np.int64), 0, segs.S)
            roots[slack, miss] = tk.components(ns, sgm["lo"].astype(np.int64), sgm["width"].astype(np.int64), n, eps, slack, miss)
        want = tk.run(ep, sgm, n, eps, slack, miss, mine, mt, root=roots[slack, miss])
        p, c = tk.compare(*got, *want, n)
        worst_p, worst_c, found = max(worst_p, p), max(worst_c, c), max(found, int(want[0]["n_found"].max()))
    print(f"{what}: {len(combos)} parameter sets x {segs.E} epochs ({segs.E // eps} streams), {int(ep['n_stored'].sum())} nodes, most tracks in a "
          f"stream {found}, power_sum error {worst_p:.2e} (bound {tk.POWER_TOL:.2e}), centre error {worst_c:.2e} bins (bound {n * tk.CENTRE_TOL:.2e})")


@pytest.mark.parametrize("n", [512, 4096])
def test_kernel_matches_twin_on_make_epochs_traffic(built, n):
    import signals
    cfg = sgpu.cfg(n)
    E = 48
    iq, _ = signals.make_epochs(cfg, E, seed=n + 3)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-2, 10, W_), 1)
    outs = _cfar(s, cfg, torch.from_numpy(iq).to(DEV), E)
    for S, g in ((16, 3), (256, 0)):
        segs = tu.Segs.from_masks(s, outs["mask"], outs["spectrum"], g, 1, S)
        for eps in (E, E // 4):
            _check(s, segs, n, eps, tu.SOME, f"make_epochs N={n} max_segments={S} eps={eps}")
    s.close()


@pytest.mark.parametrize("kind", [cs.SIG_CW, cs.SIG_RRC_QPSK])
@pytest.mark.parametrize("n_streams", [1, 4, 64])
@pytest.mark.parametrize("pu", [cs.PU_MARKOV_INTENDED, cs.PU_SWEEP])
@pytest.mark.parametrize("n", [512, 4096])
def test_kernel_matches_twin_on_generated_traffic(built, n, pu, n_streams, kind):
    """The device generator's traffic models, CFAR -> segments -> tracks."""
    cfg = sgpu.cfg(n)
    E = 256
    spe = cs.samples_per_epoch(cfg)
    iq_t = torch.zeros((cs.samples_needed(cfg, E) * 2,), dtype=torch.float32, device=DEV)
    truth_t = torch.zeros((E,), dtype=torch.int32, device=DEV)
    sc = cs.SynthCfg()
    sc.seed, sc.noise_power, sc.signal_rms = 5 + n + kind + n_streams, 1e-6, 0.02
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = 8, pu, kind, n_streams
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), E, spe, sc, truth_ptr=truth_t.data_ptr())
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, 10, W_), 1)
    outs = _cfar(s, cfg, iq_t, E)
    segs = tu.Segs.from_masks(s, outs["mask"], outs["spectrum"], 3 if kind == cs.SIG_RRC_QPSK else 0, 1, 16)
    _check(s, segs, n, E // n_streams, tu.SOME[:4], f"generator pu={pu} kind={kind} N={n} streams={n_streams}")
    s.close()


@pytest.mark.parametrize("density", [0.001, 0.03, 0.5])
def test_parameter_sweep_on_random_masks(built, density):
    """Random masks through crn_segments_device at three densities; slack_bins x max_miss x min_epochs x max_tracks x max_segments."""
    n, eps = 512, 24
    E = 4 * eps if density < 0.1 else 2 * eps
    rng = np.random.default_rng(int(1000 * density) + 1)
    det = rng.random((E, n)) < density
    det[rng.random(E) < 0.1] = False                          # some empty epochs
    P = (rng.gamma(10.0, 1e-4, (E, n)) * np.where(rng.random((E, n)) < 0.02, 1e4, 1.0)).astype(np.float32)
    mask_t, spec_t = sgpu.upload_mask(det), sgpu.upload_rows(P)
    s = cs.Sensor(sgpu.cfg(n))
    for S in MAX_SEGMENTS:
        segs = tu.Segs.from_masks(s, mask_t, spec_t, 1, 1, S)
        combos = [(sl, mi, me, mt) for sl in SLACKS for mi in MAX_MISS for me in MIN_EPOCHS for mt in MAX_TRACKS]
        _check(s, segs, n, eps, combos, f"random masks density {density} max_segments={S}")
    s.close()


def hand_made(n):
    """(name, E, epochs_per_stream, {epoch: [(lo, width[, power, centroid, peak])]}, parameter sets): the cases of tests/test_tracks_host.py
    at size n, and a few that only make sense on the device (every slot of an epoch in use, garbage behind n_stored is never read)."""
    few = [(0, 0, 1, 64), (1, 0, 1, 64), (0, 1, 1, 64), (5, 0, 1, 64), (4, 0, 1, 64), (1, 3, 2, 2), (0, 2, 3, 64)]
    merge = {e: [(10, 2), (20, 2)] for e in (0, 1, 2, 4, 5)}
    merge[3] = [(10, 12)]
    singles = {e: [(100, 2)] for e in range(1, 6)}
    singles[2] = [(30, 1), (100, 2)]
    singles[4] = [(100, 2), (180, 1)]
    return [("emitter in epochs 3..9", 12, 12, {e: [(10, 3, 2.0 + e, 0.5 * e % 3, 1.0 + e)] for e in range(3, 10)}, few),
            ("one-epoch gap", 8, 8, {e: [(40, 2)] for e in (2, 3, 5, 6)}, few),
            ("pair across the wrap", 2, 2, {0: [(n - 1, 1, 1.0, 0.0)], 1: [(0, 1, 3.0, 0.0)]}, few),
            ("pair across the wrap, the other way", 2, 2, {0: [(0, 1, 3.0, 0.0)], 1: [(n - 1, 1, 1.0, 0.0)]}, few),
            ("width N", 2, 2, {0: [(0, n)], 1: [(77, 1), (200, 3)]}, few), ("wrap-crossing segment", 2, 2, {0: [(n - 2, 4)], 1: [(1, 1), (2, 1)]}, few),
            ("sweep", 6, 6, {e: [(8 * e, 4)] for e in range(6)}, few), ("carriers that merge once", 6, 6, merge, few),
            ("singles", 7, 7, singles, few), ("truncation", 3, 3, {0: [(20 * k, 2) for k in range(4)], 1: [(20 * k, 2) for k in range(4)], 2: [(200, 1)]}, few),
            ("stream boundary", 8, 4, {e: [(50, 4)] for e in range(2, 6)}, few), ("every epoch, two streams", 8, 4, {e: [(50, 4)] for e in range(8)}, few),
            ("nothing at all", 6, 3, {}, few), ("zero power", 3, 3, {e: [(9, 2, 0.0, 0.0, 0.0)] for e in range(3)}, few),
            ("centre that rounds up to N", 2, 2, {0: [(n - 1, 1, 1.0, 1 - 2.0 ** -24)], 1: [(n - 1, 1, 1.0, 1 - 2.0 ** -24)]}, few)]


@pytest.mark.parametrize("n", [512, 4096])
def test_hand_made_lists(built, n):
    s = cs.Sensor(sgpu.cfg(n))
    for name, E, eps, lists, combos in hand_made(n):
        ep, segs = tk.make_lists(E, 4, lists)
        _check(s, tu.Segs.from_host(ep, segs), n, eps, combos, f"N={n} {name}")
    s.close()


@pytest.mark.parametrize("case", ["solid", "alternating"])
def test_worst_cases_at_4096_epochs(built, case):
    """One stream of 4096 epochs.  solid: one segment of width N in every epoch, a chain as long as the stream.  alternating: 256
    one-bin segments in every epoch with max_miss 3, the most links (every segment links to 4 x up to 3 segments at slack_bins 2)."""
    n, E = 512, 4096
    word = 0xFFFFFFFF if case == "solid" else 0x55555555
    mask_t = torch.full((E, n // 32), word - (1 << 32) if word >> 31 else word, dtype=torch.int32, device=DEV)
    spec_t = torch.rand((E, n), dtype=torch.float32, device=DEV) + 0.5
    s = cs.Sensor(sgpu.cfg(n))
    if case == "solid":
        for S in (1, 16):
            _check(s, tu.Segs.from_masks(s, mask_t, spec_t, 0, 1, S), n, E, [(0, 0, 1, 64), (40, 3, 5, 1)], f"solid, max_segments {S}")
    else:
        _check(s, tu.Segs.from_masks(s, mask_t, spec_t, 0, 1, 256), n, E, [(0, 3, 1, 1024), (2, 3, 2, 64)], "alternating")
    s.close()


def test_refusals_and_n_epochs_zero(built):
    n, E, S = 512, 8, 4
    L = cs.lib()
    s = cs.Sensor(cs.cfg_reference())                         # the handle supplies fft_len and the device only
    ep, sgm = tk.make_lists(E, S, {e: [(50, 4)] for e in range(2, 6)})
    segs = tu.Segs.from_host(ep, sgm)
    out = tu.Tracks(E, S, 2, 64)

    def rc(h=None, ep_=segs.epochs.data_ptr(), sg_=segs.segments.data_ptr(), E_=E, q=None, st=out.streams.data_ptr(), tr=out.tracks.data_ptr(),
           of=out.track_of.data_ptr(), ws=out.ws.data_ptr(), nb=out.ws_bytes, **kw):
        if q is None:
            q = cs.track_params(kw.get("S", S), kw.get("eps", 4), kw.get("slack", 1), kw.get("miss", 0), kw.get("mine", 1), kw.get("mt", 64))
            q.reserved[0], q.reserved[1] = kw.get("r0", 0), kw.get("r1", 0)
        v = lambda p: C.c_void_p(p or None)               # noqa: E731
        return L.crn_tracks_device(s._h if h is None else h, v(ep_), v(sg_), E_, C.byref(q) if q != 0 else None, v(st), v(tr), v(of), v(ws), nb, None)
    assert rc() == 0
    for bad in ({"ep_": 0}, {"sg_": 0}, {"q": 0}, {"st": 0}, {"tr": 0}, {"ws": 0}, {"E_": -4}, {"S": 0}, {"S": 257}, {"eps": 0}, {"eps": 3}, {"eps": -4},
                {"slack": -1}, {"slack": n}, {"miss": -1}, {"miss": 16}, {"mine": 0}, {"mt": 0}, {"mt": 1025}, {"r0": 1}, {"r1": 7},
                {"ep_": segs.epochs.data_ptr() + 4}, {"sg_": segs.segments.data_ptr() + 8}, {"st": out.streams.data_ptr() + 8},
                {"tr": out.tracks.data_ptr() + 8}, {"of": out.track_of.data_ptr() + 2}, {"ws": out.ws.data_ptr() + 4}, {"nb": out.ws_bytes - 1}, {"nb": 0}):
        assert rc(**bad) == cs.CRN_ERR_ARG, bad
        assert b"crn_tracks_device" in L.crn_last_error()
    assert rc(slack=n - 1) == 0 and rc(miss=15) == 0 and rc(of=0) == 0 and rc(mt=1) == 0 and rc(eps=8) == 0
    _check(s, segs, n, 4, [(0, 0, 1, 64)], "REF_MAG handle")
    # n_epochs = 0 succeeds and launches nothing
    fresh = tu.Tracks(E, S, 2, 64)
    assert rc(E_=0, st=fresh.streams.data_ptr(), tr=fresh.tracks.data_ptr(), of=fresh.track_of.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (fresh.streams.cpu().numpy() == 255).all() and (fresh.tracks.cpu().numpy() == 255).all() and (fresh.track_of.cpu().numpy() == 0x7F).all()
    # d_track_of = NULL leaves the labels alone and changes nothing else
    a, b = tu.tracks(s, segs, 4), tu.tracks(s, segs, 4, labels=False)
    torch.cuda.synchronize()
    assert a.tracks.cpu().numpy().tobytes() == b.tracks.cpu().numpy().tobytes() and (b.track_of.cpu().numpy() == 0x7F).all()
    s.close()


def test_stream_independence_and_repeatability(built):
    """A batch of S streams gives, stream for stream, the bytes that S separate calls give; two runs on the same input give the same
    bytes in every integer field (the order the unions landed in does not show)."""
    n, n_streams, eps, S = 512, 8, 64, 16
    E = n_streams * eps
    rng = np.random.default_rng(9)
    det = rng.random((E, n)) < 0.02
    for k in range(6):                                        # a few emitters that stay, so that tracks are long
        det[:, 40 + 70 * k: 43 + 70 * k] |= (rng.random(E) < 0.8)[:, None]
    P = rng.gamma(10.0, 1e-4, (E, n)).astype(np.float32)
    s = cs.Sensor(sgpu.cfg(n))
    segs = tu.Segs.from_masks(s, sgpu.upload_mask(det), sgpu.upload_rows(P), 1, 1, S)
    ints = [f for f in np.dtype(cs.TRACK_DTYPE).names if f not in ("power_sum", "centre")]
    for slack, miss, mine, mt in ((1, 0, 1, 64), (2, 2, 2, 8)):
        whole = tu.tracks(s, segs, eps, slack, miss, mine, mt)
        again = tu.tracks(s, segs, eps, slack, miss, mine, mt)
        w, a = whole.host(), again.host()
        assert w[0].tobytes() == a[0].tobytes() and (w[2] == a[2]).all()
        for f in ints:
            assert w[1][f].tobytes() == a[1][f].tobytes(), f
        for st in range(n_streams):
            part = tu.Segs(eps, S)
            part.epochs, part.segments = segs.epochs[st * eps:(st + 1) * eps], segs.segments[st * eps:(st + 1) * eps]
            one = tu.tracks(s, part, eps, slack, miss, mine, mt).host()
            assert one[0].tobytes() == w[0][st:st + 1].tobytes(), st
            assert one[1].tobytes() == w[1][st:st + 1].tobytes(), st
            assert (one[2] == w[2][st * eps:(st + 1) * eps]).all(), st
    _check(s, segs, n, eps, [(1, 0, 1, 64), (2, 2, 2, 8)], "staying emitters over clutter")
    s.close()


def test_end_to_end_markov_dwell_runs(built):
    """The parameters chosen on the twins (tests/tracks_cases.py, E2E): intended-Markov CW traffic from crn_synth_fill_device_ex with
    d_truth, 64 streams x 104 epochs, N = 4096, max_miss 0, min_epochs 1.  Every maximal run of one band in a stream's truth has exactly
    one track whose centre lies inside that band and whose first_t / last_t are the run's; every other track has n_epochs_hit 1; the
    3 x 3 transition counts rebuilt from the matched tracks equal those counted in the truth."""
    cfg = e2e_cfg()
    n_streams, eps = 64, E2E["eps"]
    E = n_streams * eps
    iq_t = torch.zeros((cs.samples_needed(cfg, E) * 2,), dtype=torch.float32, device=DEV)
    truth_t = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), E, cs.samples_per_epoch(cfg), e2e_synth(n_streams), truth_ptr=truth_t.data_ptr())
    s.set_cfar(E2E["guard"], E2E["train"], cs.cfar_alpha(E2E["pfa"], E2E["k"], E2E["train"]), 1)
    outs = _cfar(s, cfg, iq_t, E)
    segs = tu.Segs.from_masks(s, outs["mask"], outs["spectrum"], E2E["merge_gap"], E2E["min_width"], E2E["max_segments"])
    got = tu.tracks(s, segs, eps, E2E["slack_bins"], E2E["max_miss"], E2E["min_epochs"], E2E["max_tracks"]).host()
    truth = truth_t.cpu().numpy().reshape(n_streams, eps)
    ep, _ = segs.host()
    s.close()
    assert (ep["n_found"] == ep["n_stored"]).all()
    n_runs, n_other = check_end_to_end(cfg, truth, got[0], got[1])
    want_runs = sum(len(runs_of_truth(r)) for r in truth)
    print(f"end to end: {n_streams} streams x {eps} epochs, {want_runs} dwell runs in the truth, {n_runs} matched one track each, "
          f"{n_other} other tracks of one epoch")
    assert n_runs == want_runs


# CFAR launch + crn_segments_device (what the parent commit runs, arm A) against the same followed by crn_tracks_device (arm B), measured
# on the MI355X (Tracks): B / A at 64 streams and at 1 stream, and the stage alone at 1 stream over the stage alone at 64.
# Measured on two boxes: 1.141 and 1.152, 1.135 and 1.127, 1.071 and 1.076; the constants are the means.  Each bar is the mean times 1.06, the margin the CA and segments speed tests carry over their own measurements.
RATIO_64_MEASURED, RATIO_1_MEASURED, ONE_OVER_64_MEASURED = 1.146, 1.131, 1.074
MARGIN = 1.06


def test_cost_next_to_cfar_and_segments(built):
    """N = 4096, K = 10, rect, 64 bands, the 2.18 GB batch of 6656 epochs, 16 slots, the traffic of tests/test_segments_gpu.py's speed
    test; the method of tests/stage_gpu.py (best_of_windows): each timed window holds 8 launches issued back to back behind one already
    queued, the arms alternate, 5 windows each after a warm-up, the best counts.  Printed, not asserted: the stage alone on the same segments plus one emitter that stays in bins 324..326 of
    every epoch, a track as long as the stream, where the members' atomic adds to one accumulator queue up."""
    n, k = 4096, 10
    cfg = sgpu.cfg(n, k=k, bands=64)
    E, S = 6656, 16
    iq_t = sgpu.add_tones(sgpu.noise_batch(E, k, n), E, k, n)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = _cfar(s, cfg, iq_t, E)
    segs = tu.Segs(E, S)
    out = {64: tu.Tracks(E, S, 64, 64), 1: tu.Tracks(E, S, 1, 64)}
    torch.cuda.synchronize()

    def arm_a():
        _cfar(s, cfg, iq_t, E, outs=outs)
        s.segments_device(outs["mask"].data_ptr(), outs["spectrum"].data_ptr(), E, segs.epochs.data_ptr(), segs.segments.data_ptr(), max_segments=S)

    def alone(ns):
        tu.tracks(s, segs, E // ns, 1, 0, 1, 64, out=out[ns])

    def arm_b(ns):
        arm_a()
        alone(ns)
    arm_a()
    stay = outs["mask"].clone()
    stay[:, 10] |= 0x70
    segs_stay = tu.Segs.from_masks(s, stay, outs["spectrum"], 0, 1, S)

    def alone_stay(ns):
        tu.tracks(s, segs_stay, E // ns, 1, 0, 1, 64, out=out[ns])
    arms = {"A": arm_a, "B 64": lambda: arm_b(64), "B 1": lambda: arm_b(1), "alone 64": lambda: alone(64), "alone 1": lambda: alone(1)}
    times = sgpu.best_of_windows(arms)
    st64, st1 = out[64].host()[0], out[1].host()[0]
    ep = segs.host()[0]
    stay_us = {}
    for ns in (64, 1):
        stay_us[ns] = min(sgpu.best_of_windows({ns: lambda: alone_stay(ns)}, windows=3, warm_up=False, report=False)[ns]) * 1e3
    longest = int(out[1].host()[1]["n_epochs_hit"].max())
    s.close()
    best = {name: min(v) for name, v in times.items()}
    r64, r1, one_over_64 = best["B 64"] / best["A"], best["B 1"] / best["A"], best["alone 1"] / best["alone 64"]
    print(f"N=4096 K=10 rect 64 bands, {E} epochs, {S} slots, {int(ep['n_stored'].sum())} nodes; tracks found: {int(st64['n_found'].sum())} in 64 "
          f"streams, {int(st1['n_found'].sum())} in one; arm A (CFAR + segments) {best['A']:.4f} ms")
    print(f"  B / A = {r64:.4f} at 64 streams, {r1:.4f} at 1 stream; the stage alone {best['alone 64'] * 1e3:.1f} us at 64 streams, "
          f"{best['alone 1'] * 1e3:.1f} us at 1 stream: x{one_over_64:.3f}")
    print(f"  with an emitter that stays (longest track {longest} epochs): the stage alone {stay_us[64]:.1f} us at 64 streams, {stay_us[1]:.1f} us at 1 stream")
    assert st64["n_nodes"].sum() == st1["n_nodes"].sum() == ep["n_stored"].sum() > 0
    assert r64 <= RATIO_64_MEASURED * MARGIN, (r64, RATIO_64_MEASURED * MARGIN)
    assert r1 <= RATIO_1_MEASURED * MARGIN, (r1, RATIO_1_MEASURED * MARGIN)
    assert one_over_64 <= ONE_OVER_64_MEASURED * MARGIN, (one_over_64, ONE_OVER_64_MEASURED * MARGIN)
