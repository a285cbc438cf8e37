"""The STREAMING forms of the sensing kernel at 512 and 1024 points, pinned to float64 at their smallest failing shapes.

A launch of at most one epoch per compute unit runs the dealt-frame kernel at these sizes (crn_api.cpp, run_device_impl), so every
other small 512 / 1024-point test in tests/ checks that kernel; what bench.py times for cfg1 (1024-point) and cfg3 (ref512) — and what
every large batch runs — is the streaming kernel, where one wave holds two (512) or one (1024) lane groups and no barrier separates
the exchanges.  Here every case selects the streaming form through tests/forms.py and asserts that no launch was dealt.

FORMS lists what is pinned, each by the row of the table of compiled forms it runs, written as csrc/crn_forms.h writes it
(add_forms_of_size; select_form in csrc/crn_forms.cpp picks it; r3 = N / 256).

Shapes: K in {1, 2, 3, 10} (no averaging; the ping-pong frame loop's even and odd ends); L in {N, 364, 363, 1} where the form takes short
packets; 100 epochs at N = 512 and 50 at N = 1024 = 13 epoch groups, the last one with 4 / 2 live epochs (and 97 / 49 epochs: a last
group with ONE live epoch); launch geometries GEOMETRIES through the A/B codes 100 + epw, 200 + n, 300 + n: every workgroup one
group; two or three big workgroups of 3 or 4 groups (the cross-epoch prefetch) followed by single-group tail workgroups, by a ragged
workgroup of fewer groups than it was given, or by tail workgroups of 2 groups with a ragged last one.

Reference: float64 — per bin signals.spectrum_f64; features, network outputs and decisions tests/ref_f64.py for the plans it models
and float64 band sums of spectrum_f64 over signals.band_bins for the custom plans — with the C oracle alongside as
test_gpu_parity.check_against_oracle has it.

Bounds.  Per bin tests/parity_policy.py's: PER_BIN_TOL at floor 1e-2 * mean for K >= 4 and at floor 1e-1 * mean for K < 4 (the
argument is in test_gpu_parity.test_frames_per_epoch_edge_cases), and never further from float64 than twice the oracle's distance +
2e-6.  One exception: in |X| mode at K < 4 the first clause is asserted only where the fp32 C oracle itself stays below PER_BIN_TOL / 2
(every L = 1 case).  The K < 4 floor is argued for energies (a bin at 10 % of the mean ENERGY holds |X| ~ 0.3 rms); in |X| mode mean |X|
is not lifted by a carrier the way mean |X|^2 is, a bin at 10 % of it holds |X| ~ 0.1 rms, and the oracle sits at 1.0e-5 .. 6.7e-5
there on these inputs (1.4e-5 .. 3.2e-5 behind Blackman-Harris): no fp32 transform meets 1e-5 at that floor, so there the bar would say
nothing about the kernel and the second clause alone holds it.  At K = 10 the |X| forms are held to PER_BIN_TOL like the others
(oracle <= 8.4e-6).
Features against float64: max(pol.FEATURE_TOL, 2 x the C oracle's own relative distance d from float64 on the same input + 2e-6) — the
oracle is the same fp32 arithmetic in another order, so a factor of 2 covers ordering; d is computed on the CPU from the oracle, never
from GPU output.  Features against the oracle: max(pol.FEATURE_TOL, 3 d + 2e-6) — FEATURE_TOL as everywhere in tests/ while the oracle
is within 2.67e-6 of float64, beyond that what the two float64 distances add up to.  The family that needs it is hop-N/2 Hann at K = 1,
64 bands of 8 / 16 bins: a band next to a +38 dB carrier's holds a sliver of its energy, and the oracle itself is 6.3e-6 .. 1.2e-5 from
float64 there, so a flat 1e-5 between two fp32 paths is not a statement about either.
Decisions and occupancy equal float64's for EVERY epoch: each input is asserted to keep every epoch outside pol.ANN_MARGIN /
pol.THRESHOLD_MARGIN in the float64 reference alone; `PYTHONPATH=cognitive-radio-network_amd:tests python
tests/test_streaming_small_gpu.py` recomputes that and the table below on the CPU (SEED_BUMP lists the seeds moved off a margin band).

The C oracle's distance from float64 on exactly these inputs, maximum per form over N, K, L and epochs, and the smallest distance of any
epoch from a compare (needed: 6e-6 for the network, 4e-6 for thresholds):
    form               features   per bin    smallest margin
    ref_mag_whole      2.88e-06   -          1.99e-01
    ref_mag_short      2.34e-06   -          1.99e-01
    ref_energy_whole   2.05e-06   -          2.45e-01
    ref_energy_short   3.94e-06   -          2.98e-04
    other_plan_whole   2.49e-06   -          1.48e-02
    other_plan_short   2.18e-06   -          5.90e-04
    sixteen_bands      2.24e-06   -          1.64e-04
    spectrum_energy    2.55e-06   7.17e-06   1.20e-03
    spectrum_mag       2.98e-06   6.65e-05   1.99e-01     (per bin at K = 10: 8.44e-06)
    bh_energy          2.82e-06   3.48e-06   1.97e-02
    bh_mag             2.66e-06   3.20e-05   1.99e-01     (per bin at K = 10: 7.03e-06)
    hann_disjoint      2.44e-06   3.77e-06   2.36e-02
    hann_welch         1.11e-05   4.35e-06   1.87e-04     (features at K >= 2: <= 5.7e-06)
    hann_welch_gaps    1.21e-05   4.45e-06   7.09e-05     (features at K >= 2: <= 6.6e-06)

Bit identity: the same input gives the same bits under every geometry; those bits are the dealt form's on the same 50 - 100 epoch
batch; a hop-N/2 stream in one launch equals the same stream cut at an epoch boundary into two launches.  Window discipline: poison
(NaN) behind the last sample a launch may read, and between epochs that lie further apart than they are long, changes no bit — all of
it inside the allocation.
"""
import functools
import zlib

import numpy as np
import pytest

import crnsense as cs
import forms
import oracle_py as orc
import parity_policy as pol
import ref_f64
import signals
from test_dealt_frames import _plans

pytestmark = pytest.mark.gpu

NS = (512, 1024)
KS = (1, 2, 3, 10)
N_EPOCHS = {512: 100, 1024: 50}          # 13 epoch groups (8 / 4 epochs each), the last one ragged
N_EPOCHS_ONE_LIVE = {512: 97, 1024: 49}  # ... with a single live epoch
# (epw, tail, tail_epw) -> set_variant(100 + epw), (200 + tail), (300 + tail_epw); None = the library's own.  With 13 groups:
GEOMETRIES = [
    (1, None, None),   # 13 workgroups of one group
    (3, None, None),   # tail = 13 / 4 = 3 groups: 3 big workgroups of 3 groups, then 4 single-group workgroups
    (3, 0, 3),         # no short tail: 4 workgroups of 3 groups, then a workgroup given 3 groups that has 1
    (4, 1, 2),         # tail capped at 3 groups: 2 big workgroups of 4, then tail workgroups of 2, 2 and 1 groups
]
GEO_IDS = ["epw1", "epw3", "epw3_no_tail_ragged", "epw4_tail_of_2"]


def _short(n):
    return (n, 364, 363, 1)


def _whole(n):
    return (n,)


def _plan_of(name):
    def make(n):
        return dict(_plans(n))[name]
    return make


def _ref_mag(n):
    return cs.cfg_reference_scaled(n)


def _ref_energy(n):
    return cs.cfg_energy_scaled(n, 4.0)


def _windowed(base, window):
    def make(n):
        c = base(n)
        c.window = window
        return c
    return make


def _welch(n):
    return cs.cfg_welch(n, 8, 64)


# name -> (cfg maker, packet lengths, spectrum request, layout).  The comment names the kernel: its row of csrc/crn_forms.h
FORMS = {
    # the reference plan: pass 3 and the accumulate pruned to its rows, band sums from registers
    "ref_mag_whole": (_ref_mag, _whole, False, "dense"),            # streaming(r3, kRegBands | kRows).magnitude().whole()
    "ref_mag_short": (_ref_mag, lambda n: _short(n)[1:], False, "dense"),        # streaming(r3, kRegBands | kRows).magnitude()
    "ref_energy_whole": (_ref_energy, _whole, False, "dense"),      # streaming(r3, kRegBands | kRows).whole()
    "ref_energy_short": (_ref_energy, lambda n: _short(n)[1:], False, "dense"),  # streaming(r3, kRegBands | kRows)
    # a small plan with a bin outside the reference rows (test_dealt_frames._plans "other plan"): all rows, register close on whole
    # frames, the LDS walk on short packets
    "other_plan_whole": (_plan_of("other plan"), _whole, False, "dense"),                     # streaming(r3, kRegBands).whole()
    "other_plan_short": (_plan_of("other plan"), lambda n: _short(n)[1:], False, "dense"),    # streaming(r3)
    # 16 bands (no row entries) and spectrum requests: the LDS walk
    "sixteen_bands": (_plan_of("16 bands"), _short, False, "dense"),            # streaming(r3).whole() / streaming(r3)
    "spectrum_energy": (_ref_energy, _short, True, "dense"),        # streaming(r3).whole() / streaming(r3)
    "spectrum_mag": (_ref_mag, _short, True, "dense"),              # streaming(r3).magnitude()
    # the table window (Blackman-Harris), pass-2 twiddles in LDS
    "bh_energy": (_windowed(_ref_energy, cs.WINDOW_BLACKMAN_HARRIS), _whole, True, "dense"),  # streaming(r3).window().tw2_from_lds()
    "bh_mag": (_windowed(_ref_mag, cs.WINDOW_BLACKMAN_HARRIS), _whole, True, "dense"),        # streaming(r3).window().tw2_from_lds().magnitude()
    # periodic Hann, whole frames, energy mode: streaming(r3, kHannSym | kTw2Early).window().tw2_from_lds().whole()
    "hann_disjoint": (_windowed(_ref_energy, cs.WINDOW_HANN), _whole, True, "dense"),   # disjoint frames: the plain stream
    "hann_welch": (_welch, _whole, True, "dense"),                                      # hop N/2, dense epochs: launch_cfg's welch_stream
    "hann_welch_gaps": (_welch, _whole, True, "gaps"),                                  # hop N/2, epoch_stride > an epoch: the non-multi path
}


def _cfg(form, n, K, L):
    cfg = FORMS[form][0](n)
    cfg.frames_per_epoch = K
    if cfg.n_bands == 16:       # between the idle and the driven level of a band: 4 x the noise a band of n / 16 bins collects
        for b in range(16):
            cfg.thresh[b] = 4.0 * (n // 16) * L * 1e-6
    if cfg.n_bands == 64:       # Welch: E|X|^2 = sigma^2 sum w^2 = 1e-6 x 0.375 n per bin
        for b in range(64):
            cfg.thresh[b] = 4.0 * (n // 64) * 0.375 * n * 1e-6
    return cfg


# seeds: one per (form, N, K, L); SEED_BUMP moves the few whose float64 reference lands an epoch inside a margin band
SEED_BUMP = {"hann_welch_gaps/512/1/512/100": 1}


def _seed(form, n, K, L, n_epochs):
    key = f"{form}/{n}/{K}/{L}/{n_epochs}"
    return zlib.crc32(key.encode()) % 100000 + SEED_BUMP.get(key, 0)


def _gap_stride(cfg, L):
    return cs.samples_per_epoch(cfg, L) + cfg.fft_len // 2 + 64


def _extent(cfg, L):
    """Samples from an epoch's first to its last (what samples_needed(cfg, 1, L) says)."""
    return cs.samples_needed(cfg, 1, L)


def _spread(cfg, dense_iq, n_epochs, L, stride, fill):
    """The dense batch `dense_iq` laid out with `stride` samples from epoch to epoch; `fill(shape)` gives what lies between."""
    spe, ext = cs.samples_per_epoch(cfg, L), _extent(cfg, L)
    x = np.asarray(dense_iq, np.float32).reshape(-1, 2)
    out = fill(((n_epochs - 1) * stride + ext, 2)).astype(np.float32)
    for e in range(n_epochs):
        out[e * stride: e * stride + ext] = x[e * spe: e * spe + ext]
    return out.ravel()


def _f64_model(form, cfg, n, K):
    """The tests/ref_f64.py plan of this form, or None for the custom band plans."""
    win = {cs.WINDOW_RECT: "rect", cs.WINDOW_HANN: "hann", cs.WINDOW_BLACKMAN_HARRIS: "bh"}[cfg.window]
    if FORMS[form][0] is _welch:
        return ref_f64.plan_welch(n, K, 64, [float(np.float32(cfg.thresh[b])) for b in range(64)])
    if form in ("ref_mag_whole", "ref_mag_short", "spectrum_mag", "bh_mag"):
        runs = {b: tuple((lo * (n // 512), hi * (n // 512)) for lo, hi in rr) for b, rr in ref_f64.REF_RUNS_512.items()}
        return ref_f64.Plan(n=n, k=K, mode="mag", window=win, runs=runs, decide="ann", w_ih=ref_f64.W_IH, w_ho=ref_f64.W_HO)
    if form in ("ref_energy_whole", "ref_energy_short", "spectrum_energy", "bh_energy", "hann_disjoint"):
        p = ref_f64.plan_energy_scaled(n, 4.0)
        p.k, p.window = K, win
        return p
    return None


@functools.lru_cache(maxsize=3)
def reference(form, n, K, L, n_epochs):
    """Input and everything expected of it, computed once per (form, N, K, L) on the CPU and shared by every geometry, the dealt-form
    comparison and the split-launch comparison.  Read-only."""
    cfg = _cfg(form, n, K, L)
    want_spectrum, layout = FORMS[form][2], FORMS[form][3]
    iq, _ = signals.make_epochs(cfg, n_epochs, seed=_seed(form, n, K, L, n_epochs), L=L)
    stride = 0
    if layout == "gaps":      # every epoch starts `stride` samples after the previous one; loud noise in between
        stride = _gap_stride(cfg, L)
        rng = np.random.default_rng(_seed(form, n, K, L, n_epochs) + 1)
        dense = iq
        iq = _spread(cfg, dense, n_epochs, L, stride, lambda shape: rng.normal(0, 1e-2, shape))
        ext = _extent(cfg, L)
        x = iq.reshape(-1, 2)
        truth = np.concatenate([signals.spectrum_f64(cfg, x[e * stride: e * stride + ext].ravel(), 1, L=L) for e in range(n_epochs)])
    else:
        truth = signals.spectrum_f64(cfg, iq, n_epochs, L=L)
    model = _f64_model(form, cfg, n, K)
    r = {"cfg": cfg, "iq": iq, "stride": stride, "truth": truth, "want_spectrum": want_spectrum, "n_epochs": n_epochs, "L": L}
    if model is not None:
        f = ref_f64.run(model, iq, n_epochs, L=L, epoch_stride=stride)
        assert np.allclose(f["spectrum"], truth, rtol=1e-9, atol=1e-12 * truth.mean())      # two float64 statements of one spectrum
        r.update(features=f["features"], decision=f["decision"], occupancy=f["occupancy"], margin=f["margin"],
                 ann_out=f["ann_out"] if cfg.decide == cs.DECIDE_ANN else None)
    else:                     # custom plan: float64 band sums of the float64 spectrum, thresholds in float64
        feat = np.stack([truth[:, signals.band_bins(cfg, b)].sum(axis=1) for b in range(cfg.n_bands)], axis=1)
        thr = np.array([cfg.thresh[b] for b in range(cfg.n_bands)], np.float64)[None, :]
        lim = np.where(np.isinf(thr), np.inf, thr * (feat[:, cfg.ref_band:cfg.ref_band + 1] if cfg.ref_band >= 0 else 1.0))
        occ = feat > lim
        rel = np.where(np.isfinite(lim), np.abs(feat / np.where(np.isfinite(lim), lim, 1.0) - 1.0), np.inf)
        r.update(features=feat, decision=occ.sum(axis=1).astype(np.int32), occupancy=occ.astype(np.uint8), margin=rel.min(axis=1), ann_out=None)
    r["margin_needed"] = pol.ANN_MARGIN if cfg.decide == cs.DECIDE_ANN else pol.THRESHOLD_MARGIN
    want = orc.run(cfg, iq, n_epochs, L=L, want_spectrum=want_spectrum, epoch_stride=stride)
    r["oracle"] = want
    r["oracle_feature_distance"] = float((np.abs(want["features"] - r["features"]) / np.abs(r["features"])).max())
    r["floor"] = 1e-2 if K >= 4 else 1e-1
    r["absolute_per_bin_bar"] = True
    if want_spectrum:
        r["oracle_per_bin"] = float(_per_bin_err(want["spectrum"], truth, r["floor"]))
        # the absolute per-bin bar is stated for energies at every K and for |X| at K >= 4; |X| at K < 4: where the oracle meets it with
        # room, elsewhere the oracle-relative clause alone (module docstring, "Bounds")
        r["absolute_per_bin_bar"] = not (cfg.mode == cs.MODE_REF_MAG and K < 4) or r["oracle_per_bin"] < pol.PER_BIN_TOL / 2
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _per_bin_err(spec, truth, floor):
    fl = floor * truth.mean(axis=1, keepdims=True)
    return (np.abs(spec - truth) / np.maximum(truth, fl)).max()


def check_reference(r):
    """What must hold of the reference alone (CPU): every epoch outside the margin band, and the oracle on float64's side of it."""
    assert (r["margin"] > r["margin_needed"]).all(), "fixture inside the margin band"
    assert np.array_equal(r["oracle"]["decision"], r["decision"]) and np.array_equal(r["oracle"]["occupancy"], r["occupancy"])
    if r["want_spectrum"] and r["absolute_per_bin_bar"]:
        assert r["oracle_per_bin"] < 2 * pol.PER_BIN_TOL


def _run(r, geometry=None, form="streaming", n_epochs=None, first=0):
    """One launch of r's input (epochs [first, first + n_epochs)) on a fresh handle pinned to `form`; asserts the form that ran."""
    cfg, L = r["cfg"], r["L"]
    n_epochs = r["n_epochs"] - first if n_epochs is None else n_epochs
    s = forms.sensor(cfg, form)
    if geometry is not None:
        epw, tail, tail_epw = geometry
        s.set_variant(100 + epw)
        if tail is not None:
            s.set_variant(200 + tail)
        if tail_epw is not None:
            s.set_variant(300 + tail_epw)
    step = r["stride"] or cs.samples_per_epoch(cfg, L)
    got = s.run_host(r["iq"][2 * first * step:], n_epochs, L=L, want_spectrum=r["want_spectrum"], epoch_stride=r["stride"])
    forms.assert_ran(s, form, 1, L=L)
    s.close()
    return got


def _keys(r):
    return ["features", "occupancy", "decision"] + (["ann_out"] if r["cfg"].decide == cs.DECIDE_ANN else []) + (["spectrum"] if r["want_spectrum"] else [])


def _same_bits(a, b, r, what):
    for k in _keys(r):
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@functools.lru_cache(maxsize=3)
def streaming_bits(form, n, K, L, n_epochs):
    """The streaming form's outputs under the first geometry (one epoch group per workgroup): what every other geometry, the dealt
    form and the split launches must reproduce bit for bit."""
    return _run(reference(form, n, K, L, n_epochs), GEOMETRIES[0])


def check_against_float64(got, r):
    cfg = r["cfg"]
    want = r["oracle"]
    check_reference(r)
    if r["want_spectrum"]:
        err = _per_bin_err(got["spectrum"], r["truth"], r["floor"])
        what = f"per bin {err:.3g} at floor {r['floor']:g} (oracle {r['oracle_per_bin']:.3g})"
        if r["absolute_per_bin_bar"]:
            assert err < pol.PER_BIN_TOL, what
        assert err < 2.0 * r["oracle_per_bin"] + 2e-6, what
    d = r["oracle_feature_distance"]
    rel64 = float((np.abs(got["features"] - r["features"]) / np.abs(r["features"])).max())
    rel_orc = float((np.abs(got["features"] - want["features"]) / np.maximum(np.abs(want["features"]), 1e-30)).max())
    what = f"features {rel64:.3g} from float64, {rel_orc:.3g} from the oracle, the oracle {d:.3g} from float64"
    assert rel64 < max(pol.FEATURE_TOL, 2.0 * d + 2e-6), what
    assert rel_orc < max(pol.FEATURE_TOL, 3.0 * d + 2e-6), what
    if cfg.decide == cs.DECIDE_ANN:
        assert np.abs(got["ann_out"] - r["ann_out"]).max() < 1e-6
    assert np.array_equal(got["decision"], r["decision"])
    assert np.array_equal(got["occupancy"], r["occupancy"])


def _cases(geometries=True, only=None):
    out = []
    for form, (_, Ls, _, _) in FORMS.items():
        if only is not None and not only(form):
            continue
        for n in NS:
            for K in KS:
                for L in Ls(n):
                    if geometries:
                        out += [pytest.param(form, n, K, L, g, id=f"{form}-{n}-K{K}-L{L}-{gid}") for g, gid in zip(GEOMETRIES, GEO_IDS)]
                    else:
                        out.append(pytest.param(form, n, K, L, id=f"{form}-{n}-K{K}-L{L}"))
    return out


@pytest.mark.parametrize("form,n,K,L,geometry", _cases())
def test_streaming_form_matches_float64(built, form, n, K, L, geometry):
    """Every form, K, packet length and launch geometry against float64 (module docstring); and the same bits as under the first
    geometry, whatever the workgroups' spans."""
    r = reference(form, n, K, L, N_EPOCHS[n])
    base = streaming_bits(form, n, K, L, N_EPOCHS[n])
    got = base if geometry == GEOMETRIES[0] else _run(r, geometry)
    check_against_float64(got, r)
    _same_bits(got, base, r, geometry)


@pytest.mark.parametrize("form,n,K,L", [p for p in _cases(geometries=False)
                                        if forms.has_dealt_form(_cfg(p.values[0], p.values[1], p.values[2], p.values[3]), p.values[3])])
def test_dealt_form_equals_the_streaming_form_over_many_workgroups(built, form, n, K, L):
    """tests/test_dealt_frames.py holds the two forms together at 1 to 5 epochs; the automatic switch hands the dealt form up to one
    epoch per compute unit.  The same 50 / 100-epoch batches, dealt: the streaming form's bits.  (Every case that has a dealt form.)"""
    r = reference(form, n, K, L, N_EPOCHS[n])
    _same_bits(_run(r, form="dealt"), streaming_bits(form, n, K, L, N_EPOCHS[n]), r, "dealt")


@pytest.mark.parametrize("form,n,K,L", [p for p in _cases(geometries=False) if p.values[2] == 3 and p.values[3] in (p.values[1], 363)])
def test_a_last_group_with_one_live_epoch(built, form, n, K, L):
    """97 / 49 epochs: the last epoch group holds one live epoch, the other lane groups of its workgroup close inactive epochs; under
    the geometry whose last workgroup is ragged as well.  Odd K, the odd packet length."""
    r = reference(form, n, K, L, N_EPOCHS_ONE_LIVE[n])
    got = _run(r, GEOMETRIES[2])
    check_against_float64(got, r)
    _same_bits(got, streaming_bits(form, n, K, L, N_EPOCHS_ONE_LIVE[n]), r, "one live epoch")


@pytest.mark.parametrize("epw", [1, 3])
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n", NS)
def test_welch_stream_equals_two_launches_cut_at_an_epoch_boundary(built, n, K, epw):
    """Hop N/2 over dense epochs: a lane group's epochs are one stream of half-frames, the half an epoch ends with is the half the next
    one starts with.  Cutting the batch at an epoch boundary — not a multiple of the epoch groups, so every later epoch changes lane
    group and workgroup — into two launches gives the same bits."""
    r = reference("hann_welch", n, K, n, N_EPOCHS[n])
    cut = 37 if n == 512 else 19
    geometry = (epw, None, None)
    a, b = _run(r, geometry, n_epochs=cut), _run(r, geometry, first=cut)
    whole = streaming_bits("hann_welch", n, K, n, N_EPOCHS[n])
    for k in _keys(r):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k


def _device_run(cfg, L, n_epochs, stride, want_spectrum, geometry, buf):
    import torch
    dev = buf.device
    s = forms.sensor(cfg, "streaming")
    s.set_variant(100 + geometry[0])
    out = {"features": torch.zeros(n_epochs, cfg.n_bands, device=dev), "ann_out": torch.zeros(n_epochs, 3, dtype=torch.float64, device=dev),
           "decision": torch.full((n_epochs,), -7, dtype=torch.int32, device=dev),
           "occupancy": torch.full((n_epochs, cfg.n_bands), 9, dtype=torch.uint8, device=dev)}
    if want_spectrum:
        out["spectrum"] = torch.zeros(n_epochs, cfg.fft_len, device=dev)
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    ptrs.setdefault("spectrum", 0)
    s.run_device(buf.data_ptr(), n_epochs, L, ptrs, epoch_stride=stride)
    torch.cuda.synchronize()
    forms.assert_ran(s, "streaming", 1, L=L)
    s.close()
    return out


# every form on dense epochs and on epochs with gaps (the Welch forms are listed per layout: hann_welch dense, hann_welch_gaps the other)
_POISON_CASES = [(form, layout) for form in FORMS for layout in ("dense", "gaps")
                 if FORMS[form][0] is not _welch or FORMS[form][3] == layout]


@pytest.mark.parametrize("epw", [1, 3])
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("form,layout", _POISON_CASES)
def test_prefetch_stays_inside_the_launch_window(built, form, layout, n, epw):
    """The streaming workgroup asks for its next frame — the next epoch group's first — from inside the current one; what it may read
    ends with the last sample of the batch's last epoch, and with each epoch's last sample when epochs lie further apart than they are
    long.  A device buffer larger than the launch needs, NaN behind the last sample it may read (and between the epochs): the same
    bits as with finite samples there, and no NaN out.  Odd K and the odd packet length; all poison inside the allocation."""
    import torch
    K = 3
    L = 363 if 363 in FORMS[form][1](n) else n
    n_epochs = N_EPOCHS[n]
    r = reference(form, n, K, L, n_epochs)
    cfg = r["cfg"]
    if r["stride"]:
        stride, clean = r["stride"], r["iq"]
    elif layout == "gaps":
        stride = cs.samples_per_epoch(cfg, L) + 777
        rng = np.random.default_rng(n + 1)
        clean = _spread(cfg, r["iq"], n_epochs, L, stride, lambda shape: rng.normal(0, 1e-2, shape))
    else:
        stride, clean = 0, r["iq"]
    ext = _extent(cfg, L)
    need = (n_epochs - 1) * (stride or cs.samples_per_epoch(cfg, L)) + ext
    assert clean.size == 2 * need
    slack = 4 * n                     # behind the last sample the launch may read, inside the allocation
    rng = np.random.default_rng(5)
    a = np.concatenate([clean, rng.normal(0, 1e-2, 2 * slack).astype(np.float32)])
    b = np.concatenate([clean, np.full(2 * slack, np.nan, np.float32)])
    if stride:
        bb = b.reshape(-1, 2)
        for e in range(n_epochs - 1):
            bb[e * stride + ext: (e + 1) * stride] = np.nan
    dev = torch.device("cuda", 0)
    want = _device_run(cfg, L, n_epochs, stride, r["want_spectrum"], (epw,), torch.from_numpy(a).to(dev))
    got = _device_run(cfg, L, n_epochs, stride, r["want_spectrum"], (epw,), torch.from_numpy(b).to(dev))
    for k in _keys(r):
        assert not torch.isnan(got[k].double()).any(), k
        assert torch.equal(got[k], want[k]), k
    # ... and they are the bits of the dense host-buffer run (the epochs hold the same samples wherever they lie), which is held to float64
    base = streaming_bits(form, n, K, L, n_epochs)
    for k in _keys(r):
        assert np.array_equal(got[k].cpu().numpy(), base[k]), k


@pytest.mark.parametrize("name", ["ref512", "energy1024"])
def test_the_switch_between_the_forms_at_one_epoch_per_compute_unit(built, name):
    """The library's own choice ("auto"): n_cus epochs run the dealt form, n_cus + 1 the streaming form (crn_api.cpp, deal_max).
    Both against the oracle, and bit for bit the same on the epochs they share."""
    import torch
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    cfg, L = (cs.cfg_reference(), 364) if name == "ref512" else (cs.cfg_energy_scaled(1024, 4.0), 1024)
    iq, _ = signals.make_epochs(cfg, n_cus + 1, seed=2025 + cfg.fft_len, L=L)
    want = orc.run(cfg, iq, n_cus + 1, L=L)
    if cfg.decide == cs.DECIDE_ANN:
        assert (np.abs(want["ann_out"] - cfg.ann_threshold) > pol.ANN_MARGIN).all(), "fixture inside the margin band"
    else:
        thr = np.array(cfg.thresh[:cfg.n_bands], np.float32)[None, :] * want["features"][:, cfg.ref_band:cfg.ref_band + 1]
        fin = np.isfinite(thr)
        assert (np.abs(want["features"][fin] / thr[fin] - 1) > pol.THRESHOLD_MARGIN).all(), "fixture inside the margin band"
    s = forms.sensor(cfg, "auto")
    at = s.run_host(iq, n_cus, L=L)
    assert s.dealt_launches() == 1, "one epoch per compute unit: the dealt form"
    above = s.run_host(iq, n_cus + 1, L=L)
    assert s.dealt_launches() == 1, "one epoch more: the streaming form"
    s.close()
    for got, m in ((at, n_cus), (above, n_cus + 1)):
        assert (np.abs(got["features"] - want["features"][:m]) / np.abs(want["features"][:m])).max() < pol.FEATURE_TOL
        assert np.array_equal(got["decision"], want["decision"][:m]) and np.array_equal(got["occupancy"], want["occupancy"][:m])
        if cfg.decide == cs.DECIDE_ANN:
            assert np.abs(got["ann_out"] - want["ann_out"][:m]).max() < 1e-6
    for k in ("features", "occupancy", "decision", "ann_out"):
        assert np.array_equal(at[k], above[k][:n_cus]), k


if __name__ == "__main__":
    # CPU only: every reference's margin clearance and the C oracle's distance from float64, per form (the table of the docstring)
    worst = {}
    for p in _cases(geometries=False):
        form, n, K, L = p.values
        for n_epochs in {N_EPOCHS[n]} | ({N_EPOCHS_ONE_LIVE[n]} if K == 3 and L in (n, 363) else set()):
            r = reference(form, n, K, L, n_epochs)
            try:
                check_reference(r)
            except AssertionError as e:
                print(f"FAIL {form}/{n}/{K}/{L}/{n_epochs}: {e} (min margin {r['margin'].min():.3g})")
            w = worst.setdefault(form, [0.0, 0.0, np.inf])
            w[0] = max(w[0], r["oracle_feature_distance"])
            w[1] = max(w[1], r.get("oracle_per_bin", 0.0))
            w[2] = min(w[2], float(r["margin"].min()))
    for form, (d, pb, m) in worst.items():
        print(f"  {form:18s} features {d:.2e}   per bin {pb:.2e}   smallest margin {m:.2e}")
