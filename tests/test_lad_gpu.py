"""crn_lad_device on the MI355X: the kernel against the twin (tests/lad_f64.py) fed the kernel's own inputs.  On decided rows (every
comparison of the definition further than 2^-36 from equality: include/crn_sense.h) the mask, every integer field, d_floor, floor_min
and floor_max are compared byte for byte; undecided rows are skipped and counted, at most one per test, and
tests/test_lad_host.py::test_the_gpu_tests_rows_are_decided checks that the synthetic rows (tests/lad_cases.py) have none.  Every output
array has 256 bytes of 0xFF behind it that must stay, and NULL outputs must stay unwritten.  Then the optional arguments, cut
independence, the refusals that need a live handle, band-noise traffic end to end next to the CFAR mask, and the cost next to the CFAR
launch alone."""
import ctypes as C
import functools

import numpy as np
import pytest

import crnsense as cs
import lad_cases as lc
import lad_f64 as lf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402

G_, W_ = 2, 16
Q10 = lc.params(10)


@functools.lru_cache(maxsize=None)
def _batch(n):
    return lc.batch(n)[0]


@functools.lru_cache(maxsize=None)
def _twin(n, n_blocks, init_percent):
    """The twin on the whole synthetic batch, computed once: rows are independent, so any slice of it serves."""
    return lf.run(_batch(n), n_blocks, init_percent, **Q10)


def _slice(want, rows):
    return tuple(w[rows] for w in want)


class _Out(sgpu.Padded):
    """The mask, the headers and the floors of a batch on the device, each with 0xFF bytes behind it (stage_gpu.Padded)."""

    def __init__(self, E, n, n_blocks):
        self.E, self.n, self.nb = E, n, n_blocks
        super().__init__(mask=E * n // 8, rows=E * 32, floor=E * n_blocks * 4)

    def host(self):
        super().host()
        return self.view("mask", np.uint32, (self.E, self.n // 32)), self.view("rows", cs.LAD_ROW_DTYPE), self.view("floor", np.float32, (self.E, self.nb))


def _launch(s, spec_t, E, n_blocks, init_percent, q, out, or_ptr=0, mask=True, rows=True, floor=True):
    s.lad_device(spec_t.data_ptr(), E, cs.lad_params(n_blocks, init_percent, **q), mask_ptr=out.mask.data_ptr() if mask else 0,
                 rows_ptr=out.rows.data_ptr() if rows else 0, floor_ptr=out.floor.data_ptr() if floor else 0, or_mask_ptr=or_ptr)
    return out


def _check(s, P, n_blocks, init_percent, what, q=Q10, want=None, or_mask=None, spec_t=None):
    """One launch with every output against the twin.  Returns (the outputs, the number of undecided rows)."""
    E, n = P.shape
    spec_t = sgpu.upload_rows(P) if spec_t is None else spec_t
    out = _Out(E, n, n_blocks)
    or_t = None if or_mask is None else sgpu.upload_mask(or_mask)
    _launch(s, spec_t, E, n_blocks, init_percent, q, out, or_ptr=0 if or_t is None else or_t.data_ptr())
    got = out.host()
    assert out.pads_untouched(), (what, "memory behind an output array was written")
    if want is None:
        want = lf.run(P, n_blocks, init_percent, or_mask=or_mask, **q)
    skipped = lf.compare(got[0], got[1], got[2], want, what)
    return got, skipped


@pytest.mark.parametrize("E", [1, 3, 65])
@pytest.mark.parametrize("n", lc.SIZES)
def test_shapes_against_twin(built, n, E):
    """Every row kind of tests/lad_cases.py, every allowed n_blocks, init_percent 1, 10 and 50.  E = 3 takes the rows from the batch's
    other end, E = 1 the row with one bin 90 dB over the floor."""
    rows = {1: slice(10, 11), 3: slice(lc.E_MAX - 3, lc.E_MAX), 65: slice(0, lc.E_MAX)}[E]
    P = _batch(n)[rows]
    spec_t = sgpu.upload_rows(P)
    s = cs.Sensor(sgpu.cfg(n))
    skipped = 0
    for n_blocks in lc.blocks_allowed(n):
        for ip in lc.INIT_PERCENTS:
            got, sk = _check(s, P, n_blocks, ip, f"N={n} E={E} n_blocks={n_blocks} init_percent={ip}", want=_slice(_twin(n, n_blocks, ip), rows), spec_t=spec_t)
            skipped += sk
    s.close()
    assert skipped <= 1
    if E == 1:
        # the bin 90 dB up is excised: the floor is that of the noise next to it
        assert got[1]["n_clean"][0] < n and 0.5 * lc.MEAN < got[1]["floor_min"][0] <= got[1]["floor_max"][0] < 2.0 * lc.MEAN
    print(f"N={n} E={E}: {skipped} undecided rows skipped")


@pytest.mark.parametrize("n", [512, 4096])
def test_noise_rows_of_other_seeds(built, n):
    """Gamma(K) noise for K = 1 and 10 with the factors of each K, 16 rows each, on the largest number of blocks."""
    rng = np.random.default_rng(n + 17)
    s = cs.Sensor(sgpu.cfg(n))
    skipped = 0
    for k in (1, 10):
        P = rng.gamma(float(k), lc.MEAN / k, (16, n)).astype(np.float32)
        for n_blocks in (1, lc.blocks_allowed(n)[-1]):
            skipped += _check(s, P, n_blocks, 10, f"noise K={k} N={n} n_blocks={n_blocks}", q=lc.params(k))[1]
    s.close()
    assert skipped <= 1


@pytest.mark.parametrize("n", [512, 4096])
def test_lower_all_ones(built, n):
    """t_lower under 1: every bin of a quiet row is over the lower threshold.  With one upper bin (the first, the last and a middle bin of
    the row in turn) the row is one cluster of width N; without one it is one rejected cluster."""
    rng = np.random.default_rng(n)
    q = {"t_cme": 4.0, "t_lower": 0.5, "t_upper": 1.5}
    P = rng.uniform(0.9, 1.1, (4, n)) * lc.MEAN
    for e, k in enumerate((0, n - 1, n // 2 + 7)):
        P[e, k] = 2.0 * lc.MEAN
    P = P.astype(np.float32)
    s = cs.Sensor(sgpu.cfg(n))
    for n_blocks in (1, 2):
        got, skipped = _check(s, P, n_blocks, 10, f"lower all ones N={n} n_blocks={n_blocks}", q=q)
        assert skipped == 0
        assert (got[0][:3] == 0xFFFFFFFF).all() and not got[0][3].any()
        assert list(got[1]["n_clusters"]) == [1, 1, 1, 0] and list(got[1]["n_rejected"]) == [0, 0, 0, 1] and (got[1]["n_lower"] == n).all()
    s.close()


@pytest.mark.parametrize("n", [512, 4096])
def test_optional_arguments(built, n):
    """d_or_mask given, NULL, and the same address as d_bin_mask; each output NULL in turn; n_epochs = 0 touches nothing."""
    E = 14                                                     # one row of every kind
    P = _batch(n)[:E]
    spec_t = sgpu.upload_rows(P)
    n_blocks, ip = lc.blocks_allowed(n)[-1], 10
    want = _slice(_twin(n, n_blocks, ip), slice(0, E))
    rng = np.random.default_rng(n + 1)
    om = rng.random((E, n)) < 0.01
    om[:, [0, 31, 32, n - 1]] = True
    s = cs.Sensor(sgpu.cfg(n))
    plain, _ = _check(s, P, n_blocks, ip, "no d_or_mask", want=want, spec_t=spec_t)
    with_or, _ = _check(s, P, n_blocks, ip, "d_or_mask given", or_mask=om, spec_t=spec_t)
    assert with_or[0].tobytes() == (plain[0] | lf.pack_mask(om)).tobytes() and with_or[2].tobytes() == plain[2].tobytes()
    for f in lf.ROW_INTS:
        assert f == "n_detected" or (with_or[1][f] == plain[1][f]).all()
    # aliased: the mask array holds the mask to OR in and receives the result
    out = _Out(E, n, n_blocks)
    out.mask[: E * n // 8] = torch.from_numpy(lf.pack_mask(om).view(np.uint8).reshape(-1).copy()).to(DEV)
    _launch(s, spec_t, E, n_blocks, ip, Q10, out, or_ptr=out.mask.data_ptr())
    aliased = out.host()
    assert out.pads_untouched()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(aliased, with_or))
    # each output NULL in turn, and two at a time: the others do not change and the NULL one stays 0xFF
    for kw in ({"mask": False}, {"rows": False}, {"floor": False}, {"mask": False, "rows": False}, {"rows": False, "floor": False},
               {"mask": False, "floor": False}):
        out = _launch(s, spec_t, E, n_blocks, ip, Q10, _Out(E, n, n_blocks), **kw)
        got = out.host()
        assert out.pads_untouched(), kw
        for i, name in enumerate(("mask", "rows", "floor")):
            if kw.get(name, True):
                assert got[i].tobytes() == plain[i].tobytes(), (kw, name)
            else:
                assert (out.raw[name] == 255).all(), (kw, name, "a NULL output was written")
    nothing = _launch(s, spec_t, 0, n_blocks, ip, Q10, _Out(E, n, n_blocks))
    torch.cuda.synchronize()
    assert all((x.cpu().numpy() == 255).all() for x in (nothing.mask, nothing.rows, nothing.floor))
    s.close()


@pytest.mark.parametrize("n", [512, 4096])
def test_cut_independence(built, n):
    """65 rows in one call against the same rows cut at 1, at 64, and row by row: the same bytes."""
    E = lc.E_MAX
    P = _batch(n)
    spec_t = sgpu.upload_rows(P)
    n_blocks = lc.blocks_allowed(n)[-1]
    s = cs.Sensor(sgpu.cfg(n))
    whole, _ = _check(s, P, n_blocks, 10, "whole", want=_twin(n, n_blocks, 10), spec_t=spec_t)
    for cuts in ([1], [64], list(range(1, E))):
        edges = [0] + cuts + [E]
        parts = []
        for a, b in zip(edges[:-1], edges[1:]):
            out = _launch(s, spec_t[a:b], b - a, n_blocks, 10, Q10, _Out(b - a, n, n_blocks))
            parts.append(out.host())
            assert out.pads_untouched()
        for i in range(3):
            assert np.concatenate([p[i] for p in parts]).tobytes() == whole[i].tobytes(), (cuts[:3], i)
    s.close()


def test_refusals_with_a_live_handle(built):
    """Every refusal of the header's list with a live handle; n_blocks is checked against the handle's fft_len."""
    n, E = 512, 4
    L = cs.lib()
    s = cs.Sensor(sgpu.cfg(n))
    spec_t = sgpu.upload_rows(_batch(n)[:E])
    out = _Out(E, n, 2)
    or_t = torch.zeros((E * n // 32,), dtype=torch.int32, device=DEV)
    inf, nan = float("inf"), float("nan")

    def rc(sp=spec_t.data_ptr(), n_e=E, q=None, orp=or_t.data_ptr(), m=out.mask.data_ptr(), r=out.rows.data_ptr(), f=out.floor.data_ptr(),
           reserved=(0, 0, 0), n_blocks=2, init_percent=10, **kw):
        if q is None:
            q = cs.lad_params(n_blocks, init_percent, **{**Q10, **kw})
            for i, x in enumerate(reserved):
                q.reserved[i] = x
        v = lambda p: C.c_void_p(p or None)      # noqa: E731
        return L.crn_lad_device(s._h, v(sp), n_e, C.byref(q) if q != 0 else None, v(orp), v(m), v(r), v(f), None)
    assert rc() == 0
    for bad in ({"sp": 0}, {"q": 0}, {"m": 0, "r": 0, "f": 0}, {"n_e": -1},
                {"n_blocks": 0}, {"n_blocks": 3}, {"n_blocks": 4}, {"n_blocks": 8}, {"n_blocks": 16}, {"n_blocks": -1},
                {"init_percent": 0}, {"init_percent": 51}, {"init_percent": -1},
                {"t_cme": 0.0}, {"t_cme": -1.0}, {"t_cme": inf}, {"t_cme": nan},
                {"t_lower": 0.0}, {"t_lower": -2.0}, {"t_lower": nan}, {"t_upper": inf}, {"t_upper": nan}, {"t_upper": 0.0},
                {"t_lower": 3.0, "t_upper": 2.0},
                {"reserved": (1, 0, 0)}, {"reserved": (0, 1, 0)}, {"reserved": (0, 0, -1)},
                {"sp": spec_t.data_ptr() + 4}, {"sp": spec_t.data_ptr() + 8}, {"r": out.rows.data_ptr() + 8}, {"m": out.mask.data_ptr() + 4},
                {"orp": or_t.data_ptr() + 4}, {"f": out.floor.data_ptr() + 2}):
        assert rc(**bad) == cs.CRN_ERR_ARG, bad
        assert b"crn_lad_device" in L.crn_last_error(), bad
    assert rc(n_e=0) == 0 and rc(orp=0) == 0 and rc(m=0, r=0) == 0 and rc(f=out.floor.data_ptr() + 4) == 0 and rc(n_blocks=1) == 0
    assert rc(t_lower=2.0, t_upper=2.0) == 0 and rc(init_percent=1) == 0 and rc(init_percent=50) == 0
    torch.cuda.synchronize()
    s.close()
    # a 4096-point handle takes eight blocks, a 1024-point one four and not eight
    for n, ok, bad in ((4096, 8, 16), (1024, 4, 8)):
        s = cs.Sensor(sgpu.cfg(n))
        sp = sgpu.upload_rows(_batch(n)[:1])
        o = _Out(1, n, 8)
        for nb, want in ((ok, 0), (bad, cs.CRN_ERR_ARG)):
            q = cs.lad_params(nb, 10, **Q10)
            assert L.crn_lad_device(s._h, C.c_void_p(sp.data_ptr()), 1, C.byref(q), None, C.c_void_p(o.mask.data_ptr()), None, None, None) == want
        torch.cuda.synchronize()
        s.close()


# the traffic of tests/test_holes_gpu.py's end-to-end test with band noise in the place of tones, 100 epochs to a stream
E2E = {"n": 512, "k": 10, "n_streams": 4, "eps": 100, "pfa": 1e-3, "seed": 2031, "noise_power": 1e-6, "signal_rms": 0.02,
       "spans": [(300, 10), (496, 32), (55, 30), (189, 33)]}
LAD_BAR, CFAR_BAR, OUTSIDE_BAR, SEGMENT_BAR = 0.98, 0.2, 1e-3, 0.95      # tests/test_lad_host.py::test_band_filling_emitter_cfar_against_lad


def test_end_to_end_band_noise(built):
    """The intended Markov chain of crn_synth_fill_device_ex driving band noise (every bin of the busy channel: 30-33 bins wide, the
    width of the reference's transmitters at N = 512), 4 streams x 100 epochs, K = 10, rect.  One CFAR launch (CA, guard 2, train 16,
    Pfa 1e-3), then crn_lad_device on its `spectrum` with FCME and lower at 1e-2, upper at 1e-4, one block.  Pooled over all epochs the
    LAD mask holds at least 0.98 of the driven channel's bins and the CFAR mask at most 0.2; outside every channel LAD stays under 1e-3;
    crn_segments_device (merge_gap 2, min_width 8) on the LAD mask finds, in at least 95 % of the epochs, exactly one segment that
    overlaps the driven channel, and it covers at least 0.9 of it.  Every row equals the twin."""
    n, k, S, T = E2E["n"], E2E["k"], E2E["n_streams"], E2E["eps"]
    E = S * T
    cfg = sgpu.cfg(n, k=k)
    iq_t = torch.zeros((cs.samples_needed(cfg, E) * 2,), dtype=torch.float32, device=DEV)
    truth_t = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    sc = cs.SynthCfg()
    sc.seed, sc.noise_power, sc.signal_rms = E2E["seed"], E2E["noise_power"], E2E["signal_rms"]
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = 0, cs.PU_MARKOV_INTENDED, cs.SIG_BAND_NOISE, S
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), E, cs.samples_per_epoch(cfg), sc, truth_ptr=truth_t.data_ptr())
    s.set_cfar(G_, W_, cs.cfar_alpha(E2E["pfa"], k, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, iq_t, E, band_bins=False)
    t_cme = cs.lad_factor(1e-2, k)
    q = {"t_cme": t_cme, "t_lower": cs.lad_factor(1e-2, k, t_cme), "t_upper": cs.lad_factor(1e-4, k, t_cme)}
    out = _launch(s, outs["spectrum"], E, 1, 10, q, _Out(E, n, 1))
    seg_e = torch.full((E * 16,), 255, dtype=torch.uint8, device=DEV)
    seg_s = torch.full((E * 16 * 32,), 255, dtype=torch.uint8, device=DEV)
    s.segments_device(out.mask.data_ptr(), outs["spectrum"].data_ptr(), E, seg_e.data_ptr(), seg_s.data_ptr(), merge_gap=2, min_width=8, max_segments=16)
    got = out.host()
    assert out.pads_untouched()
    P = outs["spectrum"].cpu().numpy()
    truth = truth_t.cpu().numpy()
    cfar = lf.unpack_mask(outs["mask"].cpu().numpy().view(np.uint32), n)
    heads = np.frombuffer(seg_e.cpu().numpy().tobytes(), np.dtype(cs.SEGMENT_EPOCH_DTYPE))
    segs = np.frombuffer(seg_s.cpu().numpy().tobytes(), np.dtype(cs.SEGMENT_DTYPE)).reshape(E, 16)
    s.close()
    skipped = lf.compare(got[0], got[1], got[2], lf.run(P, 1, 10, **q), "end to end")
    lad = lf.unpack_mask(got[0], n)
    assert set(np.unique(truth)) <= {1, 2, 3}
    chan = np.zeros((4, n), bool)
    for c in (1, 2, 3):
        lo, w = E2E["spans"][c]
        chan[c, (lo + np.arange(w)) % n] = True
    driven = chan[truth]                                           # [E, n]
    outside = ~chan[1:].any(axis=0)
    lad_share, cfar_share = lad[driven].mean(), cfar[driven].mean()
    lad_outside = lad[:, outside].mean()
    good = 0
    for e in range(E):
        over = []
        for sg in segs[e, : heads[e]["n_stored"]]:
            inside = np.zeros(n, bool)
            inside[(sg["lo"] + np.arange(sg["width"])) % n] = True
            if (inside & driven[e]).any():
                over.append((inside & driven[e]).sum() / driven[e].sum())
        good += len(over) == 1 and over[0] >= 0.9
    print(f"end to end, {E} epochs of band noise: driven channel's bins set by LAD {lad_share:.4f} (bar {LAD_BAR}), by CA-CFAR {cfar_share:.4f} "
          f"(bar {CFAR_BAR}); LAD outside every channel {lad_outside:.2e} (bar {OUTSIDE_BAR}); epochs with exactly one segment over the driven "
          f"channel covering 0.9 of it {good / E:.4f} (bar {SEGMENT_BAR}); undecided rows {skipped}")
    assert lad_share >= LAD_BAR and cfar_share <= CFAR_BAR
    assert lad_outside < OUTSIDE_BAR
    assert good >= SEGMENT_BAR * E


# CFAR launch + crn_lad_device against the CFAR launch alone, `spectrum` written in both arms, with the margin of
# tests/test_holes_gpu.py: 1 + 1.5 x (the larger measured B / A - 1).  Measured on an MI355X in two separate runs (profiles/r16_lad.txt,
# DESIGN.md §5): arm A 426.5 us, B / A = 1.2443, the stage alone 99.0 us; arm A 396.3 us, B / A = 1.2711, alone 102.5 us.
SPEED_RATIO = 1.407


def test_cost_next_to_the_cfar_launch(built):
    """N = 4096, K = 10, rect, 64 bands, 6656 epochs; the method of tests/stage_gpu.py (best_of_windows): each timed window holds 8
    launches issued back to back behind one already queued, the arms alternate, 5 windows each after a warm-up, the best counts.  Arm A
    is the CFAR launch alone, arm B the same launch followed by crn_lad_device on the same stream with all outputs, d_or_mask the CFAR
    mask, n_blocks = 8.  The stage alone is measured the same way and printed."""
    n, k = 4096, 10
    cfg = sgpu.cfg(n, k=k, bands=64)
    E = 6656                                  # 6656 x 10 x 4096 x 8 B = 2.18 GB
    # the traffic of every cost test here: tones over unit noise in two epochs of three
    iq_t = sgpu.add_tones(sgpu.noise_batch(E, k, n), E, k, n)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = sgpu.cfar_outs(cfg, E)
    out = _Out(E, n, 8)

    def arm_a():
        sgpu.cfar_launch(s, cfg, iq_t, E, outs=outs)

    def stage():
        _launch(s, outs["spectrum"], E, 8, 10, Q10, out, or_ptr=outs["mask"].data_ptr())

    def arm_b():
        arm_a()
        stage()
    arms = {"A": arm_a, "B": arm_b, "alone": stage}
    times = sgpu.best_of_windows(arms)
    got = out.host()
    assert out.pads_untouched()
    # the stage computed what the definition says: every 16th row against the twin on the kernel's own inputs
    pick = slice(0, E, 16)
    P = outs["spectrum"][pick].cpu().numpy()
    cfar = lf.unpack_mask(outs["mask"][pick].cpu().numpy().view(np.uint32), n)
    s.close()
    skipped = lf.compare(got[0][pick], got[1][pick], got[2][pick], lf.run(P, 8, 10, or_mask=cfar, **Q10), "cost batch")
    best = {name: min(v) for name, v in times.items()}
    nbytes = E * k * n * 8
    print(f"N=4096 K=10 rect 64 bands, {E} epochs ({nbytes / 1e9:.2f} GB), spectrum written: arm A (CFAR launch alone) {best['A']:.4f} ms "
          f"({nbytes / best['A'] / 1e6:.0f} GB/s of input); B / A = {best['B'] / best['A']:.4f}; crn_lad_device alone {best['alone'] * 1e3:.1f} us; "
          f"undecided rows of {P.shape[0]} checked: {skipped}")
    assert got[1]["n_detected"].sum() > 0
    assert best["B"] <= SPEED_RATIO * best["A"], (best["B"] / best["A"], SPEED_RATIO)
