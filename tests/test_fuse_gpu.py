"""crn_fuse_device on the MI355X: the kernel against the twin (tests/fuse_f64.py) fed the kernel's own inputs.  The definition leaves no
rounding freedom, so the comparison is exact: d_fused_mask, d_rows and d_fused_spectrum equal byte for byte, memory past the arrays still
the 0xFF fill, a NULL output left as 0xFF.  Then the inactive members, the strong neighbour, cut independence, the identity and the chain
into the segment and channel stages, the sensing kernel's own CA detector, a swept emitter end to end, the refusals that need a live
handle, and the cost next to the CFAR launch alone."""
import ctypes as C

import numpy as np
import pytest

import crnsense as cs
import fuse_f64 as fu

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402

G_, W_ = 2, 16
SIZES = (512, 1024, 2048, 4096)


class _Out(sgpu.Padded):
    """The fused mask, the fused rows and the headers of R fused rows on the device, each with 0xFF bytes behind it (stage_gpu.Padded)."""

    def __init__(self, R, n):
        self.R, self.n = R, n
        super().__init__(mask=R * n // 8, spec=R * n * 4, rows=R * 16)

    def host(self):
        """(mask words [R][n / 32] uint32, fused rows [R][n] float32, headers [R]); the three as bytes in .raw."""
        payload = super().host()
        self.raw = tuple(payload[name].tobytes() for name in ("mask", "spec", "rows"))
        return (np.frombuffer(self.raw[0], np.uint32).reshape(self.R, self.n // 32), np.frombuffer(self.raw[1], np.float32).reshape(self.R, self.n),
                np.frombuffer(self.raw[2], cs.FUSE_ROW_DTYPE))


def _upload(det, P):
    return None if det is None else sgpu.upload_mask(det), None if P is None else sgpu.upload_rows(P)


def _run(s, mask_t, spec_t, E, q, n, out=None, want=(True, True, True)):
    out = _Out(E // q.group_size, n) if out is None else out
    s.fuse_device(0 if mask_t is None else mask_t.data_ptr(), 0 if spec_t is None else spec_t.data_ptr(), E, q,
                  fused_mask_ptr=out.mask.data_ptr() if want[0] else 0, fused_spectrum_ptr=out.spec.data_ptr() if want[1] else 0,
                  rows_ptr=out.rows.data_ptr() if want[2] else 0)
    return out


def _params(rule, M, T, w, votes=0, guard=0, train=0, alpha=0.0):
    return cs.fuse_params(rule, M, T, votes=votes, guard=guard, train=train, alpha=alpha, weights=[float(x) for x in w])


def _want(det, P, M, T, w, rule, n, **kw):
    """The twin's three arrays as bytes; the fused row all 0xFF where none is written (no spectrum)."""
    fused, F, rows = fu.fuse(det, P, M, T, w, rule, **kw)
    return (fu.pack_mask(fused).tobytes(), F.tobytes() if F is not None else b"\xff" * (fused.shape[0] * n * 4), rows.tobytes()), fused, F, rows


def _check(s, mask_t, spec_t, det, P, n, M, T, w, rule, what, **kw):
    """One call with all three outputs against the twin, byte for byte.  Returns the twin's (fused det, fused row, headers)."""
    E = (det if det is not None else P).shape[0]
    q = _params(rule, M, T, w, **kw)
    out = _run(s, mask_t, spec_t, E, q, n, want=(True, P is not None, True))
    got = out.host()
    assert out.pads_untouched(), (what, "memory behind an output array was written")
    want, fused, F, rows = _want(det, P, M, T, w, rule, n, **kw)
    assert out.raw[0] == want[0], (what, "d_fused_mask", np.argwhere(fu.unpack_mask(got[0], n) != fused)[:6])
    assert out.raw[2] == want[2], (what, "d_rows", got[2][:4], rows[:4])
    assert out.raw[1] == want[1], (what, "d_fused_spectrum", np.argwhere(got[1].view(np.uint32) != np.frombuffer(want[1], np.uint32).reshape(-1, n))[:6])
    return fused, F, rows


def _weight_sets(M, rng):
    """Equal gain, random unequal, and zeros at member 0, at the last member and at all but one member."""
    sets = {"equal": np.array(fu.equal_gain(M), np.float32), "unequal": rng.uniform(0.05, 3.0, M).astype(np.float32)}
    if M > 1:
        for name, zero in (("no member 0", [0]), ("no last member", [M - 1]), ("one member", [m for m in range(M) if m != M // 2])):
            w = rng.uniform(0.05, 3.0, M).astype(np.float32)
            w[zero] = 0.0
            sets[name] = w
    return sets


def _batch(rng, E, n):
    """Random masks (rows at densities 0, 0.002, 0.5 and 1) and Gamma rows with 2 % outliers x 1e4."""
    det = rng.random((E, n)) < np.array([0.0, 0.002, 0.5, 1.0])[rng.integers(0, 4, E)][:, None]
    P = (rng.gamma(10.0, 1e-4, (E, n)) * np.where(rng.random((E, n)) < 0.02, 1e4, 1.0)).astype(np.float32)
    return det, P


@pytest.mark.parametrize("n", SIZES)
def test_shapes_against_twin(built, n):
    """Every (M, G, T), every weight set, VOTE at k = 1, the majority and n_active (with and without the spectrum), SOFT at the four
    windows (the last fills 2 (g + W) + 1 = N - 1) and three alphas (with and without the masks)."""
    rng = np.random.default_rng(n)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    for M, G, T in ((1, 1, 1), (2, 1, 3), (3, 2, 1), (32, 1, 2), (5, 2, 3)):
        E = M * G * T
        det, P = _batch(rng, E, n)
        mask_t, spec_t = _upload(det, P)
        for name, w in _weight_sets(M, rng).items():
            na = int((w > 0).sum())
            what = f"N={n} M={M} G={G} T={T} weights {name}"
            for k in sorted({1, (na + 1) // 2, na}):
                _check(s, mask_t, spec_t, det, P, n, M, T, w, fu.VOTE, what + f" VOTE {k}", votes=k)
            _check(s, mask_t, None, det, None, n, M, T, w, fu.VOTE, what + " VOTE without spectrum", votes=na)
            for g, W, alpha in ((0, 1, 0.5), (2, 16, cs.cfar_alpha(1e-2, M * 10, 16)), (0, 64, 0.5), (n // 2 - 65, 64, 1.5)):
                _check(s, mask_t, spec_t, det, P, n, M, T, w, fu.SOFT, what + f" SOFT g={g} W={W} alpha={alpha:.3f}", guard=g, train=W, alpha=alpha)
            _check(s, None, spec_t, None, P, n, M, T, w, fu.SOFT, what + " SOFT without masks", guard=2, train=16, alpha=1.5)
    s.close()


def test_null_outputs_are_left_alone(built):
    """Each output NULL in turn, under both rules: the others are the same bytes and the NULL one is still 0xFF; a SOFT call without
    d_fused_spectrum (the fused row lives in LDS only) detects the same bins."""
    n, M, G, T = 1024, 4, 2, 3
    rng = np.random.default_rng(77)
    det, P = _batch(rng, M * G * T, n)
    mask_t, spec_t = _upload(det, P)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    w = fu.equal_gain(M)
    for q in (_params(fu.VOTE, M, T, w, votes=2), _params(fu.SOFT, M, T, w, guard=G_, train=W_, alpha=1.5)):
        full = _run(s, mask_t, spec_t, det.shape[0], q, n)
        full.host()
        for drop in range(3):
            want = tuple(i != drop for i in range(3))
            part = _run(s, mask_t, spec_t, det.shape[0], q, n, want=want)
            part.host()
            assert part.pads_untouched()
            for i in range(3):
                assert part.raw[i] == (full.raw[i] if want[i] else b"\xff" * len(full.raw[i])), (q.rule, drop, i)
    s.close()


@pytest.mark.parametrize("n", [512, 4096])
def test_inactive_members_are_skipped(built, n):
    """The members of weight 0 hold NaN rows and masks of all ones: every output equals the call on the batch without them."""
    rng = np.random.default_rng(n + 1)
    M, G, T = 6, 2, 3
    keep = [1, 2, 4]
    w = np.zeros(M, np.float32)
    w[keep] = rng.uniform(0.1, 2.0, len(keep)).astype(np.float32)
    det, P = _batch(rng, M * G * T, n)
    det4, P4 = det.reshape(G, M, T, n).copy(), P.reshape(G, M, T, n).copy()
    small = (det4[:, keep].reshape(-1, n), P4[:, keep].reshape(-1, n))
    for m in range(M):
        if m not in keep:
            det4[:, m], P4[:, m] = True, np.nan
    det, P = det4.reshape(-1, n), P4.reshape(-1, n)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    mask_t, spec_t = _upload(det, P)
    mask_s, spec_s = _upload(*small)
    for rule, kw in ((fu.VOTE, {"votes": 2}), (fu.SOFT, {"guard": G_, "train": W_, "alpha": 1.2})):
        big = _run(s, mask_t, spec_t, det.shape[0], _params(rule, M, T, w, **kw), n)
        sm = _run(s, mask_s, spec_s, small[0].shape[0], _params(rule, len(keep), T, w[keep], **kw), n)
        big.host(), sm.host()
        assert big.raw == sm.raw and big.pads_untouched()
        _check(s, mask_t, spec_t, det, P, n, M, T, w, rule, f"inactive members N={n} rule {rule}", **kw)
    s.close()


@pytest.mark.parametrize("n", [512, 4096])
def test_strong_neighbour(built, n):
    """SOFT with a bin 90 dB over the floor at distance g + W + 1 (outside every window of the tested bin: it changes nothing) and at g + W
    (the outermost training cell: T rises by exactly that value), on either side, across the wrap too.  Equal to the twin exactly; the
    twin's T at the tested bins is the direct sum, small when the strong bin is the far one and large when it is the near one."""
    rng = np.random.default_rng(n + 90)
    M, T, g, W = 3, 4, 2, 16
    E = M * T
    # (tested bin, side, far): the tested bins of one batch lie further apart than two windows; bins 5 and n - 7 reach across the wrap
    batches = ([(5, -1, True), (259, -1, False), (200, +1, False), (331, +1, True)], [(5, -1, False), (331, +1, False)],
               [(n - 7, +1, True), (259, +1, True)], [(n - 7, +1, False), (200, -1, True)])
    w = rng.uniform(0.2, 1.0, M).astype(np.float32)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    for batch in batches:
        P = rng.gamma(10.0, 1e-4, (E, n))
        for k, side, far in batch:
            P[:, (k + side * (g + W + (1 if far else 0))) % n] = 1e-3 * 1e9 * rng.uniform(0.5, 2.0, E)
        P = P.astype(np.float32)
        _, spec_t = _upload(None, P)
        _, F, _ = _check(s, None, spec_t, None, P, n, M, T, w, fu.SOFT, f"strong neighbour N={n} {batch}", guard=g, train=W, alpha=1.5)
        Tsum = fu.soft_detect(F, g, W, 1.5)[1]
        Fd = F.astype(np.float64)
        for k, side, far in batch:
            direct = sum(Fd[:, (k - i) % n] + Fd[:, (k + i) % n] for i in range(g + 1, g + W + 1))
            assert np.allclose(Tsum[:, k], direct, rtol=1e-12)
            assert (Tsum[:, k] < 1.0).all() if far else (Tsum[:, k] > 1e5).all(), (k, side, far, Tsum[:, k])
    s.close()


def test_cut_independence(built):
    """One call on (G = 3, T = 40) against the same batch cut along time at 1, 17 and 39 (the members' epochs gathered into contiguous
    sub-batches) and cut into the three groups: the same bytes."""
    n, M, G, T = 512, 4, 3, 40
    rng = np.random.default_rng(40)
    det, P = _batch(rng, M * G * T, n)
    mask_t, spec_t = _upload(det, P)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    w = rng.uniform(0.1, 1.0, M).astype(np.float32)
    for rule, kw in ((fu.VOTE, {"votes": 2}), (fu.SOFT, {"guard": G_, "train": W_, "alpha": 1.3})):
        whole = _run(s, mask_t, spec_t, det.shape[0], _params(rule, M, T, w, **kw), n)
        whole.host()
        parts = [[], [], []]
        edges = [0, 1, 17, 39, T]
        for a, b in zip(edges[:-1], edges[1:]):
            m_t = mask_t.view(G * M, T, -1)[:, a:b].contiguous()
            p_t = spec_t.view(G * M, T, -1)[:, a:b].contiguous()
            part = _run(s, m_t, p_t, G * M * (b - a), _params(rule, M, b - a, w, **kw), n)
            part.host()
            assert part.pads_untouched()
            for i, per_row in enumerate((n // 8, n * 4, 16)):
                parts[i].append(np.frombuffer(part.raw[i], np.uint8).reshape(G, b - a, per_row))
        for i in range(3):
            assert np.concatenate(parts[i], axis=1).tobytes() == whole.raw[i], (rule, "time", i)
        groups = [b"", b"", b""]
        for j in range(G):
            part = _run(s, mask_t.view(G, M * T, -1)[j].contiguous(), spec_t.view(G, M * T, -1)[j].contiguous(), M * T, _params(rule, M, T, w, **kw), n)
            part.host()
            groups = [a + b for a, b in zip(groups, part.raw)]
        assert tuple(groups) == whole.raw, (rule, "groups")
    s.close()


def test_identity_and_chain(built):
    """M = 1, w = 1, VOTE k = 1 returns the input bytes.  The fused outputs of (M = 4, G = 2, T = 6) go to crn_segments_device and
    crn_channels_device with n_epochs = 12: the same bytes as those stages run on the twin's fused arrays."""
    n = 1024
    rng = np.random.default_rng(5)
    s = cs.Sensor(sgpu.cfg(n, cs.WINDOW_RECT, 10))
    det, P = _batch(rng, 7, n)
    mask_t, spec_t = _upload(det, P)
    out = _run(s, mask_t, spec_t, 7, _params(fu.VOTE, 1, 7, [1.0], votes=1), n)
    out.host()
    assert out.raw[0] == fu.pack_mask(det).tobytes() and out.raw[1] == P.tobytes() and out.pads_untouched()

    M, G, T = 4, 2, 6
    R = G * T
    det = rng.random((M * R, n)) < 0.004
    det[:, 100:130] |= rng.random((M * R, 30)) < 0.7
    P = (rng.gamma(10.0, 1e-4, (M * R, n)) * np.where(det, 8.0, 1.0)).astype(np.float32)
    mask_t, spec_t = _upload(det, P)
    w = fu.equal_gain(M)
    fused = _run(s, mask_t, spec_t, M * R, _params(fu.VOTE, M, T, w, votes=2), n)
    fused.host()
    twin_det, twin_F, _ = fu.fuse(det, P, M, T, w, fu.VOTE, votes=2)
    twin_mask_t, twin_spec_t = _upload(twin_det, twin_F)
    spans = [(90, 50), (n - 8, 16), (500, 64)]
    results = []
    for m_ptr, p_ptr in ((fused.mask.data_ptr(), fused.spec.data_ptr()), (twin_mask_t.data_ptr(), twin_spec_t.data_ptr())):
        ep = torch.full((R * 16,), 255, dtype=torch.uint8, device=DEV)
        sg = torch.full((R * 8 * 32,), 255, dtype=torch.uint8, device=DEV)
        s.segments_device(m_ptr, p_ptr, R, ep.data_ptr(), sg.data_ptr(), merge_gap=2, min_width=1, max_segments=8)
        ws_bytes = cs.channels_workspace_bytes(R, spans, T)
        st = torch.full((G * len(spans) * 192,), 255, dtype=torch.uint8, device=DEV)
        ws = torch.full((ws_bytes,), 255, dtype=torch.uint8, device=DEV)
        s.channels_device(m_ptr, p_ptr, R, st.data_ptr(), ws.data_ptr(), ws_bytes, spans, epochs_per_stream=T, first=True)
        torch.cuda.synchronize()
        results.append((ep.cpu().numpy().tobytes(), sg.cpu().numpy().tobytes(), st.cpu().numpy().tobytes()))
    s.close()
    assert results[0] == results[1]
    heads = np.frombuffer(results[0][0], cs.SEGMENT_EPOCH_DTYPE)
    assert (heads["n_found"] >= 1).all()                                  # the emitter of bins 100 .. 129 is there to be found


def test_against_the_sensing_kernels_ca_detector(built):
    """N = 512, K = 10, rect, signals.make_epochs traffic: SOFT with M = 1, w = 1 and the handle's g, W and alpha, on the launch's own
    `spectrum`, against the launch's mask.  The two evaluate the same inequality, the fusion in fp64 and the sensing kernel in fp32, so
    a bin may differ only where the two sides are closer than the fp32 evaluation resolves: |F[k] 2W / (alpha T) - 1| <=
    (2 W + 8) 2^-24 in float64 (the in-kernel fp32 additions of 2 W non-negative cells, at most one ulp each, the 1 / K rounding of each
    row value, and the rounding of alpha / 2W)."""
    import signals
    n, k, E = 512, 10, 64
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k)
    iq, _ = signals.make_epochs(cfg, E, seed=512)
    s = cs.Sensor(cfg)
    alpha = cs.cfar_alpha(1e-2, k, W_)
    s.set_cfar(G_, W_, alpha, 1)
    outs = sgpu.cfar_launch(s, cfg, torch.from_numpy(iq).to(DEV), E)
    q = _params(fu.SOFT, 1, E, [1.0], guard=G_, train=W_, alpha=alpha)
    out = _run(s, None, outs["spectrum"], E, q, n)
    words, F, rows = out.host()
    P = outs["spectrum"].cpu().numpy()
    own = fu.unpack_mask(outs["mask"].cpu().numpy().view(np.uint32), n)
    s.close()
    assert F.tobytes() == P.tobytes() and out.pads_untouched()
    got = fu.unpack_mask(words, n)
    twin, T = fu.soft_detect(P, G_, W_, alpha)
    assert (got == twin).all()
    differ = np.argwhere(got != own)
    ratio = P.astype(np.float64) * (2 * W_) / (np.float64(np.float32(alpha)) * T)
    bound = (2 * W_ + 8) * 2.0 ** -24
    worst = max((abs(ratio[e, b] - 1.0) for e, b in differ), default=0.0)
    print(f"{len(differ)} of {got.size} bins differ from the launch's mask ({int(own.sum())} detected); the furthest from the threshold "
          f"|ratio - 1| = {worst:.3e} (bound {bound:.3e})")
    assert own.sum() > 100
    assert worst <= bound, [(int(e), int(b), float(ratio[e, b])) for e, b in differ[:8]]


E2E = {"n": 512, "k": 10, "members": 8, "eps": 200, "pfa": 1e-2, "seed": 77, "noise_power": 1e-6, "signal_rms": 1.1e-4, "tones": 8, "min_bins": 3}


def _band_rate(det, truth, bands, min_bins):
    """The share of epochs in which at least min_bins bins of the driven band are detected."""
    hits = 0
    for e in range(det.shape[0]):
        hits += sum(int(det[e, lo:hi].sum()) for lo, hi in bands[int(truth[e])]) >= min_bins
    return hits / det.shape[0]


def test_end_to_end_swept_emitter(built):
    """crn_synth_fill_device_ex, CRN_PU_SWEEP (band 1, 2, 3, 2, 1, .. the same in every stream: all sensors see the same band), 8 tones
    per band, N = 512, K = 10, 8 streams of 200 epochs with independent noise, one CFAR launch (guard 2, train 16, Pfa 1e-2 per sensor),
    then SOFT fusion of the 8 with alpha = cfar_alpha(1e-2, 80, 16).  Band detection = at least 3 detected bins in the driven band.
    signal_rms = 1.1e-4 over noise_power 1e-6 puts each of the 8 tones at 512 x (1.1e-4)^2 / 8 / 1e-6 = 0.77 (-1.1 dB) of the floor of its
    bin.  Chosen with the twin on the CPU (the generator's CPU twin, tests/oracle_py.synth, the same seed; rows by numpy's FFT): the eight
    sensors' band detection rates were 0.200 .. 0.300, the fused row's 1.000, and 19 fused false alarms fell in the reference band (bins
    300 .. 309, never driven: 2000 trials, 20 expected); at 1.0e-4 the sensors reach 0.09 .. 0.19, at 1.5e-4 already 0.90 .. 0.95.
    Asserted here: every member stays below one half, the fused rate exceeds every member's, the kernel equals the twin exactly, and
    the fused false alarms in the reference band stay within 15 % of pfa x trials plus 4 binomial standard deviations."""
    n, k, M, T = E2E["n"], E2E["k"], E2E["members"], E2E["eps"]
    E = M * T
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k)
    iq_t = sgpu.zeros((cs.samples_needed(cfg, E) * 2,), torch.float32)
    truth_t = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    sc = cs.SynthCfg()
    sc.seed, sc.noise_power, sc.signal_rms = E2E["seed"], E2E["noise_power"], E2E["signal_rms"]
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = E2E["tones"], cs.PU_SWEEP, cs.SIG_TONES, M
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), E, cs.samples_per_epoch(cfg), sc, truth_ptr=truth_t.data_ptr())
    s.set_cfar(G_, W_, cs.cfar_alpha(E2E["pfa"], k, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, iq_t, E)
    alpha = cs.cfar_alpha(E2E["pfa"], M * k, W_)
    w = fu.equal_gain(M)
    out = _run(s, outs["mask"], outs["spectrum"], E, _params(fu.SOFT, M, T, w, guard=G_, train=W_, alpha=alpha), n)
    words, F, rows = out.host()
    truth = truth_t.cpu().numpy().reshape(M, T)
    det = fu.unpack_mask(outs["mask"].cpu().numpy().view(np.uint32), n)
    P = outs["spectrum"].cpu().numpy()
    s.close()
    assert (truth == truth[0]).all() and set(truth[0]) == {1, 2, 3}                  # every sensor saw the same band
    want = _want(det, P, M, T, w, fu.SOFT, n, guard=G_, train=W_, alpha=alpha)[0]
    assert out.raw == want and out.pads_untouched()
    fused = fu.unpack_mask(words, n)
    bands = {}
    for sg in cfg.segs[: cfg.n_segs]:
        bands.setdefault(sg.band, []).append((sg.lo, sg.hi))
    members = [_band_rate(det.reshape(M, T, n)[m], truth[0], bands, E2E["min_bins"]) for m in range(M)]
    rate = _band_rate(fused, truth[0], bands, E2E["min_bins"])
    (lo, hi), = bands[cfg.ref_band]
    trials = T * (hi - lo)
    fa, mean = int(fused[:, lo:hi].sum()), E2E["pfa"] * trials
    slack = 0.15 * mean + 4.0 * np.sqrt(trials * E2E["pfa"] * (1.0 - E2E["pfa"]))
    print(f"band detection rate: members {' '.join(f'{r:.3f}' for r in members)}, fused {rate:.3f}; fused false alarms in the reference band "
          f"{fa} of {trials} (expected {mean:.1f} +- {slack:.1f}); members' false alarms there {int(det[:, lo:hi].sum())} of {M * trials}")
    assert max(members) < 0.5
    assert rate > max(members)
    assert abs(fa - mean) <= slack


def test_refusals_with_a_live_handle(built):
    """Every refusal of the header, one argument at a time; a REF_MAG handle works on uploaded arrays like any other."""
    n, M, T = 512, 4, 2
    E = M * T
    L = cs.lib()
    s = cs.Sensor(cs.cfg_reference())        # REF_MAG, ANN decision: CFAR cannot even be switched on here
    assert s.get_cfar() is None
    rng = np.random.default_rng(0)
    det, P = _batch(rng, E, n)
    mask_t, spec_t = _upload(det, P)
    w = fu.equal_gain(M)
    _check(s, mask_t, spec_t, det, P, n, M, T, w, fu.VOTE, "REF_MAG handle, VOTE", votes=2)
    _check(s, mask_t, spec_t, det, P, n, M, T, w, fu.SOFT, "REF_MAG handle, SOFT", guard=G_, train=W_, alpha=1.5)
    out = _Out(E // M, n)
    inf, nan = float("inf"), float("nan")

    def rc(soft=False, m=mask_t.data_ptr(), sp=spec_t.data_ptr(), n_e=E, q=None, fm=out.mask.data_ptr(), fs=out.spec.data_ptr(), ro=out.rows.data_ptr(),
           h=True, **edit):
        if q is None:
            q = _params(fu.SOFT, M, T, w, guard=G_, train=W_, alpha=1.5) if soft else _params(fu.VOTE, M, T, w, votes=2)
            for f, val in edit.items():
                if f[0] == "w" and f[1:].isdigit():
                    q.weight[int(f[1:])] = val
                elif f[0] == "r" and f[1:].isdigit():
                    q.reserved[int(f[1:])] = val
                else:
                    setattr(q, f, val)
        v = lambda p: C.c_void_p(p or None)      # noqa: E731
        return L.crn_fuse_device(s._h if h else None, v(m), v(sp), n_e, C.byref(q) if q != 0 else None, v(fm), v(fs), v(ro), None)
    assert rc() == 0 and rc(soft=True) == 0
    both = ({"h": False}, {"q": 0}, {"fm": 0, "fs": 0, "ro": 0}, {"rule": -1}, {"rule": 2}, {"group_size": 0}, {"group_size": 33}, {"group_size": -4},
            {"epochs_per_stream": 0}, {"epochs_per_stream": -2}, {"epochs_per_stream": 3}, {"group_size": 3}, {"n_e": -8}, {"n_e": E - 1},
            {"w1": -0.25}, {"w0": inf}, {"w2": nan}, {"w4": 0.5}, {"w31": 0.5}, {"w0": 0.0, "w1": 0.0, "w2": 0.0, "w3": 0.0},
            {"r0": 1}, {"r1": 1}, {"r2": -1},
            {"m": mask_t.data_ptr() + 4}, {"fm": out.mask.data_ptr() + 4}, {"sp": spec_t.data_ptr() + 8}, {"sp": spec_t.data_ptr() + 4},
            {"fs": out.spec.data_ptr() + 8}, {"fs": out.spec.data_ptr() + 4}, {"ro": out.rows.data_ptr() + 8}, {"ro": out.rows.data_ptr() + 4})
    vote = ({"m": 0}, {"votes": 0}, {"votes": 5}, {"votes": -1}, {"w3": 0.0, "votes": 4}, {"guard": 1}, {"train": 1}, {"alpha": 1.0},
            {"sp": 0})                                                           # d_fused_spectrum without d_spectrum
    soft = ({"sp": 0}, {"sp": 0, "fs": 0}, {"votes": 1}, {"train": 0}, {"train": 65}, {"guard": -1}, {"guard": n // 2 - W_}, {"guard": 2 ** 31 - 1},
            {"alpha": 0.0}, {"alpha": -1.0}, {"alpha": inf}, {"alpha": nan})
    for is_soft, cases in ((False, both + vote), (True, both + soft)):
        for bad in cases:
            assert rc(soft=is_soft, **bad) == cs.CRN_ERR_ARG, (is_soft, bad)
            assert b"crn_fuse_device" in L.crn_last_error()
    # what is allowed: no spectrum under VOTE, no masks under SOFT, any single output, n_epochs = 0, the widest window
    assert rc(sp=0, fs=0) == 0 and rc(soft=True, m=0) == 0 and rc(fm=0, fs=0) == 0 and rc(fs=0, ro=0) == 0 and rc(soft=True, fm=0, ro=0) == 0
    assert rc(n_e=0) == 0 and rc(soft=True, guard=n // 2 - W_ - 1) == 0 and rc(w3=0.0, votes=3) == 0
    torch.cuda.synchronize()
    nothing = _Out(E // M, n)
    assert rc(n_e=0, fm=nothing.mask.data_ptr(), fs=nothing.spec.data_ptr(), ro=nothing.rows.data_ptr()) == 0
    torch.cuda.synchronize()
    assert all((x.cpu().numpy() == 255).all() for x in (nothing.mask, nothing.spec, nothing.rows))
    s.close()


# CFAR launch + crn_fuse_device (SOFT, M = 4, G = 1, T = 1664, all three outputs) against the CFAR launch alone, `spectrum` written in both
# arms.  Measured on an MI355X (profiles/r13_fuse.txt): arm A 422.5 us, B / A = 1.1345 and 1.1370 in two runs, the stage
# alone 53.8 us (2.6 TB/s of its own 141 MB); VOTE B / A = 1.08, alone 35.5 us; M = 32 B / A = 1.09, alone 38.7 us.  The bar is the larger
# measured ratio with the relative margin tests/test_segments_gpu.py carries (1.15 / 1.084, taken from the CA speed test, because boxes of
# the pool differ by a few per cent).
SPEED_MEASURED = 1.137
SPEED_RATIO = SPEED_MEASURED * 1.15 / 1.084


def test_cost_next_to_the_cfar_launch(built):
    """N = 4096, K = 10, rect, 64 bands, the 2.18 GB batch; the method of tests/stage_gpu.py (best_of_windows): each timed window holds
    8 launches issued back to back behind one already queued, the arms alternate, 5 windows each after a warm-up, the best counts.  Arm A
    is the CFAR launch alone, arm B the same launch followed by crn_fuse_device on the same stream: SOFT, M = 4, G = 1, T = 1664, guard 2,
    train 16, all three outputs written.  VOTE (majority of 4), M = 32 (SOFT, T = 208) and the stage alone are measured the same way
    and printed with the GB/s of the stage's own bytes: M (4 N + N / 8) read and 4 N + N / 8 + 16 written per fused row."""
    n, k = 4096, 10
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k, bands=64)
    E = 6656                                  # 6656 x 10 x 4096 x 8 B = 2.18 GB
    iq_t = sgpu.noise_batch(E, k, n)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, iq_t, E)
    torch.cuda.synchronize()
    runs = {"soft": (4, _params(fu.SOFT, 4, E // 4, fu.equal_gain(4), guard=G_, train=W_, alpha=cs.cfar_alpha(1e-3, 4 * k, W_))),
            "vote": (4, _params(fu.VOTE, 4, E // 4, fu.equal_gain(4), votes=2)),
            "soft32": (32, _params(fu.SOFT, 32, E // 32, fu.equal_gain(32), guard=G_, train=W_, alpha=cs.cfar_alpha(1e-3, 32 * k, W_)))}
    bufs = {name: _Out(E // M, n) for name, (M, _) in runs.items()}

    def arm_a():
        sgpu.cfar_launch(s, cfg, iq_t, E, outs=outs)

    def stage(name):
        _run(s, outs["mask"], outs["spectrum"], E, runs[name][1], n, out=bufs[name])

    def arm_b(name="soft"):
        arm_a()
        stage(name)
    arms = {"A": arm_a, "B soft": arm_b, "B vote": lambda: arm_b("vote"), "B soft32": lambda: arm_b("soft32"),
            "alone soft": lambda: stage("soft"), "alone vote": lambda: stage("vote"), "alone soft32": lambda: stage("soft32")}
    times = sgpu.best_of_windows(arms)
    rows = bufs["soft"].host()[2]
    s.close()
    best = {name: min(v) for name, v in times.items()}
    nbytes = E * k * n * 8
    print(f"N=4096 K=10 rect 64 bands, {E} epochs ({nbytes / 1e9:.2f} GB), spectrum written: arm A (CFAR launch alone) {best['A']:.4f} ms "
          f"({nbytes / best['A'] / 1e6:.0f} GB/s of input)")
    for name, (M, _) in runs.items():
        moved = (E // M) * (M * (4 * n + n // 8) + 4 * n + n // 8 + 16)
        print(f"  {name:7s} M={M:2d}: B / A = {best['B ' + name] / best['A']:.4f}   the stage alone {best['alone ' + name] * 1e3:.1f} us "
              f"({moved / best['alone ' + name] / 1e6:.0f} GB/s of its own {moved / 1e6:.0f} MB)")
    assert (rows["n_active"] == 4).all() and bufs["soft"].pads_untouched()
    assert rows["n_detected"].sum() < 3e-3 * (E // 4) * n                               # noise only at Pfa 1e-3: the fused rate is the asked one
    assert best["B soft"] <= SPEED_RATIO * best["A"], (best["B soft"] / best["A"], SPEED_RATIO)
