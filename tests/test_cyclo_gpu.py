"""crn_cyclo_device on the MI355X: the kernel against the twin (tests/cyclo_f64.py) fed the kernel's own fp32 spectra, under the
tolerances of tests/cyclo_cases.py (S within 8 F 2^-24, z within that times dz / dS, the cell equal wherever the twin's lead is more than
twice the bound, n_over between the twin's counts at z_min +- the bound); integer fields, zero-fills and the 0xFF behind every array
exact.  Then the refusals that need a live handle, the generator's RRC-QPSK carrier end to end, and the cost next to the chain that
feeds the stage."""
import ctypes as C

import numpy as np
import pytest

import crnsense as cs
import cyclo_cases as cc
import cyclo_f64 as cf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402

G_, W_ = 2, 16


def _upload(a):
    """A structured array's bytes on the device."""
    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(DEV)


def _frames(X):
    """[E][F][N] complex64 -> interleaved float32 on the device."""
    return torch.from_numpy(np.ascontiguousarray(X, np.complex64).view(np.float32)).to(DEV)


def _padded(E, q, profile=True):
    sizes = {"cyclo": E * q.max_segments * 32}
    if profile:
        sizes["profile"] = E * q.max_segments * q.n_a * q.frames * 4
    return sgpu.Padded(**sizes)


def _launch(s, n, x_t, E, q, heads_t, recs_t, out, first=0, count=None):
    """Epochs first .. first + count - 1 of the batch; the profile is asked for when `out` holds one."""
    count = E - first if count is None else count
    ms, per = q.max_segments, q.n_a * q.frames * 4
    prof = out.profile.data_ptr() + first * ms * per if "profile" in out.sizes else 0
    s.cyclo_device(x_t.data_ptr() + first * q.frames * n * 8, count, q, heads_t.data_ptr() + first * 16, recs_t.data_ptr() + first * ms * 32,
                   out.cyclo.data_ptr() + first * ms * 32, prof)


def _got(out, E, q):
    out.host()
    assert out.pads_untouched(), "memory behind an array was written"
    rec = out.view("cyclo", cs.CYCLO_DTYPE, (E, q.max_segments))
    prof = out.view("profile", np.float32, (E, q.max_segments, q.n_a, q.frames)) if "profile" in out.sizes else None
    return rec, prof


def _compare(rec, prof, X, heads, recs, q, what):
    """The rules of the module's docstring.  Returns (largest |S - S_twin|, segments with a tested cell, segments excused)."""
    F, ms = q.frames, q.max_segments
    want, want_prof, kept = cf.run(X, heads, recs, ms, F, q.a_lo, q.n_a, q.max_width, q.min_pairs, q.z_min, want_cells=True)
    sb = cc.s_bound(F)
    worst = float(np.abs(prof.astype(np.float64) - want_prof).max())
    assert worst <= sb, (what, worst, sb)
    for e in range(X.shape[0]):                                          # cells not tested and empty slots: exactly 0
        for sl in range(ms):
            untested = ~kept[(e, sl)][2] if (e, sl) in kept else np.ones(q.n_a, bool)
            assert not prof[e, sl][untested].any(), (what, e, sl)
    live = excused = 0
    for e in range(X.shape[0]):
        for sl in range(ms):
            g, w = rec[e, sl], want[e, sl]
            if (e, sl) not in kept or not kept[(e, sl)][2].any():
                assert not g.tobytes().strip(b"\0"), (what, e, sl, g)
                continue
            S, z, tested, pairs = kept[(e, sl)]
            live += 1
            zb = np.where(tested, cc.z_bound(F, np.maximum(pairs, 1)), 0.0)[:, None]          # per cell
            zt = np.where(tested[:, None], z.astype(np.float64), -np.inf)
            lo_n, hi_n = int((zt >= q.z_min + zb).sum()), int((zt >= q.z_min - zb).sum())
            assert lo_n <= g["n_over"] <= hi_n, (what, e, sl, g["n_over"], lo_n, hi_n)
            order = np.argsort(-zt, axis=None, kind="stable")[:2]                 # the twin's best cell and its runner-up
            top = zt.ravel()[order]
            zb2 = zb[order // F, 0]
            lead = top[0] - top[1] if top.size > 1 and np.isfinite(top[1]) else np.inf
            j = int(g["a"]) - q.a_lo
            assert 0 <= j < q.n_a and tested[j] and 0 <= g["q"] < F and g["n_pairs"] == pairs[j], (what, e, sl, g)
            if lead > 2 * zb2.max():                                               # "that bound" is the larger of the two cells'
                assert (g["a"], g["q"]) == (w["a"], w["q"]), (what, e, sl, g, w, lead)
            else:
                excused += 1
                assert zt[j, g["q"]] >= top[0] - 2 * max(zb2[0], zb[j, 0]), (what, e, sl, g, w)
            # whichever cell it chose, its figures are that cell's
            qq = int(g["q"])
            assert abs(float(g["stat"]) - float(S[j, qq])) <= sb and abs(float(g["z"]) - float(z[j, qq])) <= zb[j, 0], (what, e, sl, g)
            lo = float(S[j - 1, qq]) if j >= 1 and tested[j - 1] else 0.0
            hi = float(S[j + 1, qq]) if j + 1 < q.n_a and tested[j + 1] else 0.0
            assert abs(float(g["stat_lo"]) - lo) <= sb and abs(float(g["stat_hi"]) - hi) <= sb, (what, e, sl, g, lo, hi)
            if not (j >= 1 and tested[j - 1]):
                assert g["stat_lo"] == 0
            if not (j + 1 < q.n_a and tested[j + 1]):
                assert g["stat_hi"] == 0
    return worst, live, excused


def _case(n, F, a_lo, n_a, ms, E, max_width, min_pairs, seed, empty=0, scale=1.0):
    """(X, heads, recs, q, chain slot or None): white noise spectra and hand-made records.  With max_segments 16, epoch 0 holds widths
    1, a_lo + min_pairs - 1 (none tested), a_lo + min_pairs (one tested), a span across the wrap, width N, width max_width + 3, the
    chain with the known answer, a span with zero-power columns, and random spans up to n_stored = max_segments; epoch 1 (if any) is
    empty, its n_stored = `empty` (0, or a negative count that is clamped to 0); epoch 2 has n_stored beyond max_segments and records
    with lo and width out of range.  The spectra are multiplied by `scale`: S does not depend on it."""
    rng = np.random.default_rng(seed)
    X = cc.noise_spectra(rng, n, F, E)
    q = cs.cyclo_params(ms, F, a_lo=a_lo, n_a=n_a, max_width=max_width, min_pairs=min_pairs, z_min=cs.cyclo_zmin(1e-2, F, min_pairs))
    base = a_lo + min_pairs
    chain_slot = None
    if ms == 1:
        segs = {e: [(int(rng.integers(0, n)), base + 9)] for e in range(E)}
    else:
        cw = min(base + 24, n)
        X[0] = np.where(np.isin(np.arange(n), (200 + np.arange(cw)) % n)[None, :], cc.chain(rng, n, F, 200, cw, 3), X[0])
        X[0][:, [330, 333]] = 0
        lst = [(5, 1), (40, base - 1), (90, base), (n - 10, base + 30), (7, n), (100, max_width + 3), (200, cw), (320, base + 12)]
        chain_slot = 6
        while len(lst) < ms:
            lst.append((int(rng.integers(0, n)), int(rng.integers(base, base + 40))))
        segs = {0: lst}
        if E > 2:
            segs[2] = [(n + 17, base + 5), (-3, base + 8), (33, n + 7), (60, -2), (2 ** 31 - 1, base + 2), (-2 ** 31, 2 ** 31 - 1)]
    heads, recs = cc.records(E, ms, segs)
    if E > 2 and ms > 1:
        heads["n_stored"][2] = ms + 5           # clamped: the slots behind the six hold 0xFF records, lo = width = -1
        heads["n_stored"][1] = empty
    X = (X * np.float32(scale)).astype(np.complex64)
    assert np.isfinite(X.view(np.float32)).all()
    return X, heads, recs, q, (chain_slot, min(base + 24, n))


WORST = {}
# added to a case's seed where the twin's own best cell leads by less than the rule asks in more than 5 % of the segments: the rule may
# excuse that many and no more, so the inputs are chosen for it (the twin decides, not the device)
SEED_SHIFT = {(512, 64): 4000, (4096, 32): 1000, (4096, 64): 4000}


@pytest.mark.parametrize("F", [8, 16, 32, 64])
@pytest.mark.parametrize("n", [512, 4096])
def test_kernel_against_twin(built, n, F):
    """Per (fft_len, frames): n_a = 1 with one slot and one epoch, the spectra scaled by 1e12; n_a = 5 with 16 slots and 3 epochs, also
    cut as 1 + 2, the middle epoch with n_stored = 0; n_a = 128 ending at a = fft_len / 2 (at 4096 no span of 1024 bins reaches such a
    separation: all zero), the middle epoch with n_stored = -1; n_a = 128 from a = 1 with max_width 300, both chunks of separations at
    work, the spectra scaled by 1e-14 (P[k'] P[k] is below the smallest fp32 number there).  Every case also without the profile and
    twice over."""
    s = cs.Sensor(sgpu.cfg(n))
    live_all = excused_all = 0
    for a_lo, n_a, ms, E, max_width, min_pairs, empty, scale in ((3, 1, 1, 1, 256, 4, 0, 1e12), (2, 5, 16, 3, 64, 3, 0, 1.0),
                                                                 (n // 2 - 127, 128, 16, 3, min(n, 1024), 5, -1, 1.0), (1, 128, 16, 1, 300, 7, 0, 1e-14)):
        what = f"N={n} F={F} a_lo={a_lo} n_a={n_a} max_segments={ms} E={E}"
        X, heads, recs, q, (chain_slot, cw) = _case(n, F, a_lo, n_a, ms, E, max_width, min_pairs, n + 7 * F + n_a + SEED_SHIFT.get((n, F), 0), empty, scale)
        x_t, heads_t, recs_t = _frames(X), _upload(heads), _upload(recs)
        out = _padded(E, q)
        _launch(s, n, x_t, E, q, heads_t, recs_t, out)
        rec, prof = _got(out, E, q)
        worst, live, excused = _compare(rec, prof, X, heads, recs, q, what)
        WORST[F] = max(WORST.get(F, 0.0), worst)
        if E == 3:
            # the empty epoch, n_stored = 0 in one case and -1 in the other: every record and the whole profile are zero bytes
            assert heads["n_stored"][1] == empty and not rec[1].tobytes().strip(b"\0") and not prof[1].tobytes().strip(b"\0"), what
        live_all, excused_all = live_all + live, excused_all + excused
        # the same call again: the same bytes
        again = _padded(E, q)
        _launch(s, n, x_t, E, q, heads_t, recs_t, again)
        rec2, prof2 = _got(again, E, q)
        assert rec2.tobytes() == rec.tobytes() and prof2.tobytes() == prof.tobytes(), what
        # without the profile, and the batch cut as 1 + 2
        bare = _padded(E, q, profile=False)
        _launch(s, n, x_t, E, q, heads_t, recs_t, bare)
        assert _got(bare, E, q)[0].tobytes() == rec.tobytes(), what
        if E == 3:
            cut = _padded(E, q)
            _launch(s, n, x_t, E, q, heads_t, recs_t, cut, 0, 1)
            _launch(s, n, x_t, E, q, heads_t, recs_t, cut, 1, 2)
            rec3, prof3 = _got(cut, E, q)
            assert rec3.tobytes() == rec.tobytes() and prof3.tobytes() == prof.tobytes(), what
        if chain_slot is not None and a_lo + n_a - 1 <= n // 4:
            # the chain: S = 1 at q = 3 a mod F; the most pairs win
            g = rec[0, chain_slot]
            assert (g["a"], g["q"]) == (a_lo, (3 * a_lo) % F) and abs(float(g["stat"]) - 1.0) <= cc.s_bound(F), (what, g)
            t = np.flatnonzero(cw - (a_lo + np.arange(n_a)) >= min_pairs)
            assert t.size and np.abs(prof[0, chain_slot][t, (3 * (a_lo + t)) % F] - 1.0).max() <= cc.s_bound(F), what
    s.close()
    print(f"N={n} F={F}: largest |S - S_twin| {WORST[F]:.3e} (bound {cc.s_bound(F):.3e}); {live_all} segments with a tested cell, {excused_all} excused")
    assert live_all >= 20 and excused_all <= 0.05 * live_all, (live_all, excused_all)


def test_refusals_with_a_live_handle(built):
    """Every refusal of the header's list with a live handle; a refused call and n_epochs = 0 leave the outputs as they were."""
    n, F, E, ms = 512, 8, 2, 2
    L = cs.lib()
    s = cs.Sensor(sgpu.cfg(n))
    X = cc.noise_spectra(np.random.default_rng(1), n, F, E)
    heads, recs = cc.records(E, ms, {0: [(10, 60), (100, 50)], 1: [(300, 70), (500, 40)]})
    x_t, heads_t, recs_t = _frames(X), _upload(heads), _upload(recs)
    good = dict(max_segments=ms, frames=F, a_lo=4, n_a=8, max_width=64, min_pairs=4, z_min=2.0)
    q0 = cs.CycloParams(**good)
    out = _padded(E, q0)

    def rc(fr=x_t.data_ptr(), n_e=E, q=None, he=heads_t.data_ptr(), re=recs_t.data_ptr(), cy=out.cyclo.data_ptr(), pr=out.profile.data_ptr(), h=s._h,
           reserved=(0, 0), **kw):
        if q is None:
            q = cs.CycloParams(**{**good, **kw})
            for i, x in enumerate(reserved):
                q.reserved[i] = x
        v = lambda p: C.c_void_p(p or None)      # noqa: E731
        return L.crn_cyclo_device(h, v(fr), n_e, C.byref(q) if q != 0 else None, v(he), v(re), v(cy), v(pr), None)
    assert rc() == 0
    before = {k: v.copy() for k, v in out.host().items()}
    assert (out.view("cyclo", cs.CYCLO_DTYPE)["n_pairs"] > 0).all()
    out.cyclo[: E * ms * 32] = 255
    inf, nan = float("inf"), float("nan")
    for bad in ({"h": None}, {"fr": 0}, {"q": 0}, {"he": 0}, {"re": 0}, {"cy": 0}, {"n_e": -1},
                {"max_segments": 0}, {"max_segments": 257}, {"frames": 0}, {"frames": 4}, {"frames": 12}, {"frames": 128}, {"a_lo": 0}, {"a_lo": -1},
                {"n_a": 0}, {"n_a": 129}, {"a_lo": 250, "n_a": 8}, {"a_lo": 256, "n_a": 2}, {"max_width": 1}, {"max_width": 1025},
                {"min_pairs": 0}, {"min_pairs": 65}, {"z_min": inf}, {"z_min": -inf}, {"z_min": nan}, {"reserved": (1, 0)}, {"reserved": (0, -1)},
                {"fr": x_t.data_ptr() + 8}, {"he": heads_t.data_ptr() + 8}, {"re": recs_t.data_ptr() + 8}, {"cy": out.cyclo.data_ptr() + 8},
                {"pr": out.profile.data_ptr() + 4}, {"pr": out.profile.data_ptr() + 8}):
        assert rc(**bad) == cs.CRN_ERR_ARG, bad
        assert b"crn_cyclo_device" in L.crn_last_error(), bad
    assert rc(n_e=0) == 0
    assert (out.host()["cyclo"] == 255).all() and out.pads_untouched()
    # the ends of the ranges are accepted
    assert rc(a_lo=249, n_a=8) == 0 and rc(a_lo=256, n_a=1) == 0 and rc(max_width=2, min_pairs=2) == 0 and rc(max_width=1024, min_pairs=1024) == 0
    assert rc(z_min=-3.0) == 0 and rc(pr=0) == 0
    assert rc() == 0
    after = out.host()
    assert all(after[k].tobytes() == before[k].tobytes() for k in before) and out.pads_untouched()
    s.close()


# The generator's carrier end to end.  LAD factors of 300 keep what stands 25 dB over the excised floor: the carrier's own band without the
# leakage skirt that the rectangular window puts around a carrier 38 dB over the noise (the skirt is coherent at q = 0 and would win:
# include/crn_sense.h, Limits); max_width = the channel's width keeps to the band should a segment still be wider.
E2E = {"n": 1024, "frames": 32, "epochs": 64, "seed": 2051, "noise_power": 1e-6, "signal_rms": 0.02, "lad_factor": 300.0, "merge_gap": 3,
       "max_segments": 16, "a_lo": 8, "n_a": 64, "min_pairs": 8, "channel": 2, "idle_merge_gap": 64}
# measured on an MI355X: all 20 driven epochs of the channel passed (profiles/r20_cyclo.txt).  The bar is the measured share less the
# binomial margin: with a share of 1 of n epochs the spread sqrt(p (1 - p) / n) is 0, so the margin is one epoch, 1 / n.
E2E_SHARE = 1.0


def test_end_to_end_symbol_rate_of_the_generators_carrier(built):
    """crn_synth_fill_device_ex, RRC-QPSK at the default levels, a uniform pick among idle and the three channels, N = 1024, 32 frames per
    epoch, rect; the spectrum rows of a CFAR launch, crn_lad_device on them, crn_segments_device, crn_fft_forward_device on the same
    samples, this stage.  In the epochs that drive channel 2 (60 bins: 60 / 1.35 symbols per frame) cyclo_bins of the strongest segment
    must be within 1 / 32 bin of that rate.  The idle epochs' segments come from a CA-CFAR mask at Pfa 1e-2 closed over 64 bins, noise
    joined into wide segments: none may reach cyclo_zmin(1e-3 / cells)."""
    n, F, E, ms = E2E["n"], E2E["frames"], E2E["epochs"], E2E["max_segments"]
    cfg = sgpu.cfg(n, k=F)
    chan = {}
    for g in cfg.segs[: cfg.n_segs]:
        if g.band != 0:
            chan.setdefault(g.band, []).extend(range(g.lo, g.hi))
    nb = len(chan[E2E["channel"]])
    assert nb == 60 and cs.samples_per_epoch(cfg) == F * n
    rate = nb / (1.0 + cc.ROLLOFF)
    iq_t = sgpu.zeros((cs.samples_needed(cfg, E) * 2,), torch.float32)
    truth_t = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    sc = cs.SynthCfg()
    sc.seed, sc.noise_power, sc.signal_rms = E2E["seed"], E2E["noise_power"], E2E["signal_rms"]
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = 0, cs.PU_UNIFORM, cs.SIG_RRC_QPSK, 1
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), E, cs.samples_per_epoch(cfg), sc, truth_ptr=truth_t.data_ptr())
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-2, F, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, iq_t, E, band_bins=False)
    x_t = sgpu.zeros((E * F * n * 2,), torch.float32)
    s.fft_forward_device(iq_t.data_ptr(), E * F, n, x_t.data_ptr())
    t_cme = cs.lad_factor(1e-2, F)
    lad_mask = sgpu.zeros((E, n // 32), torch.int32)
    s.lad_device(outs["spectrum"].data_ptr(), E, cs.lad_params(1, 10, t_cme, E2E["lad_factor"], E2E["lad_factor"]), mask_ptr=lad_mask.data_ptr())
    cells = E * ms * E2E["n_a"] * F
    q = cs.cyclo_params(ms, F, a_lo=E2E["a_lo"], n_a=E2E["n_a"], max_width=nb, min_pairs=E2E["min_pairs"], pfa=1e-3 / cells)
    res = {}
    for name, mask, gap in (("driven", lad_mask, E2E["merge_gap"]), ("idle", outs["mask"], E2E["idle_merge_gap"])):
        heads_t, recs_t = sgpu.zeros((E * 16,), torch.uint8), sgpu.zeros((E * ms * 32,), torch.uint8)
        s.segments_device(mask.data_ptr(), outs["spectrum"].data_ptr(), E, heads_t.data_ptr(), recs_t.data_ptr(), merge_gap=gap, max_segments=ms)
        out = _padded(E, q, profile=False)
        _launch(s, n, x_t, E, q, heads_t, recs_t, out)
        rec, _ = _got(out, E, q)
        res[name] = (rec, np.frombuffer(heads_t.cpu().numpy().tobytes(), cs.SEGMENT_EPOCH_DTYPE),
                     np.frombuffer(recs_t.cpu().numpy().tobytes(), cs.SEGMENT_DTYPE).reshape(E, ms))
    truth = truth_t.cpu().numpy()
    s.close()

    rec, heads, recs = res["driven"]
    driven = np.flatnonzero(truth == E2E["channel"])
    ok, lines = 0, []
    for e in driven:
        ns = int(heads["n_stored"][e])
        if ns < 1:
            lines.append(f"epoch {e}: no segment")
            continue
        sl = int(np.argmax(recs["power"][e, :ns]))
        est = cs.cyclo_bins(rec[e, sl], F)
        good = abs(est - rate) <= 1.0 / F and rec[e, sl]["z"] >= q.z_min
        ok += int(good)
        lines.append(f"epoch {e}: segment lo {recs['lo'][e, sl]} width {recs['width'][e, sl]}; cell ({rec['a'][e, sl]}, {rec['q'][e, sl]}) "
                     f"z {rec['z'][e, sl]:.1f}; {est:.4f} bins, error {est - rate:+.4f}{'' if good else '  <-- outside'}")
    print("\n".join(lines))
    share = ok / max(len(driven), 1)
    margin = 1.0 / len(driven) if E2E_SHARE in (0.0, 1.0) else 2.0 * np.sqrt(E2E_SHARE * (1 - E2E_SHARE) / len(driven))
    print(f"channel {E2E['channel']}: rate {rate:.4f} bins; {ok} of {len(driven)} driven epochs within 1 / {F} bin: share {share:.3f} "
          f"(bar {E2E_SHARE - margin:.3f}); z_min {q.z_min:.2f}")
    assert len(driven) >= 8
    assert share >= E2E_SHARE - margin, (share, E2E_SHARE, margin)

    rec, heads, recs = res["idle"]
    idle = np.flatnonzero(truth == 0)
    stored = (np.arange(ms)[None, :] < heads["n_stored"][idle][:, None])
    tested = stored & (rec["n_pairs"][idle] > 0)
    zmax = float(rec["z"][idle][tested].max()) if tested.any() else float("nan")
    print(f"idle: {len(idle)} epochs, {int(stored.sum())} segments, {int(tested.sum())} with a tested cell; largest z {zmax:.2f} (z_min {q.z_min:.2f}); "
          f"n_over total {int(rec['n_over'][idle].sum())}")
    assert len(idle) >= 8 and tested.sum() >= 8
    assert not (rec["z"][idle][tested] >= q.z_min).any() and rec["n_over"][idle].sum() == 0


# fft_forward + CFAR launch + crn_segments_device + crn_cyclo_device against the first three alone, with the margin of the other stages:
# 1 + 1.5 x (the larger measured B / A - 1).  Measured on an MI355X in two separate runs (profiles/r20_cyclo.txt): arm A
# 309.8 us, B / A = 1.1590, the stage alone 36.7 us; arm A 309.5 us, B / A = 1.1694, alone 36.6 us.
SPEED_RATIO = 1.254
# ... and the launch in which every slot is a 256-bin span, the path that does the work: 1.5 x the larger of the two runs' figures,
# 9.539 and 9.535 ms
WIDE_MS = 14.3


def test_cost_next_to_the_chain_that_feeds_it(built):
    """N = 1024, 32 frames per epoch, rect, 2048 epochs (537 MB), add_tones traffic, max_segments 16, n_a = 64 from a = 8, max_width 256,
    min_pairs 16; the method of tests/stage_gpu.py (best_of_windows).  Arm A is the transform of every frame, the CFAR launch and
    crn_segments_device; arm B the same followed by this stage on the same stream.  The stage alone is measured the same way, and once
    more on records that make every slot a 256-bin span (the most a launch of this shape can cost); both are printed."""
    n, F, ms, E = 1024, 32, 16, 2048
    cfg = sgpu.cfg(n, k=F)
    iq_t = sgpu.add_tones(sgpu.noise_batch(E, F, n), E, F, n)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, F, W_), 1)
    outs = sgpu.cfar_outs(cfg, E)
    x_t = sgpu.zeros((E * F * n * 2,), torch.float32)
    heads_t, recs_t = sgpu.zeros((E * 16,), torch.uint8), sgpu.zeros((E * ms * 32,), torch.uint8)
    q = cs.cyclo_params(ms, F, a_lo=8, n_a=64, max_width=256, min_pairs=16)
    out = _padded(E, q, profile=False)
    heads_w, recs_w = cc.records(E, ms, {e: [((97 * e + 61 * sl) % n, 256) for sl in range(ms)] for e in range(E)})
    heads_wt, recs_wt = _upload(heads_w), _upload(recs_w)
    wide = _padded(E, q, profile=False)

    def arm_a():
        s.fft_forward_device(iq_t.data_ptr(), E * F, n, x_t.data_ptr())
        sgpu.cfar_launch(s, cfg, iq_t, E, outs=outs)
        s.segments_device(outs["mask"].data_ptr(), outs["spectrum"].data_ptr(), E, heads_t.data_ptr(), recs_t.data_ptr(), max_segments=ms)

    def stage():
        _launch(s, n, x_t, E, q, heads_t, recs_t, out)

    def arm_b():
        arm_a()
        stage()

    def stage_wide():
        _launch(s, n, x_t, E, q, heads_wt, recs_wt, wide)
    times = sgpu.best_of_windows({"A": arm_a, "B": arm_b, "alone": stage, "every slot 256 bins": stage_wide})
    rec, _ = _got(out, E, q)
    recw, _ = _got(wide, E, q)
    # the stage computed what the definition says: every 128th epoch once more with the profile, against the twin; two of them with the
    # 256-bin spans as well
    pick = np.arange(0, E, 128)
    X = x_t.view(E, F, n, 2)[pick].cpu().numpy().view(np.complex64)[..., 0]
    heads = np.frombuffer(heads_t.cpu().numpy().tobytes(), cs.SEGMENT_EPOCH_DTYPE)
    recs = np.frombuffer(recs_t.cpu().numpy().tobytes(), cs.SEGMENT_DTYPE).reshape(E, ms)
    for name, hh, rr, whole, count in (("traffic", heads[pick], recs[pick], rec[pick], len(pick)), ("256-bin spans", heads_w[pick], recs_w[pick], recw[pick], 2)):
        small = _padded(count, q)
        _launch(s, n, _frames(X[:count]), count, q, _upload(hh[:count]), _upload(rr[:count]), small)
        r, pr = _got(small, count, q)
        assert r.tobytes() == whole[:count].tobytes(), name
        _compare(r, pr, X[:count], hh[:count], rr[:count], q, name)
    s.close()
    best = {name: min(v) for name, v in times.items()}
    stored = int(np.clip(heads["n_stored"], 0, ms).sum())
    print(f"N=1024 F=32 rect, {E} epochs ({E * F * n * 8 / 1e6:.0f} MB): arm A (transform + CFAR launch + crn_segments_device) {best['A']:.4f} ms; "
          f"B / A = {best['B'] / best['A']:.4f}; crn_cyclo_device alone {best['alone'] * 1e3:.1f} us; {stored} stored segments, "
          f"{int((rec['n_pairs'] > 0).sum())} with a tested cell; every slot a 256-bin span ({E * ms} segments): {best['every slot 256 bins']:.3f} ms")
    assert (recw["n_pairs"] > 0).all()
    assert best["B"] <= SPEED_RATIO * best["A"], (best["B"] / best["A"], SPEED_RATIO)
    assert best["every slot 256 bins"] <= WIDE_MS, (best["every slot 256 bins"], WIDE_MS)
