"""crn_tcfar_device on the MI355X: the kernel against the twin (tests/tcfar_f64.py) fed the kernel's own inputs, byte for byte and on every
bin (the rule is an fp32 product and an fp32 compare: there is no rounding freedom).  Every output array, the history and d_seen have 256
bytes of 0xFF behind them that must stay, NULL outputs must stay unwritten, and a history starts out as 0xFF bytes (NaN) so that a slot
read before it was written shows.  Then the carry across cuts, the optional arguments, the refusals that need a live handle, band-noise
traffic end to end through a receiver with a shaped floor, a spur and a DC spike next to crn_lad_device, and the cost next to the CFAR
launch alone."""
import ctypes as C

import numpy as np
import pytest

import crnsense as cs
import tcfar_cases as tc
import tcfar_f64 as tf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402

G_, W_ = 2, 16
SIZES = (512, 1024, 2048, 4096)
WINDOWS = ((2, 0), (4, 2), (64, 1), (128, 16))      # (cells, guard_epochs)


def _out(E, n):
    return sgpu.Padded(mask=E * n // 8, rows=E * 16)


def _state(S, n, cells, guard):
    return sgpu.Padded(hist=S * (cells + guard) * n * 4, seen=S * 8)


def _launch(s, spec_t, E, q, out, st, or_ptr=0, mask=True, rows=True):
    s.tcfar_device(spec_t.data_ptr(), E, q, st.hist.data_ptr(), st.seen.data_ptr(), mask_ptr=out.mask.data_ptr() if mask else 0,
                   rows_ptr=out.rows.data_ptr() if rows else 0, or_mask_ptr=or_ptr)


def _views(out, st, E, n, S, H):
    out.host(), st.host()
    assert out.pads_untouched() and st.pads_untouched(), "memory behind an array was written"
    return (out.view("mask", np.uint32, (E, n // 32)), out.view("rows", cs.TCFAR_ROW_DTYPE), st.view("hist", np.uint32, (S, H, n)), st.view("seen", np.int64))


def _nan_state(S, n, cells, guard):
    """The twin's carry as the device's starts out: 0xFF bytes."""
    hist = np.frombuffer(b"\xff" * (S * (cells + guard) * n * 4), np.float32).reshape(S, cells + guard, n).copy()
    return hist, np.full(S, -1, np.int64)


def _same(got, want_mask, want_rows, want_hist, want_seen, what):
    mask, rows, hist, seen = got
    assert mask.tobytes() == tf.pack_mask(want_mask).tobytes(), (what, "mask, rows", np.flatnonzero((mask != tf.pack_mask(want_mask)).any(axis=1))[:8])
    for f in ("n_detected", "n_new", "n_cells", "reserved"):
        assert (rows[f] == want_rows[f]).all(), (what, f, np.flatnonzero(rows[f] != want_rows[f])[:8])
    assert (seen == want_seen).all(), (what, "d_seen", seen, want_seen)
    assert hist.tobytes() == want_hist.view(np.uint32).tobytes(), (what, "d_hist, (stream, slot)", np.argwhere((hist != want_hist.view(np.uint32)).any(axis=2))[:8])


def _check(s, P, T, cells, guard, rank, alpha, what, or_mask=None):
    """One call with first = 1 over a NaN-filled history, every output against the twin; a list of ranks is a call each."""
    E, n = P.shape
    S = E // T
    ranks = [rank] if isinstance(rank, int) else list(rank)
    spec_t = sgpu.upload_rows(P)
    or_t = None if or_mask is None else sgpu.upload_mask(or_mask)
    hist, seen = _nan_state(S, n, cells, guard)
    want = tf.run_ranks(P, T, cells, guard, ranks, alpha, hist, seen, True, or_mask)
    for r in ranks:
        out, st = _out(E, n), _state(S, n, cells, guard)
        _launch(s, spec_t, E, cs.tcfar_params(T, cells, r, alpha, guard, first=True), out, st, or_ptr=0 if or_t is None else or_t.data_ptr())
        got = _views(out, st, E, n, S, cells + guard)
        _same(got, want[r][0], want[r][1], hist, seen, (what, "rank", r))
    return got


@pytest.mark.parametrize("cells,guard", WINDOWS)
@pytest.mark.parametrize("n", SIZES)
def test_shapes_against_twin(built, n, cells, guard):
    """T in {1, H - 1, H, H + 1, 2 H + 3}, one stream and three, rank in {1, cells / 4, cells}; Gamma(10) rows at alpha = 1.1 and rows
    quantised to quarters at alpha = 2, where fl32(alpha c) == P is common and must not count.  T = H + 1 is the first size with a
    decision, 2 H + 3 has decisions whose cells all lie in the batch, and at 128 + 16 it takes more than one run of a stream."""
    H = cells + guard
    ranks = sorted({1, max(1, cells // 4), cells})
    s = cs.Sensor(sgpu.cfg(n))
    detected = 0
    for T, S, rks, quantised in ((1, 3, ranks[:1], False), (H - 1, 1, ranks[1:2], False), (H, 1, ranks[-1:], True), (H + 1, 3, ranks, False),
                                 (H + 1, 3, ranks[1:2], True), (2 * H + 3, 1, ranks[1:2], False), (2 * H + 3, 1, ranks, True)):
        P = tc.gamma_rows(n + 7 * T + S, S * T, n, quantised)
        got = _check(s, P, T, cells, guard, rks, 2.0 if quantised else 1.1, f"N={n} D={cells} g={guard} T={T} S={S} quantised={quantised}")
        detected += int(got[1]["n_detected"].sum())
        assert (got[1]["n_cells"].reshape(S, T)[:, :H] == 0).all()
    s.close()
    assert detected > 0


@pytest.mark.parametrize("cells,guard", [(4, 2), (64, 1), (128, 16)])
@pytest.mark.parametrize("n", [512, 4096])
def test_carry_across_cuts(built, n, cells, guard):
    """Two streams of 2 H + 3 epochs in one call, and cut as [1, 2, H - 1, the rest] (first = 1, then 0): the same masks, headers, d_seen
    and history, which is the twin's.  The first call of each starts over a history and a d_seen of 0xFF bytes."""
    H, S = cells + guard, 2
    T = 2 * H + 3
    rank, alpha = max(1, cells // 4), 2.0
    P = tc.gamma_rows(n + cells, S * T, n, quantised=True).reshape(S, T, n)
    s = cs.Sensor(sgpu.cfg(n))
    whole = _check(s, P.reshape(S * T, n), T, cells, guard, rank, alpha, "whole")
    edges = [0, 1, 3, H + 2, T]
    st = _state(S, n, cells, guard)
    masks, rows = np.zeros((S, T, n // 32), np.uint32), np.zeros((S, T), np.dtype(cs.TCFAR_ROW_DTYPE))
    for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
        E = S * (b - a)
        out = _out(E, n)
        _launch(s, sgpu.upload_rows(P[:, a:b].reshape(E, n)), E, cs.tcfar_params(b - a, cells, rank, alpha, guard, first=i == 0), out, st)
        got = _views(out, st, E, n, S, H)
        masks[:, a:b], rows[:, a:b] = got[0].reshape(S, b - a, -1), got[1].reshape(S, b - a)
        assert (got[3] == b).all()
    s.close()
    assert masks.tobytes() == whole[0].tobytes() and rows.tobytes() == whole[1].tobytes()
    assert got[2].tobytes() == whole[2].tobytes() and (got[3] == whole[3]).all()
    assert rows["n_detected"].sum() > 0


@pytest.mark.parametrize("n", [512, 4096])
def test_optional_arguments(built, n):
    """d_or_mask NULL, separate, and the same address as d_bin_mask; the mask NULL with the headers given and the reverse; calls that only
    feed the history, after which a call with first = 0 gives what the whole stream gives; n_epochs = 0 touches nothing."""
    cells, guard, rank, alpha, S = 4, 1, 1, 1.3, 2
    H = cells + guard
    T = H + 6
    P = tc.gamma_rows(n + 1, S * T, n)
    spec_t = sgpu.upload_rows(P)
    E = S * T
    rng = np.random.default_rng(n)
    om = rng.random((E, n)) < 0.01
    om[:, [0, 31, 32, 63, 64, n - 1]] = True
    s = cs.Sensor(sgpu.cfg(n))
    q = cs.tcfar_params(T, cells, rank, alpha, guard, first=True)
    plain = _check(s, P, T, cells, guard, rank, alpha, "no d_or_mask")
    with_or = _check(s, P, T, cells, guard, rank, alpha, "d_or_mask given", or_mask=om)
    assert with_or[0].tobytes() == (plain[0] | tf.pack_mask(om)).tobytes() and (with_or[1]["n_new"] <= plain[1]["n_new"]).all()
    assert plain[1]["n_new"].sum() > 0 and (with_or[1]["n_detected"][: H] == om[:H].sum(axis=1)).all()      # the warm-up passes or_mask on
    # aliased: the mask array holds the mask to OR in and receives the result
    out, st = _out(E, n), _state(S, n, cells, guard)
    out.mask[: E * n // 8] = torch.from_numpy(tf.pack_mask(om).view(np.uint8).reshape(-1).copy()).to(DEV)
    _launch(s, spec_t, E, q, out, st, or_ptr=out.mask.data_ptr())
    aliased = _views(out, st, E, n, S, H)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(aliased, with_or))
    # one output NULL: the other and the carry do not change, and the NULL one stays 0xFF
    for kw, kept, i in (({"mask": False}, "mask", 1), ({"rows": False}, "rows", 0)):
        out, st = _out(E, n), _state(S, n, cells, guard)
        _launch(s, spec_t, E, q, out, st, **kw)
        got = _views(out, st, E, n, S, H)
        assert (out.raw[kept] == 255).all(), (kw, "a NULL output was written")
        assert got[i].tobytes() == plain[i].tobytes() and got[2].tobytes() == plain[2].tobytes() and (got[3] == plain[3]).all(), kw
    # history only: the first H + 2 epochs without an output, the rest with first = 0
    cut = H + 2
    P3 = P.reshape(S, T, n)
    out, st = _out(E, n), _state(S, n, cells, guard)
    _launch(s, sgpu.upload_rows(P3[:, :cut].reshape(S * cut, n)), S * cut, cs.tcfar_params(cut, cells, rank, alpha, guard, first=True), out, st, mask=False, rows=False)
    fed = _views(out, st, E, n, S, H)
    assert (out.raw["mask"] == 255).all() and (out.raw["rows"] == 255).all() and (fed[3] == cut).all()
    rest = T - cut
    out = _out(S * rest, n)
    _launch(s, sgpu.upload_rows(P3[:, cut:].reshape(S * rest, n)), S * rest, cs.tcfar_params(rest, cells, rank, alpha, guard), out, st)
    got = _views(out, st, S * rest, n, S, H)
    assert got[0].tobytes() == plain[0].reshape(S, T, -1)[:, cut:].tobytes() and got[1].tobytes() == plain[1].reshape(S, T)[:, cut:].tobytes()
    assert got[2].tobytes() == plain[2].tobytes() and (got[3] == T).all()
    # n_epochs = 0, with first != 0 too: nothing is touched
    out = _out(E, n)
    before = st.host()["hist"].copy(), st.raw["seen"].copy()
    _launch(s, spec_t, 0, q, out, st)
    o, t = out.host(), st.host()
    assert (o["mask"] == 255).all() and (o["rows"] == 255).all() and (t["hist"] == before[0]).all() and (t["seen"] == before[1]).all()
    s.close()


def test_refusals_with_a_live_handle(built):
    """Every refusal of the header's list with a live handle; a refused call and n_epochs = 0 leave the state as it was."""
    n, T, S = 512, 6, 2
    E = S * T
    L = cs.lib()
    s = cs.Sensor(sgpu.cfg(n))
    spec_t = sgpu.upload_rows(tc.gamma_rows(1, E, n))
    out, st = _out(E, n), _state(S, n, 4, 1)
    or_t = torch.zeros((E * n // 32,), dtype=torch.int32, device=DEV)
    inf, nan = float("inf"), float("nan")

    def rc(sp=spec_t.data_ptr(), n_e=E, q=None, orp=or_t.data_ptr(), m=out.mask.data_ptr(), r=out.rows.data_ptr(), hi=st.hist.data_ptr(),
           se=st.seen.data_ptr(), reserved=(0, 0), **kw):
        if q is None:
            q = cs.tcfar_params(**{"epochs_per_stream": T, "cells": 4, "rank": 2, "alpha": 1.5, "guard_epochs": 1, "first": True, **kw})
            for i, x in enumerate(reserved):
                q.reserved[i] = x
        v = lambda p: C.c_void_p(p or None)      # noqa: E731
        return L.crn_tcfar_device(s._h, v(sp), n_e, C.byref(q) if q != 0 else None, v(orp), v(m), v(r), v(hi), v(se), None)
    assert rc() == 0
    torch.cuda.synchronize()
    before = {k: v.copy() for k, v in {**out.host(), **st.host()}.items()}
    for bad in ({"sp": 0}, {"q": 0}, {"hi": 0}, {"se": 0}, {"n_e": -1}, {"n_e": E + 1}, {"epochs_per_stream": 0}, {"epochs_per_stream": -1},
                {"epochs_per_stream": 5},
                {"cells": 0}, {"cells": 3}, {"cells": 130}, {"cells": -4}, {"guard_epochs": -1}, {"guard_epochs": 17},
                {"rank": 0}, {"rank": 5}, {"rank": -1}, {"alpha": 0.0}, {"alpha": -1.0}, {"alpha": inf}, {"alpha": nan},
                {"reserved": (1, 0)}, {"reserved": (0, 1)},
                {"sp": spec_t.data_ptr() + 4}, {"sp": spec_t.data_ptr() + 8}, {"r": out.rows.data_ptr() + 8}, {"hi": st.hist.data_ptr() + 8},
                {"m": out.mask.data_ptr() + 4}, {"orp": or_t.data_ptr() + 4}, {"se": st.seen.data_ptr() + 4}):
        assert rc(**bad) == cs.CRN_ERR_ARG, bad
        assert b"crn_tcfar_device" in L.crn_last_error(), bad
    assert rc(n_e=0) == 0 and rc(n_e=0, first=False) == 0
    torch.cuda.synchronize()
    after = {**out.host(), **st.host()}
    assert all((after[k] == before[k]).all() for k in before) and out.pads_untouched() and st.pads_untouched()
    assert rc(orp=0) == 0 and rc(m=0, r=0) == 0 and rc(m=0) == 0 and rc(r=0) == 0 and rc(epochs_per_stream=E) == 0
    torch.cuda.synchronize()
    s.close()


# the receiver of tests/test_tcfar_host.py's simulation over the library's own traffic: the channels are the handle's bands 1..3
E2E = {"n": 512, "k": 10, "eps": 64 + 1 + 448, "seed": 2032, "noise_power": 1e-6}
# band noise of total power signal_rms^2 over w bins against noise_power over N bins: +10 dB per bin on the widest channel
E2E["signal_rms"] = float(np.sqrt(10.0 * 33 / 512 * E2E["noise_power"]))


def test_end_to_end_shaped_floor_spur_and_dc_spike(built):
    """crn_synth_fill_device_ex, a uniform pick among idle and the three channels per epoch, band noise 10 dB over the noise in every bin
    of the driven channel, one stream of 64 + 1 + 448 epochs, N = 512, K = 10, rect, through the CFAR launch.  The `spectrum` rows are then
    multiplied on the device by the receiver's gain (tests/tcfar_cases.py: 1 + 0.75 cos(2 pi k / N), x100 at bin 100, x30 at bin 0) and go
    through crn_lad_device (one block, 1e-2 / 1e-4) and through this stage (D = 64, rank 16, guard 1, alpha for 1e-3).  The host test's
    bars: the driven channel's bins set >= 0.99, the bins outside every channel within a factor 1.5 of 1e-3, the spur bin in under 1 % of
    the epochs; LAD sets over 0.2 of the idle bins of the same rows.  Every row equals the twin."""
    n, k, T = E2E["n"], E2E["k"], E2E["eps"]
    H = tc.CELLS + tc.GUARD
    cfg = sgpu.cfg(n, k=k)
    iq_t = torch.zeros((cs.samples_needed(cfg, T) * 2,), dtype=torch.float32, device=DEV)
    truth_t = torch.full((T,), -1, dtype=torch.int32, device=DEV)
    sc = cs.SynthCfg()
    sc.seed, sc.noise_power, sc.signal_rms = E2E["seed"], E2E["noise_power"], E2E["signal_rms"]
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = 0, cs.PU_UNIFORM, cs.SIG_BAND_NOISE, 1
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), T, cs.samples_per_epoch(cfg), sc, truth_ptr=truth_t.data_ptr())
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = sgpu.cfar_launch(s, cfg, iq_t, T, band_bins=False)
    outs["spectrum"] *= torch.from_numpy(tc.gain(n).astype(np.float32)).to(DEV)[None, :]
    t_cme = cs.lad_factor(1e-2, k)
    lad_mask = torch.zeros((T, n // 32), dtype=torch.int32, device=DEV)
    s.lad_device(outs["spectrum"].data_ptr(), T, cs.lad_params(1, 10, t_cme, cs.lad_factor(1e-2, k, t_cme), cs.lad_factor(1e-4, k, t_cme)),
                 mask_ptr=lad_mask.data_ptr())
    alpha = cs.tcfar_alpha(tc.PFA, k, tc.CELLS, tc.RANK)
    out, st = _out(T, n), _state(1, n, tc.CELLS, tc.GUARD)
    _launch(s, outs["spectrum"], T, cs.tcfar_params(T, tc.CELLS, tc.RANK, alpha, tc.GUARD, first=True), out, st)
    got = _views(out, st, T, n, 1, H)
    P = outs["spectrum"].cpu().numpy()
    truth = truth_t.cpu().numpy()
    lad = tf.unpack_mask(lad_mask.cpu().numpy().view(np.uint32), n)
    s.close()
    hist, seen = _nan_state(1, n, tc.CELLS, tc.GUARD)
    want = tf.run(P, T, tc.CELLS, tc.GUARD, tc.RANK, alpha, hist, seen, True)
    _same(got, want[0], want[1], hist, seen, "end to end")
    mask = tf.unpack_mask(got[0], n)
    assert set(np.unique(truth)) == {0, 1, 2, 3}
    chan = np.zeros((4, n), bool)
    for g in cfg.segs[: cfg.n_segs]:                              # band 1 has two segments, one on either side of the wrap; band 0 is never driven
        if g.band != 0:
            chan[g.band, g.lo: g.hi] = True
    assert sorted(chan.sum(axis=1)) == [0, 30, 31, 33]
    driven = chan[truth][H:]
    idle = ~chan.any(axis=0)
    idle[[tc.SPUR_BIN, tc.DC_BIN]] = False
    share, lad_share = mask[H:][driven].mean(), lad[H:][driven].mean()
    false, lad_false = mask[H:][:, idle].mean(), lad[H:][:, idle].mean()
    spur, lad_spur = mask[H:, tc.SPUR_BIN].mean(), lad[H:, tc.SPUR_BIN].mean()
    print(f"end to end, {T - H} epochs behind the warm-up, band noise +10 dB: driven channel's bins set: LAD {lad_share:.4f} / along time {share:.4f} "
          f"(bar {tc.SHARE_10DB}); bins outside every channel set: LAD {lad_false:.4f} (bar > {tc.LAD_FALSE_BAR}) / along time {false:.3e} "
          f"(bar {tc.FA_LO:.2e} .. {tc.FA_HI:.2e}, {mask[H:][:, idle].size} decisions); spur bin set: LAD {lad_spur:.3f} / along time {spur:.4f} "
          f"(bar < {tc.SPUR_BAR}); warm-up rows set: {int(mask[:H].sum())}")
    assert not mask[:H].any()
    assert share >= tc.SHARE_10DB
    assert tc.FA_LO <= false <= tc.FA_HI
    assert spur < tc.SPUR_BAR
    assert lad_false > tc.LAD_FALSE_BAR


# CFAR launch + crn_tcfar_device against the CFAR launch alone, `spectrum` written in both arms, with the margin of tests/test_lad_gpu.py:
# 1 + 1.5 x (the larger measured B / A - 1).  Measured on an MI355X in two separate runs (profiles/r17_tcfar.txt): one stream,
# arm A 427.5 us, B / A = 1.3991, the stage alone 167.6 us; arm A 427.4 us, B / A = 1.4183, alone 171.4 us.  64 streams: arm A 396.5 us,
# B / A = 1.4999, alone 189.2 us; arm A 430.3 us, B / A = 1.4582, alone 190.5 us.
SPEED_RATIO = {1: 1.627, 64: 1.750}


@pytest.mark.parametrize("S", [1, 64])
def test_cost_next_to_the_cfar_launch(built, S):
    """N = 4096, K = 10, rect, 64 bands, 6656 epochs as one stream and as 64 streams of 104; the method of tests/stage_gpu.py (best_of_windows):
    each timed window holds 8 launches issued back to back behind one already queued, the arms alternate, 5 windows each after a warm-up,
    the best counts.  Arm A is the CFAR launch alone, arm B the same launch followed by crn_tcfar_device on the same stream with all
    outputs, d_or_mask the CFAR mask, D = 64, guard 1, rank 16, first = 0 (the rows before the batch come from the history, which every
    call leaves as the batch's last 65 rows).  The stage alone is measured the same way and printed."""
    n, k = 4096, 10
    cells, guard, rank = tc.CELLS, tc.GUARD, tc.RANK
    H = cells + guard
    cfg = sgpu.cfg(n, k=k, bands=64)
    E = 6656                                  # 6656 x 10 x 4096 x 8 B = 2.18 GB
    T = E // S
    # the traffic of every cost test here: tones over unit noise in two epochs of three
    iq_t = sgpu.add_tones(sgpu.noise_batch(E, k, n), E, k, n)
    s = cs.Sensor(cfg)
    s.set_cfar(G_, W_, cs.cfar_alpha(1e-3, k, W_), 1)
    outs = sgpu.cfar_outs(cfg, E)
    alpha = cs.tcfar_alpha(1e-3, k, cells, rank)
    out, st = _out(E, n), _state(S, n, cells, guard)

    def arm_a():
        sgpu.cfar_launch(s, cfg, iq_t, E, outs=outs)

    def stage(first=False):
        _launch(s, outs["spectrum"], E, cs.tcfar_params(T, cells, rank, alpha, guard, first=first), out, st, or_ptr=outs["mask"].data_ptr())

    def arm_b():
        arm_a()
        stage()
    arms = {"A": arm_a, "B": arm_b, "alone": stage}
    arm_a()
    stage(first=True)
    times = sgpu.best_of_windows(arms)
    got = _views(out, st, E, n, S, H)
    # the stage computed what the definition says: every 16th epoch of every stream, restated on the kernel's own inputs.  Every call saw
    # the same batch, so the rows before it are the batch's own last H
    P = outs["spectrum"].cpu().numpy().reshape(S, T, n)
    cfar = outs["mask"].cpu().numpy().view(np.uint32).reshape(S, T, n // 32)
    s.close()
    a32 = np.float32(alpha)
    pick = np.arange(0, T, 16)
    for si in range(S):
        ring = np.concatenate([P[si, T - H:], P[si]])            # row t of the batch is ring[H + t]
        det = np.stack([((a32 * ring[t + H - guard - cells: t + H - guard]) < P[si, t][None, :]).sum(axis=0) >= rank for t in pick])
        want = tf.pack_mask(det) | cfar[si, pick]
        rows = got[1].reshape(S, T)[si, pick]
        assert got[0].reshape(S, T, -1)[si, pick].tobytes() == want.tobytes(), ("cost batch, stream", si)
        assert (rows["n_detected"] == tf.unpack_mask(want, n).sum(axis=1)).all() and (rows["n_cells"] == cells).all()
        assert (rows["n_new"] == (det & ~tf.unpack_mask(cfar[si, pick], n)).sum(axis=1)).all()
        assert got[2][si].tobytes() == P[si, T - H + ((np.arange(H) - (got[3][si] - H)) % H)].view(np.uint32).tobytes()
    best = {name: min(v) for name, v in times.items()}
    nbytes = E * k * n * 8
    print(f"N=4096 K=10 rect 64 bands, {E} epochs ({nbytes / 1e9:.2f} GB) as {S} stream(s), spectrum written: arm A (CFAR launch alone) {best['A']:.4f} ms "
          f"({nbytes / best['A'] / 1e6:.0f} GB/s of input); B / A = {best['B'] / best['A']:.4f}; crn_tcfar_device alone {best['alone'] * 1e3:.1f} us; "
          f"bits set {int(got[1]['n_detected'].sum())}, new {int(got[1]['n_new'].sum())}")
    assert got[1]["n_new"].sum() > 0
    assert best["B"] <= SPEED_RATIO[S] * best["A"], (best["B"] / best["A"], SPEED_RATIO[S])
