"""crn_hops_device on the MI355X: the records against the twin (tests/hops_twin.py) byte for byte over stream lengths around the 64-epoch
chunks, three lag sets, 1, 3 and 63 channels and six kinds of busy words; cut independence; what a carried record may hold; the same
call twice; memory behind every array still the 0xFF fill; every refusal; the Markov chain and the sweep of the generator end to end
through the CFAR launch and crn_channels_device; and the cost next to those two."""
import ctypes as C

import numpy as np
import pytest

import crnsense as cs
import hops_cases as hc
import hops_twin as ht

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402


class _Out(sgpu.Padded):
    """The records and the workspace of a batch on the device, each exactly the size the library asks for, with 0xFF bytes behind it."""

    def __init__(self, E, n_streams, nch, lags, eps):
        self.S, self.L = n_streams, len(lags)
        self.rec_bytes = cs.hops_bytes(n_streams, nch, lags)
        self.ws_bytes = cs.hops_workspace_bytes(E, nch, eps, lags)
        super().__init__(records=self.rec_bytes, ws=self.ws_bytes)

    def host(self):
        super().host()
        return self.raw["records"].tobytes()


def _busy(w):
    return torch.from_numpy(np.ascontiguousarray(w, np.uint64).view(np.int64)).to(DEV)


def _run(s, busy_t, E, nch, lags, eps, first=True, out=None):
    out = _Out(E, E // eps, nch, lags, eps) if out is None else out
    s.hops_device(busy_t.data_ptr(), E, cs.hop_params(nch, eps, lags, first), out.records.data_ptr(), out.rec_bytes, out.ws.data_ptr(), out.ws_bytes)
    return out


def _diff(got, want, n_lags, what):
    """Where two batches of records differ, for the message of a failed comparison."""
    g, w = np.frombuffer(got, ht.dtype(n_lags)), np.frombuffer(want, ht.dtype(n_lags))
    return what, [(f, np.argwhere(g[f] != w[f])[:4].tolist()) for f in ("n_epochs", "n_channels", "n_lags", "lag", "reserved", "hist", "hop")
                  if (g[f] != w[f]).any()] + [(f, np.argwhere(g["lags"][f] != w["lags"][f])[:4].tolist()) for f in ("from", "to", "pair")
                                              if (g["lags"][f] != w["lags"][f]).any()]


@pytest.fixture(scope="module")
def sensor(built):
    s = cs.Sensor(sgpu.cfg(512, cs.WINDOW_RECT, 10))
    yield s
    s.close()


@pytest.mark.parametrize("lags", hc.LAG_SETS, ids=lambda v: f"lags{len(v)}")
@pytest.mark.parametrize("eps", hc.EPS)
def test_records_against_twin(sensor, eps, lags):
    """Every stream length x lag set; inside, 1, 3 and 63 channels, 1 and 3 streams, and the six kinds of words."""
    rng = np.random.default_rng(eps * 10 + len(lags))
    for nch in hc.CHANNELS:
        for n_streams in (1, 3):
            for kind in hc.WORD_KINDS:
                E = eps * n_streams
                w = hc.words(kind, E, nch, rng)
                out = _run(sensor, _busy(w), E, nch, lags, eps)
                got = out.host()
                want = ht.update(None, w, nch, lags, eps, True).tobytes()
                what = f"eps {eps} lags {lags} C {nch} streams {n_streams} {kind}"
                assert got == want, _diff(got, want, len(lags), what)
                assert out.pads_untouched(), (what, "memory behind the records or the workspace was written")


@pytest.mark.parametrize("nch", [3, 63])
def test_cut_independence(sensor, nch):
    """Three streams of 193 epochs in one call, and cut as 1, 2, 61, 1, 64, 64 (first = 1, then 0): the same bytes, and the twin's."""
    rng = np.random.default_rng(nch)
    lags, T, S = hc.LAG_SETS[2], 193, 3
    for kind in ("chain", "d0.5", "high"):
        w = hc.words(kind, S * T, nch, rng).reshape(S, T)
        whole = _run(sensor, _busy(w), S * T, nch, lags, T).host()
        assert whole == ht.update(None, w.reshape(-1), nch, lags, T, True).tobytes()
        out, at = None, 0
        for n in (1, 2, 61, 1, 64, 64):
            part = _Out(S * n, S, nch, lags, n)
            if out is not None:
                part.records = out.records
            out = _run(sensor, _busy(w[:, at: at + n]), S * n, nch, lags, n, first=(at == 0), out=part)
            got = out.host()
            assert out.pads_untouched()
            at += n
        assert got == whole, _diff(got, whole, len(lags), f"cut, C {nch} {kind}")


def _carry(sensor, old, w, nch, lags, eps, S):
    """One call with first = 0 on the carried bytes `old`: (the records after it, the twin's)."""
    out = _Out(S * eps, S, nch, lags, eps)
    out.records[: len(old)] = torch.from_numpy(np.frombuffer(old, np.uint8).copy()).to(DEV)
    got = _run(sensor, _busy(w), S * eps, nch, lags, eps, first=False, out=out).host()
    assert out.pads_untouched()
    return got, ht.update(old, w, nch, lags, eps, False).tobytes()


def test_carries(sensor):
    """What first = 0 may find: 0xFF bytes, a head of another call's kind, a record with no epochs (all taken as empty); and a valid head
    over counts of 2^31 - 2, negative counts and hist bits outside the mask.  After that carry the saturated counts stay at 2^31 - 1."""
    rng = np.random.default_rng(5)
    nch, lags, eps, S = 3, (1, 2, 64), 70, 2
    dt = ht.dtype(len(lags))
    w = hc.words("d0.5", S * eps, nch, rng)
    fresh = ht.update(None, w, nch, lags, eps, True).tobytes()
    got, want = _carry(sensor, b"\xff" * (S * dt.itemsize), w, nch, lags, eps, S)
    assert got == want == fresh
    for field, idx, v in (("n_channels", (), 4), ("n_lags", (), 2), ("lag", (2,), 63), ("lag", (5,), 1), ("n_epochs", (), 0), ("n_epochs", (), -3)):
        old = ht.update(None, w, nch, lags, eps, True)
        old[field][(slice(None),) + idx] = v
        got, want = _carry(sensor, old.tobytes(), w, nch, lags, eps, S)
        assert got == want == fresh, (field, v)
    # a head that is valid, over whatever bytes
    old = ht.update(None, w, nch, lags, eps, True)
    old["hop"][:] = ht.SAT - 1
    old["hop"][:, ::2, 1::2] = rng.integers(-2 ** 31, 0, old["hop"][:, ::2, 1::2].shape)
    old["lags"]["pair"][:, 0] = ht.SAT - 2
    old["lags"]["pair"][:, 1] = -1
    old["lags"]["from"][:, 1:] = ht.SAT - 1
    old["lags"]["to"][:, 1:] = rng.integers(-2 ** 31, 2 ** 31, old["lags"]["to"][:, 1:].shape)
    old["hist"] = rng.integers(0, 2 ** 64, old["hist"].shape, dtype=np.uint64)
    old["n_epochs"] = [7, 2 ** 40]                                # hist: 7 bits count in stream 0, all 64 in stream 1
    got, want = _carry(sensor, old.tobytes(), w, nch, lags, eps, S)
    assert got == want, _diff(got, want, len(lags), "spoilt carry")
    r = np.frombuffer(got, dt)
    assert (r["hop"] >= 0).all() and (r["lags"]["pair"] >= 0).all() and r["hop"].max() == ht.SAT and not r["hist"][:, nch:63].any()
    assert r["n_epochs"].tolist() == [7 + eps, 2 ** 40 + eps]
    again, want = _carry(sensor, got, w, nch, lags, eps, S)
    assert again == want
    r2 = np.frombuffer(again, dt)
    assert (r2["hop"][r["hop"] == ht.SAT] == ht.SAT).all() and (r2["lags"]["from"][r["lags"]["from"] == ht.SAT] == ht.SAT).all()
    assert (r2["hop"] >= r["hop"]).all() and (r2["lags"]["pair"] >= r["lags"]["pair"]).all()


def test_the_same_call_twice_and_nothing_to_do(sensor):
    rng = np.random.default_rng(6)
    nch, lags, eps, S = 63, hc.LAG_SETS[2], 193, 3
    w = hc.words("d0.5", S * eps, nch, rng)
    busy_t = _busy(w)
    a, b = _run(sensor, busy_t, S * eps, nch, lags, eps).host(), _run(sensor, busy_t, S * eps, nch, lags, eps).host()
    assert a == b
    w2 = hc.words("d0.05", S * eps, nch, rng)
    assert _carry(sensor, a, w2, nch, lags, eps, S)[0] == _carry(sensor, a, w2, nch, lags, eps, S)[0]
    # n_epochs = 0 touches nothing, with first != 0 too
    for first in (True, False):
        nothing = _Out(0, S, nch, lags, eps)
        sensor.hops_device(busy_t.data_ptr(), 0, cs.hop_params(nch, eps, lags, first), nothing.records.data_ptr(), nothing.rec_bytes,
                           nothing.ws.data_ptr(), nothing.ws_bytes)
        torch.cuda.synchronize()
        assert (nothing.records.cpu().numpy() == 255).all() and (nothing.ws.cpu().numpy() == 255).all()


def test_refusals_and_any_handle(built):
    """Every refusal, on a REF_MAG handle with CFAR off, which serves the stage like any other."""
    L = cs.lib()
    s = cs.Sensor(cs.cfg_reference())
    assert s.get_cfar() is None
    rng = np.random.default_rng(0)
    nch, lags, eps, E = 5, (1, 2), 4, 8
    w = hc.words("d0.5", E, nch, rng)
    busy_t = _busy(w)
    out = _run(s, busy_t, E, nch, lags, eps)
    assert out.host() == ht.update(None, w, nch, lags, eps, True).tobytes() and out.pads_untouched()

    def rc(b=busy_t.data_ptr(), n_e=E, q=None, rp=out.records.data_ptr(), rb=out.rec_bytes, ws=out.ws.data_ptr(), wb=out.ws_bytes, nch=nch, eps=eps,
           lags=lags, r=None, n_lags=None, h=s._h):
        if q is None:
            q = cs.hop_params(nch, eps, lags, True)
            if r is not None:
                q.reserved[r] = 1
            if n_lags is not None:
                q.n_lags = n_lags
        v = lambda p: C.c_void_p(p or None)      # noqa: E731
        return L.crn_hops_device(h, v(b), n_e, C.byref(q) if q != 0 else None, v(rp), rb, v(ws), wb, None)
    assert rc() == 0
    for bad in ({"h": None}, {"b": 0}, {"q": 0}, {"rp": 0}, {"ws": 0}, {"n_e": -1}, {"nch": 0}, {"nch": 64}, {"n_lags": 0}, {"n_lags": 9},
                {"lags": (2, 1)}, {"lags": (1, 1)}, {"lags": (0, 1)}, {"lags": (0,)}, {"lags": (65,)}, {"lags": (1, 65)}, {"eps": 0}, {"eps": 3},
                {"r": 0}, {"r": 3}, {"b": busy_t.data_ptr() + 4}, {"ws": out.ws.data_ptr() + 4}, {"rp": out.records.data_ptr() + 8},
                {"rb": out.rec_bytes - 1}, {"rb": 0}, {"wb": out.ws_bytes - 1}, {"wb": 0}):
        assert rc(**bad) == cs.CRN_ERR_ARG, bad
        assert b"crn_hops_device" in L.crn_last_error()
    assert rc(n_e=0) == 0 and rc(n_e=0, rb=0) == 0 and rc(lags=(64,), rb=out.rec_bytes) == 0 and rc(nch=63) == 0
    torch.cuda.synchronize()
    s.close()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def _end_to_end(pu_model, lags):
    """The generator's chain of hops_cases.E2E through the CFAR launch and crn_channels_device, d_busy into crn_hops_device.  Returns
    (the records, the kernel's busy words, the truth's busy words, the number of epochs whose augmented words differ)."""
    e = hc.E2E
    n, k, S, T = e["n"], e["k"], e["n_streams"], e["eps"]
    E, nch = S * T, len(e["spans"])
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k)
    iq_t = sgpu.zeros((cs.samples_needed(cfg, E) * 2,), torch.float32)
    truth_t = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    sc = cs.SynthCfg()
    sc.seed, sc.noise_power, sc.signal_rms = e["seed"], e["noise_power"], e["signal_rms"]
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = e["tones"], pu_model, cs.SIG_TONES, S
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), E, cs.samples_per_epoch(cfg), sc, truth_ptr=truth_t.data_ptr())
    s.set_cfar(e["guard"], e["train"], cs.cfar_alpha(e["pfa"], k, e["train"]), 1)
    outs = sgpu.cfar_launch(s, cfg, iq_t, E)
    ch_out = sgpu.Padded(stats=S * nch * 192, busy=E * 8)
    ws_bytes = cs.channels_workspace_bytes(E, e["spans"], T, e["min_bins"])
    ws = sgpu.zeros((ws_bytes,), torch.uint8)
    s.channels_device(outs["mask"].data_ptr(), 0, E, ch_out.stats.data_ptr(), ws.data_ptr(), ws_bytes, e["spans"], epochs_per_stream=T,
                      min_bins=e["min_bins"], first=True, busy_ptr=ch_out.busy.data_ptr())
    out = _Out(E, S, nch, lags, T)
    s.hops_device(ch_out.busy.data_ptr(), E, cs.hop_params(nch, T, lags, True), out.records.data_ptr(), out.rec_bytes, out.ws.data_ptr(), out.ws_bytes)
    got = out.host()
    ch_out.host()
    busy = ch_out.view("busy", np.uint64)
    truth = truth_t.cpu().numpy()
    s.close()
    assert out.pads_untouched() and ch_out.pads_untouched()
    assert got == ht.update(None, busy, nch, lags, T, True).tobytes()            # the twin on the kernel's own words
    assert set(truth.tolist()) == {1, 2, 3}
    true_words = (np.uint64(1) << truth.astype(np.uint64)).astype(np.uint64)
    differ = sum(ht.augment(a, nch) != ht.augment(b, nch) for a, b in zip(busy.tolist(), true_words.tolist()))
    print(f"end to end: {differ} of {E} epochs differ from the truth (cap {E // 100})")
    assert differ <= E // 100
    return np.frombuffer(got, ht.dtype(len(lags))), busy, true_words, differ


def test_end_to_end_markov_chain(built):
    """CRN_PU_MARKOV_INTENDED, lags 1 and 2: pooled over the streams, pair[0][i][j] / from[0][i] for CH1..CH3 lies within 4.5 binomial
    standard deviations sqrt(p (1 - p) / from[i]) of the chain's table and the lag-2 estimate within 4.5 of the table's square, plus
    2 x differing epochs / from[i] (one wrong epoch moves at most two pairs per lag)."""
    r, busy, true_words, differ = _end_to_end(cs.PU_MARKOV_INTENDED, (1, 2))
    for m, table in ((0, hc.TABLE), (1, hc.TABLE @ hc.TABLE)):
        pair = r["lags"]["pair"][:, m].astype(np.int64).sum(axis=0)
        frm = r["lags"]["from"][:, m].astype(np.int64).sum(axis=0)
        worst = 0.0
        for i in (1, 2, 3):
            for j in (1, 2, 3):
                p = table[i - 1, j - 1]
                est, sd = pair[i, j] / frm[i], np.sqrt(p * (1 - p) / frm[i])
                worst = max(worst, abs(est - p) / sd)
                assert abs(est - p) <= 4.5 * sd + 2 * differ / frm[i], (m, i, j, est, p, sd, int(frm[i]))
            print(f"lag {m + 1}, from CH{i} ({int(frm[i])} epochs): {np.round(pair[i, 1:4] / frm[i], 4).tolist()} against {np.round(table[i - 1], 4).tolist()}")
        print(f"lag {m + 1}: worst cell {worst:.2f} standard deviations")


def test_end_to_end_sweep(built):
    """CRN_PU_SWEEP (CH1, CH2, CH3, CH2, CH1, ..), lags 1 and 2: every count within 2 x differing epochs of the twin on the truth's
    words (equal when none differ), and the forecast knows the sweep's next stops: CH2 one epoch after CH1; two epochs on, CH3 after
    CH1 and CH2 after CH2, each with probability above 0.95."""
    lags = (1, 2)
    r, busy, true_words, differ = _end_to_end(cs.PU_SWEEP, lags)
    nch, T = len(hc.E2E["spans"]), hc.E2E["eps"]
    want = ht.update(None, true_words, nch, lags, T, True)
    for f in ("hop",):
        assert np.abs(r[f].astype(np.int64) - want[f]).max() <= 2 * differ, f
    for f in ("from", "to", "pair"):
        assert np.abs(r["lags"][f].astype(np.int64) - want["lags"][f]).max() <= 2 * differ, f
    if differ == 0:
        assert r.tobytes() == want.tobytes()
    for st in range(r.size):
        rec = cs.hop_record(r[st].tobytes(), len(lags))
        for m, now, then in ((0, 1, 2), (1, 1, 3), (1, 2, 2)):
            p = cs.hop_forecast(rec, m, 1 << now)
            assert int(np.argmax(p[:nch])) == then and p[then] > 0.95, (st, m, now, then, p[:nch])
    print("stream 0, one epoch after CH1:", np.round(cs.hop_forecast(cs.hop_record(r[0].tobytes(), 2), 0, 2)[:nch], 3).tolist(),
          "one epoch after CH2:", np.round(cs.hop_forecast(cs.hop_record(r[0].tobytes(), 2), 0, 4)[:nch], 3).tolist())


# CFAR launch + crn_channels_device (d_busy written, the plan's first 63 bands) against the same followed by crn_hops_device with the lags
# 1, 2, 3, 4.  Measured on an MI355X, two separate runs (profiles/r21_hops.txt): one stream of 6656 epochs, arm A 477.7 us,
# B / A = 1.0630, the stage alone 30.3 us; arm A 441.2 us, B / A = 1.0729, alone 30.3 us.  64 streams of 104: arm A 460.9 us, B / A = 1.0429,
# alone 18.8 us; arm A 425.9 us, B / A = 1.0540, alone 19.2 us.  The bar is the larger measured excess over arm A with the relative margin
# the other stages' speed tests carry, because boxes of the pool differ by a few per cent: 1 + 1.5 x 0.0729 = 1.109.
SPEED_EXCESS = 0.0729
SPEED_RATIO = 1.0 + 1.5 * SPEED_EXCESS


def test_cost_next_to_the_cfar_launch(built):
    """N = 4096, K = 10, rect, 64 bands, the 2.18 GB batch of 6656 epochs; the method of tests/stage_gpu.py (best_of_windows).  Arm A is
    the CFAR launch (`spectrum` written) followed by crn_channels_device writing d_busy for the plan's first 63 bands, arm B the same followed by
    crn_hops_device with four lags, both as one stream of 6656 epochs and as 64 streams of 104; the stage alone is measured in both
    layouts and printed."""
    n, k, nch, lags = 4096, 10, 63, (1, 2, 3, 4)
    cfg = sgpu.cfg(n, cs.WINDOW_RECT, k, bands=64)
    E = 6656
    iq_t = sgpu.add_tones(sgpu.noise_batch(E, k, n), E, k, n)
    s = cs.Sensor(cfg)
    s.set_cfar(2, 16, cs.cfar_alpha(1e-3, k, 16), 1)
    outs = sgpu.cfar_launch(s, cfg, iq_t, E)
    spans = [(sp.lo, sp.width) for sp in cs.channel_spans_from_bands(cfg)][:nch]
    busy_t = sgpu.zeros((E,), torch.int64)
    layouts = {}
    for name, eps in (("one stream", E), ("64 streams", 104)):
        ws_bytes = cs.channels_workspace_bytes(E, spans, eps, 1)
        layouts[name] = (eps, sgpu.zeros((E // eps * nch * 192,), torch.uint8), sgpu.zeros((ws_bytes,), torch.uint8), ws_bytes, _Out(E, E // eps, nch, lags, eps))
    torch.cuda.synchronize()

    def arm_a(name):
        eps, stats, ws, ws_bytes, _ = layouts[name]
        sgpu.cfar_launch(s, cfg, iq_t, E, outs=outs)
        s.channels_device(outs["mask"].data_ptr(), outs["spectrum"].data_ptr(), E, stats.data_ptr(), ws.data_ptr(), ws_bytes, spans,
                          epochs_per_stream=eps, first=True, busy_ptr=busy_t.data_ptr())

    def stage(name):
        eps, _, _, _, out = layouts[name]
        _run(s, busy_t, E, nch, lags, eps, out=out)

    def arm_b(name):
        arm_a(name)
        stage(name)
    arms = {}
    for name in layouts:
        arms.update({"A " + name: lambda name=name: arm_a(name), "B " + name: lambda name=name: arm_b(name), "alone " + name: lambda name=name: stage(name)})
    times = sgpu.best_of_windows(arms)
    recs = {name: np.frombuffer(layouts[name][4].host(), ht.dtype(len(lags))) for name in layouts}
    busy = busy_t.cpu().numpy().view(np.uint64)
    s.close()
    best = {name: min(v) for name, v in times.items()}
    for name in layouts:
        print(f"N=4096 K=10 rect 64 bands, {E} epochs, {name}: arm A (CFAR launch + channels) {best['A ' + name]:.4f} ms, B / A = "
              f"{best['B ' + name] / best['A ' + name]:.4f}, the two kernels alone {best['alone ' + name] * 1e3:.1f} us")
    # the two layouts saw the same epochs, and the stage counted them
    one, many = recs["one stream"], recs["64 streams"]
    assert int(one["n_epochs"][0]) == E and (many["n_epochs"] == 104).all()
    assert int(one["lags"]["to"][0, 0].sum()) >= E - 1 and 0 < int(one["hop"].sum())
    spot = ht.update(None, busy[:104], nch, lags, 104, True)
    assert many[0].tobytes() == spot[0].tobytes()
    for name in layouts:
        assert best["B " + name] <= SPEED_RATIO * best["A " + name], (name, best["B " + name] / best["A " + name], SPEED_RATIO)
