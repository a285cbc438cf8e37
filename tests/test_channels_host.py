"""Channel statistics without a GPU: the twin (tests/channels_f64.py) on hand-written sequences whose answers are written out here by
hand from the rule in include/crn_sense.h; the C ABI (symbols, the three structure sizes, the refusals that need no device, the
workspace size); crn_channel_forecast against its closed forms; best_channel's tie rules; channel_spans_from_bands.

What is refused without a device: crn_channels_device needs a handle for everything but its NULL-handle refusal (a handle needs a
device), so here its parameter refusals are reached through crn_channels_workspace_bytes, which runs the same checking code with the
span limit of the largest fft_len, 4096.  The span limits of the handle's own fft_len, the alignments, d_power without d_spectrum and
the workspace that is too small need a live handle: tests/test_channels_gpu.py::test_refusals_and_any_handle, as tests/test_segments_host.py
leaves the like to tests/test_segments_gpu.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import channels_f64 as ch
import crnsense as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fields(R):
    return (int(R["n_epochs"]), int(R["n_busy"]), R["n_trans"].tolist(), R["n_runs"].tolist(), R["run_sum"].tolist(), R["run_max"].tolist(),
            int(R["run"]), int(R["state"]))


def _hist(**bins):
    h = [0] * 16
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


# ---- the twin, by hand ----------------------------------------------------------------------------------------------------------
def test_all_idle_and_all_busy():
    R = ch.sequence([0] * 10)
    assert _fields(R) == (10, 0, [[9, 0], [0, 0]], [0, 0], [0, 0], [0, 0], 10, 0) and R["idle_hist"].tolist() == _hist()
    R = ch.sequence([1] * 10)
    assert _fields(R) == (10, 10, [[0, 0], [0, 9]], [0, 0], [0, 0], [0, 0], 10, 1) and R["idle_hist"].tolist() == _hist()
    R = ch.sequence([1])
    assert _fields(R) == (1, 1, [[0, 0], [0, 0]], [0, 0], [0, 0], [0, 0], 1, 1)
    assert _fields(ch.sequence([])) == (0, 0, [[0, 0], [0, 0]], [0, 0], [0, 0], [0, 0], 0, 0)


def test_alternating():
    """0 1 0 1 0 1 0 1: seven transitions, seven completed runs of one epoch (four idle, the first of them the left-censored one, and
    three busy), the eighth epoch is the run in progress."""
    R = ch.sequence([0, 1] * 4)
    assert _fields(R) == (8, 4, [[0, 4], [3, 0]], [4, 3], [4, 3], [1, 1], 1, 1) and R["idle_hist"].tolist() == _hist(b0=4)
    R = ch.sequence([1, 0] * 4 + [1])
    assert _fields(R) == (9, 5, [[0, 4], [4, 0]], [4, 4], [4, 4], [1, 1], 1, 1) and R["idle_hist"].tolist() == _hist(b0=4)


def test_a_single_flip():
    R = ch.sequence([0] * 5 + [1] * 3)
    assert _fields(R) == (8, 3, [[4, 1], [0, 2]], [1, 0], [5, 0], [5, 0], 3, 1) and R["idle_hist"].tolist() == _hist(b2=1)
    R = ch.sequence([1] * 3 + [0] * 5)
    assert _fields(R) == (8, 3, [[4, 0], [1, 2]], [0, 1], [0, 3], [0, 3], 5, 0) and R["idle_hist"].tolist() == _hist()
    # a mixed one, every count by hand: runs 2 idle, 3 busy, 1 idle, then 1 busy in progress
    R = ch.sequence([0, 0, 1, 1, 1, 0, 1])
    assert _fields(R) == (7, 4, [[1, 2], [1, 2]], [2, 1], [3, 3], [2, 3], 1, 1) and R["idle_hist"].tolist() == _hist(b0=1, b1=1)


def test_long_runs_land_in_the_last_histogram_bin():
    """floor(log2) of 2^15 - 1 is 14, of 2^15 it is 15, and bin 15 also takes everything longer."""
    for length, b in ((2 ** 15 - 1, 14), (2 ** 15, 15), (2 ** 15 + 12345, 15), (2 ** 17, 15)):
        R = ch.sequence([0] * length + [1])
        assert _fields(R) == (length + 1, 1, [[length - 1, 1], [0, 0]], [1, 0], [length, 0], [length, 0], 1, 1)
        assert R["idle_hist"].tolist() == _hist(**{f"b{b}": 1})
    R = ch.sequence([1] * 2 ** 15 + [0])                # busy runs have no histogram
    assert R["idle_hist"].tolist() == _hist() and R["run_max"].tolist() == [0, 2 ** 15]


def test_invariants_and_cut_independence_of_the_rule():
    rng = np.random.default_rng(3)
    bits = (rng.random(700) < 0.3).astype(int).tolist()
    whole = ch.sequence(bits)
    assert whole["n_trans"].sum() == whole["n_epochs"] - 1 and whole["run_sum"].sum() + whole["run"] == whole["n_epochs"]
    busy = np.array(bits, np.uint64)
    st = ch.update(None, busy[:1], None, 1, True, 1)
    st = ch.update(st, busy[1:300], None, 299, False)
    st = ch.update(st, busy[300:], None, 400, False)
    ch.compare(st[0, 0], whole)


def test_epochs_of_the_twin():
    """n_det, busy and power of one hand-made epoch at N = 64: a span across the wrap, overlapping spans, min_bins above the width."""
    n = 64
    det = np.zeros((1, n), bool)
    det[0, [62, 63, 0, 5, 6]] = True
    P = np.arange(n, dtype=np.float64)[None, :] + 1.0
    spans = [(62, 4), (0, 8), (5, 1), (6, 2), (0, 64)]
    n_det, busy, power = ch.epochs(det, P, spans, 2)
    assert n_det.tolist() == [[3, 3, 1, 1, 5]]
    assert int(busy[0]) == 0b10011
    assert power.tolist() == [[63 + 64 + 1 + 2, 36.0, 6.0, 7 + 8, 64 * 65 / 2]]
    assert int(ch.epochs(det, None, spans, 4)[1][0]) == 0b10000 and not ch.epochs(det, None, spans, 4)[2].any()
    assert int(ch.epochs(det, None, [(5, 1)], 2)[1][0]) == 0          # min_bins larger than the width: never busy


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_structures_and_binding(built):
    L = cs.lib()
    for name in ("crn_channels_workspace_bytes", "crn_channels_device", "crn_channel_forecast"):
        assert name in cs.EXPORTS and hasattr(L, name)
    assert (C.sizeof(cs.ChannelSpan), C.sizeof(cs.ChannelParams), C.sizeof(cs.ChannelStats)) == (8, 544, 192)
    assert np.dtype(cs.CHANNEL_STATS_DTYPE).itemsize == 192 and np.dtype(cs.CHANNEL_STATS_DTYPE) == ch.STATS
    assert [(n, np.dtype(cs.CHANNEL_STATS_DTYPE).fields[n][1]) for n in ch.STATS.names] == \
        [(f[0], getattr(cs.ChannelStats, f[0]).offset) for f in cs.ChannelStats._fields_]
    hdr = open(os.path.join(ROOT, "include", "crn_sense.h")).read()
    assert re.search(r"#define CRN_MAX_CHANNELS 64\b", hdr) and cs.CRN_MAX_CHANNELS == 64

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.sub(r"\[\w+\]", "", f).strip() for decl in body.split(";") if decl.strip()
                for f in re.sub(r"^\s*(int32_t|int64_t|double|crn_channel_span)\s", "", decl.strip()).split(",")]
    assert fields("crn_channel_span") == [f[0] for f in cs.ChannelSpan._fields_]
    assert fields("crn_channel_params") == [f[0] for f in cs.ChannelParams._fields_]
    assert fields("crn_channel_stats") == list(ch.STATS.names)
    assert callable(cs.Sensor.channels_device)
    assert L.crn_abi_version() == cs.CRN_ABI_VERSION == 4     # additive: the ABI version stays


def test_refusals_that_need_no_device(built):
    L = cs.lib()
    q = cs.channel_params([(0, 8), (500, 24)], 4, 1)
    buf = (C.c_uint8 * 65536)()
    p = (C.addressof(buf) + 63) & ~63
    nb = L.crn_channels_workspace_bytes(8, C.byref(q))
    assert 0 < nb <= 65536 - 64
    # no handle: refused before anything is looked at, whatever else is right or wrong
    assert L.crn_channels_device(None, p, p, 8, C.byref(q), p, p, p, p, nb, None) == cs.CRN_ERR_ARG
    assert b"crn_channels_device" in L.crn_last_error()
    assert L.crn_channels_device(None, p, None, 0, C.byref(q), p, None, None, p, nb, None) == cs.CRN_ERR_ARG
    assert L.crn_channels_device(None, None, None, -1, None, None, None, None, None, 0, None) == cs.CRN_ERR_ARG
    assert not bytes(buf).strip(b"\0")


def test_workspace_bytes(built):
    L = cs.lib()

    def nb(E, spans=((0, 8), (500, 24)), eps=1, mb=1, first=0, r=(0, 0, 0, 0), nch=None):
        q = cs.channel_params(spans, eps, mb, first)
        for i, v in enumerate(r):
            q.reserved[i] = v
        if nch is not None:
            q.n_channels = nch
        return L.crn_channels_workspace_bytes(E, C.byref(q))
    assert nb(0) > 0 and nb(0, first=1) > 0 and nb(0, eps=1000) > 0
    sizes = [nb(E, eps=E or 1) for E in (0, 1, 2, 64, 65, 6656, 100000)]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    sizes = [nb(6656, spans=[(0, 1)] * c) for c in (1, 2, 3, 63, 64)]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # room for one busy word per epoch and one fp32 power per epoch and channel
    assert nb(6656, spans=[(0, 1)] * 64) >= 6656 * (8 + 64 * 4)
    assert nb(6656, eps=104) == cs.channels_workspace_bytes(6656, [(0, 8), (500, 24)], 104)
    assert nb(6656, spans=[(4095, 4096)]) > 0 and nb(6656, mb=5000) > 0 and nb(6656, first=7) > 0
    for bad in ({"E": -1}, {"nch": 0}, {"nch": 65}, {"nch": -1}, {"eps": 0}, {"eps": -4}, {"E": 10, "eps": 3}, {"mb": 0}, {"mb": -1},
                {"r": (1, 0, 0, 0)}, {"r": (0, 0, 0, 1)}, {"spans": [(-1, 4)]}, {"spans": [(0, 0)]}, {"spans": [(0, -2)]},
                {"spans": [(4096, 1)]}, {"spans": [(0, 4097)]}, {"spans": [(0, 8), (3, 0)]}):
        assert nb(**{"E": 6656, **bad}) == -1, bad
    assert L.crn_channels_workspace_bytes(4, None) == -1
    # the longest stream the parameters can name, 2^31 - 1 epochs: the size is computed in 64 bits (a busy word and a power per epoch,
    # and the time stage's summaries on top)
    big = 2 ** 31 - 1
    assert big * 12 < nb(big, spans=[(0, 1)], eps=big) < big * 16
    assert nb(2 * big, spans=[(0, 1)], eps=big) > nb(big, spans=[(0, 1)], eps=big)
    with pytest.raises(cs.CrnError):
        cs.channels_workspace_bytes(10, [(0, 8)], 3)
    with pytest.raises(ValueError):
        cs.channel_params([(0, 1)] * 65, 1)


# ---- the forecast -----------------------------------------------------------------------------------------------------------------
def _record(n00=0, n01=0, n10=0, n11=0, state=0, **kw):
    R = np.zeros((), ch.STATS)
    R["n_trans"] = [[n00, n01], [n10, n11]]
    R["state"] = state
    for k, v in kw.items():
        R[k] = v
    return R


def test_forecast_against_closed_forms(built):
    rel = 1e-12
    # known counts: 30 idle-idle, 10 idle-busy, 6 busy-idle, 18 busy-busy
    for state in (0, 1):
        R = _record(30, 10, 6, 18, state)
        for prior, p01, p10 in ((0.0, 10 / 40, 6 / 24), (1.0, 11 / 42, 7 / 26), (0.5, 10.5 / 41, 6.5 / 25)):
            for h in (1, 10):
                want = p10 * (1 - p01) ** (h - 1) if state else (1 - p01) ** h
                got = cs.channel_forecast(R, h, prior)
                assert got == pytest.approx((p01, p10, want), rel=rel), (state, prior, h)
                assert got == pytest.approx(ch.forecast(R, h, prior), rel=rel)
    # horizon 1 from a busy state is p10 itself, from an idle one 1 - p01
    assert cs.channel_forecast(_record(30, 10, 6, 18, 1), 1, 0.0)[2] == pytest.approx(0.25, rel=rel)
    assert cs.channel_forecast(_record(30, 10, 6, 18, 0), 1, 0.0)[2] == pytest.approx(0.75, rel=rel)
    # 0 / 0 gives 0.5: nothing seen at all, and a row never seen (prior 0 only; a positive prior gives 1/2 by itself)
    assert cs.channel_forecast(_record(), 1, 0.0) == pytest.approx((0.5, 0.5, 0.5), rel=rel)
    assert cs.channel_forecast(_record(), 3, 1.0) == pytest.approx((0.5, 0.5, 0.125), rel=rel)
    assert cs.channel_forecast(_record(7, 0, 0, 0, 0), 10, 0.0) == pytest.approx((0.0, 0.5, 1.0), rel=rel)
    assert cs.channel_forecast(_record(0, 0, 0, 9, 1), 10, 0.0) == pytest.approx((0.5, 0.0, 0.0), abs=0, rel=rel)
    # only bit 0 of the state is read
    assert cs.channel_forecast(_record(30, 10, 6, 18, 3), 4, 1.0) == cs.channel_forecast(_record(30, 10, 6, 18, 1), 4, 1.0)
    # large counts stay exact to the tolerance
    big = _record(2 ** 40, 2 ** 20, 3, 2 ** 41, 0)
    assert cs.channel_forecast(big, 10, 1.0)[2] == pytest.approx((1 - (2 ** 20 + 1) / (2 ** 40 + 2 ** 20 + 2)) ** 10, rel=rel)


def test_forecast_refusals_and_null_outputs(built):
    L = cs.lib()
    st = cs.ChannelStats()
    st.n_trans[0][0], st.n_trans[0][1] = 3, 1
    out = C.c_double(-1.0)
    assert L.crn_channel_forecast(None, 1, 1.0, None, None, C.byref(out)) == cs.CRN_ERR_ARG
    assert b"crn_channel_forecast" in L.crn_last_error()
    for h, prior in ((0, 1.0), (-3, 1.0), (1, -0.5), (1, float("nan")), (1, float("inf")), (1, float("-inf"))):
        assert L.crn_channel_forecast(C.byref(st), h, prior, None, None, C.byref(out)) == cs.CRN_ERR_ARG, (h, prior)
    assert out.value == -1.0
    assert L.crn_channel_forecast(C.byref(st), 2, 0.0, None, None, None) == 0
    assert L.crn_channel_forecast(C.byref(st), 2, 0.0, None, None, C.byref(out)) == 0 and out.value == pytest.approx(0.5625, rel=1e-12)
    assert L.crn_channel_forecast(C.byref(st), 2, 0.0, C.byref(out), None, None) == 0 and out.value == pytest.approx(0.25, rel=1e-12)
    assert L.crn_channel_forecast(C.byref(st), 2, 0.0, None, C.byref(out), None) == 0 and out.value == 0.5
    with pytest.raises(cs.CrnError):
        cs.channel_forecast(_record(), 0)


def test_best_channel_and_its_ties(built):
    quiet = dict(n_epochs=100, n_busy=20)
    rows = np.zeros(4, ch.STATS)
    rows[0] = _record(60, 19, 19, 1, 0, **quiet)          # leaves idle often
    rows[1] = _record(78, 1, 1, 19, 0, **quiet)           # the best: stays idle
    rows[2] = _record(78, 1, 1, 19, 1, **quiet)           # the same chain, but busy now
    rows[3] = _record(70, 9, 9, 11, 0, **quiet)
    assert cs.best_channel(rows, 5) == 1 and cs.best_channel(rows, 5, prior=0.0) == 1
    # equal p_idle: the lower idle power per bin wins
    rows[:] = _record(78, 1, 1, 19, 0, **quiet)
    rows["power"][:, 0] = [8.0, 4.0, 2.0, 6.0]            # over 80 idle epochs
    assert cs.best_channel(rows, 5) == 2
    assert cs.best_channel(rows, 5, widths=[1, 1, 8, 1]) == 2 and cs.best_channel(rows, 5, widths=[8, 1, 1, 8]) == 3
    # ... and then the lower index
    rows["power"][:, 0] = [3.0, 1.0, 1.0, 1.0]
    assert cs.best_channel(rows, 5) == 1
    rows["power"][:, 0] = 0.0
    assert cs.best_channel(rows, 5) == 0
    # a channel never seen idle has no idle power: it loses the tie
    rows[0] = _record(0, 0, 0, 0, 0, n_epochs=0, n_busy=0)
    rows[1:] = _record(0, 0, 0, 0, 0, n_epochs=4, n_busy=0)
    rows[1:]["state"] = 0
    assert cs.channel_forecast(rows[0], 2)[2] == cs.channel_forecast(rows[1], 2)[2] and cs.best_channel(rows, 2) == 1
    with pytest.raises(ValueError):
        cs.best_channel(rows[:0], 2)


def test_channel_spans_from_bands(built):
    w = cs.cfg_welch(4096, 10, 64)
    spans = cs.channel_spans_from_bands(w)
    assert [(s.lo, s.width) for s in spans] == [(64 * b, 64) for b in range(64)]
    w = cs.cfg_welch(512, 10, 64)
    assert [(s.lo, s.width) for s in cs.channel_spans_from_bands(w)] == [(8 * b, 8) for b in range(64)]
    # two segments that meet at the wrap are one circular interval; the energy plan's CH1 leaves a hole before the wrap and is refused
    two = cs.cfg_welch(512, 10, 64)
    two.n_bands, two.n_segs = 2, 3
    for i, (lo, hi, b) in enumerate(((0, 16, 0), (500, 512, 0), (100, 140, 1))):
        two.segs[i].lo, two.segs[i].hi, two.segs[i].band = lo, hi, b
    assert [(s.lo, s.width) for s in cs.channel_spans_from_bands(two)] == [(500, 28), (100, 40)]
    with pytest.raises(ValueError):
        cs.channel_spans_from_bands(cs.cfg_energy_scaled(4096))
