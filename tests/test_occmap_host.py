"""The occupancy map without a GPU: the twin (tests/occmap_f64.py) against an independent statement of the same fields by run-length
encoding each column; the twin's two forms against each other; its cut independence; the Python helpers; the C ABI (symbols, the three
structure sizes, the workspace size, the refusals that need no device); and a simulation of what the stage buys, in the definition's own
terms: the floor's shape from mean_idle.

What is refused without a device: crn_occmap_device needs a handle for everything but its NULL-handle refusal (a handle needs a device),
so here its parameter refusals are reached through crn_occmap_workspace_bytes, which runs the same checking code.  The alignments and the
workspace that is too small need a live handle: tests/test_occmap_gpu.py::test_refusals_with_a_live_handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crnsense as cs
import occmap_cases as oc
import occmap_f64 as om

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the twin -------------------------------------------------------------------------------------------------------------------
def _by_runs(s, P):
    """The record of one column from zero, stated over its runs and not epoch by epoch: (fields dict, the two power sums)."""
    s = np.asarray(s, int)
    T = s.size
    edges = np.flatnonzero(np.diff(s)) + 1                       # where a new run starts
    starts = np.concatenate([[0], edges])
    lengths = np.diff(np.concatenate([starts, [T]]))
    states = s[starts]
    done_len, done_state = lengths[:-1], states[:-1]             # every run but the one in progress is complete, the first included
    u = om.bits_of(P) if P is not None else np.zeros(T, np.uint32)
    want = {"n_epochs": T, "n_busy": int(s.sum()), "n_rise": int((states[1:] == 1).sum()), "n_fall": int((states[1:] == 0).sum()),
            "run": int(lengths[-1]), "state": int(s[-1]),
            "run_max": [int(done_len[done_state == a].max(initial=0)) for a in (0, 1)], "max_hold": int(u.max()), "min_hold": int(u.min())}
    pw = [0.0, 0.0] if P is None else [float(np.sum(np.asarray(P, np.float64)[s == a])) for a in (0, 1)]
    return want, pw


def _columns(rng):
    cols = [oc.pattern(kind, T, rng) for kind in range(oc.N_PATTERNS) for T in oc.LENGTHS]
    cols += [(rng.random(T) < p).astype(int) for T in (1, 5, 64, 300) for p in (0.02, 0.5, 0.97)]
    return cols


def test_twin_against_run_lengths():
    rng = np.random.default_rng(1)
    zero = om.to_dict(np.zeros((), om.BIN))
    for s in _columns(rng):
        for P in (None, oc.rows(s.size, s.size, 1, quantised=bool(s.size % 2))[:, 0]):
            R = om.column(zero, s, P, first=True)
            want, pw = _by_runs(s, P)
            assert {k: R[k] for k in want} == want, (s.tolist(), R, want)
            assert R["power"] == pytest.approx(pw, rel=1e-12, abs=0) and R["reserved"] == [0, 0]
            assert R["n_rise"] + R["n_fall"] <= R["n_epochs"] - 1 and abs(R["n_rise"] - R["n_fall"]) <= 1


def test_the_twin_by_hand():
    zero = om.to_dict(np.zeros((), om.BIN))

    def rec(bits, **kw):
        R = om.column(zero, bits, None, **kw)
        return (R["n_epochs"], R["n_busy"], R["n_rise"], R["n_fall"], R["run"], R["state"], R["run_max"])
    assert rec([0] * 10) == (10, 0, 0, 0, 10, 0, [0, 0])
    assert rec([1]) == (1, 1, 0, 0, 1, 1, [0, 0])
    # 0 0 1 1 1 0 1: the left-censored idle run of 2 counts when it ends; the run in progress is in no figure
    assert rec([0, 0, 1, 1, 1, 0, 1]) == (7, 4, 2, 1, 1, 1, [2, 3])
    assert rec([0, 1] * 4) == (8, 4, 4, 3, 1, 1, [1, 1])
    # max hold and min hold compare bit patterns: -1.0 lies above NaN above +inf above 2.0, and 0.0 is the smallest of all
    R = om.column(zero, [0, 0, 0], np.array([2.0, np.inf, 0.5], np.float32))
    assert (R["max_hold"], R["min_hold"]) == (0x7f800000, 0x3f000000)
    R = om.column(zero, [0, 1, 0, 1], np.array([np.nan, np.inf, -1.0, 0.0], np.float32))
    assert (R["max_hold"], R["min_hold"]) == (0xbf800000, 0)
    assert np.isnan(R["power"][0]) and R["power"][1] == np.inf


def test_carried_records_of_the_rule():
    """What the header says of a carry: n_epochs <= 0 is empty, run below 0 is 0, only bit 0 of state is read, and the counts saturate."""
    zero = om.to_dict(np.zeros((), om.BIN))
    R = dict(zero, n_epochs=-5, n_busy=77, n_rise=9, run=12, state=1, run_max=[40, 50], max_hold=99, power=[3.0, 4.0])
    assert om.column(R, [1, 1, 0], None) == om.column(zero, [1, 1, 0], None, first=True)
    R = dict(zero, n_epochs=4, n_busy=4, run=-7, state=1, run_max=[0, 0])
    got = om.column(R, [1, 0], None)
    assert (got["run_max"], got["run"], got["n_fall"], got["n_epochs"]) == ([0, 1], 1, 1, 6)
    a, b = (om.column(dict(zero, n_epochs=3, state=st, run=2), [0, 0, 1], None) for st in (0x7ffffffe, 0))
    assert a == b and a["run_max"] == [4, 0] and a["n_rise"] == 1 and a["n_fall"] == 0
    big = 2 ** 31 - 3
    got = om.column(dict(zero, n_epochs=big, n_busy=big, run=big, state=1, run_max=[3, 8]), [1] * 5, None)
    assert (got["n_epochs"], got["n_busy"], got["run"], got["run_max"]) == (om.SAT, om.SAT, om.SAT, [3, 8])
    got = om.column(dict(zero, n_epochs=big, n_busy=big, run=big, state=1, run_max=[3, 8]), [1, 1, 1, 1, 0], None)
    assert (got["run"], got["run_max"], got["n_fall"]) == (1, [3, om.SAT], 1)


def _batch(seed, S, T, n, carry=False):
    rng = np.random.default_rng(seed)
    det = rng.random((S * T, n)) < rng.random(n)[None, :]
    P = oc.rows(seed, S * T, n, quantised=True)
    bins = None
    if carry:
        bins = om.update(None, rng.random((S * 9, n)) < 0.4, oc.rows(seed + 1, S * 9, n), 9, True)
        bins["n_epochs"][0, :3] = (-1, 0, -9)
        bins["run"][0, 3] = -4
        bins["state"][0, 4:6] = (6, 7)
    return det, P, bins


def test_the_two_forms_of_the_twin_agree():
    """update, the rule applied to all columns at once, against column, the rule in plain Python: the same bytes, power[] included."""
    S, T, n = 2, 70, 32
    for carry in (False, True):
        det, P, bins = _batch(7, S, T, n, carry)
        for spec in (P, None):
            got = om.update(bins, det, spec, T, not carry)
            for j in range(S):
                for k in range(n):
                    old = om.to_dict(np.zeros((), om.BIN) if bins is None else bins[j, k])
                    col = None if spec is None else spec.reshape(S, T, n)[j, :, k]
                    want = om.from_dict(om.column(old, det.reshape(S, T, n)[j, :, k], col, first=not carry))
                    assert got[j, k].tobytes() == want.tobytes(), (carry, j, k, got[j, k], want)


def test_cut_independence_of_the_rule():
    S, T, n = 2, 193, 32
    det, P, _ = _batch(9, S, T, n)
    whole = om.update(None, det, P, T, True)
    for cuts in (oc.CUTS, (192, 1), (64, 129)):
        assert sum(cuts) == T
        bins, a = None, 0
        for c in cuts:
            part = lambda x: x.reshape(S, T, n)[:, a: a + c].reshape(S * c, n)       # noqa: E731
            bins = om.update(bins, part(det), part(P), c, a == 0)
            a += c
        assert om.exact_bytes(bins) == om.exact_bytes(whole), cuts
        om.compare(bins, whole, f"cuts {cuts}")
        for duty in (1, 500000, 1000000):
            h1, m1 = om.headers(bins, duty)
            h2, m2 = om.headers(whole, duty)
            assert h1.tobytes() == h2.tobytes() and m1.tobytes() == m2.tobytes()


def test_headers_of_the_twin():
    bins = np.zeros((1, 64), om.BIN)
    bins["n_epochs"] = 10
    bins["n_busy"][0, :4] = (10, 5, 4, 1)
    bins["state"][0, :3] = (1, 3, 2)
    for duty, want in ((1, 0b1111), (100000, 0b1111), (100001, 0b0111), (500000, 0b0011), (500001, 0b0001), (1000000, 0b0001)):
        st, mask = om.headers(bins, duty)
        assert mask.tolist() == [[want, 0]], duty
        assert (int(st["busy_sum"][0]), int(st["n_epochs"][0]), int(st["usual_bins"][0]), int(st["clear_bins"][0]), int(st["busy_now"][0])) == \
            (20, 10, bin(want).count("1"), 60, 2)


# ---- the Python helpers -----------------------------------------------------------------------------------------------------------
def test_occupancy_map_and_floor_db():
    bins = np.zeros((2, 3), cs.OCCMAP_BIN_DTYPE)
    bins["n_epochs"] = 8
    bins["n_busy"][0] = (0, 2, 8)
    bins["n_rise"][0] = (0, 2, 0)
    bins["power"][0, :, 0] = (8.0, 0.6, 0.0)
    bins["power"][0, :, 1] = (0.0, 20.0, 80.0)
    bins["max_hold"][0], bins["min_hold"][0] = (3.0, 12.0, 11.0), (0.5, 0.05, 9.0)
    bins["n_epochs"][1] = 0
    m = cs.occupancy_map(bins)
    assert sorted(m) == ["duty", "max_hold", "mean_busy", "mean_idle", "min_hold", "rise_rate"] and all(v.shape == (2, 3) for v in m.values())
    assert m["duty"].tolist() == [[0.0, 0.25, 1.0], [0, 0, 0]] and m["rise_rate"].tolist() == [[0.0, 0.25, 0.0], [0, 0, 0]]
    assert m["mean_idle"][0] == pytest.approx([1.0, 0.1, 0.0]) and m["mean_busy"][0].tolist() == [0.0, 10.0, 10.0]
    assert not m["mean_idle"][1].any() and not m["mean_busy"][1].any()
    assert m["max_hold"][0].tolist() == [3.0, 12.0, 11.0] and m["min_hold"][0].tolist() == [0.5, pytest.approx(0.05), 9.0]
    db = cs.floor_db(bins)
    assert db[0, :2] == pytest.approx([0.0, -10.0]) and np.isnan(db[0, 2]) and np.isnan(db[1]).all()
    assert cs.floor_db(bins, fallback=-3.0)[0].tolist() == pytest.approx([0.0, -10.0, -3.0]) and (cs.floor_db(bins, -3.0)[1] == -3.0).all()
    assert cs.occupancy_map(bins[0, 1])["duty"] == 0.25                       # one record
    q = cs.occmap_params(12)
    assert (q.epochs_per_stream, q.first, q.duty_ppm, list(q.reserved)) == (12, 0, 500000, [0] * 5)
    q = cs.occmap_params(3, duty=0.123456, first=True)
    assert (q.epochs_per_stream, q.first, q.duty_ppm) == (3, 1, 123456)


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_structures_and_binding(built):
    L = cs.lib()
    for name in ("crn_occmap_workspace_bytes", "crn_occmap_device"):
        assert name in cs.EXPORTS and hasattr(L, name)
    assert C.sizeof(cs.OccmapParams) == 32
    assert np.dtype(cs.OCCMAP_BIN_DTYPE).itemsize == 64 and np.dtype(cs.OCCMAP_BIN_DTYPE) == om.BIN
    assert np.dtype(cs.OCCMAP_STREAM_DTYPE).itemsize == 32 and np.dtype(cs.OCCMAP_STREAM_DTYPE) == om.STREAM
    hdr = open(os.path.join(ROOT, "include", "crn_sense.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.sub(r"\[\w+\]", "", f).strip() for decl in body.split(";") if decl.strip()
                for f in re.sub(r"^\s*(int32_t|int64_t|double|float)\s", "", decl.strip()).split(",")]
    assert fields("crn_occmap_params") == [f[0] for f in cs.OccmapParams._fields_]
    assert fields("crn_occmap_bin") == list(om.BIN.names) and fields("crn_occmap_stream") == list(om.STREAM.names)
    assert [om.BIN.fields[f][1] for f in om.BIN.names] == [0, 4, 8, 12, 16, 20, 24, 32, 36, 40, 48]
    assert [om.STREAM.fields[f][1] for f in om.STREAM.names] == [0, 8, 12, 16, 20, 24]
    assert callable(cs.Sensor.occmap_device)
    assert L.crn_abi_version() == cs.CRN_ABI_VERSION == 4     # additive: the ABI version stays


def test_refusals_that_need_no_device(built):
    L = cs.lib()
    q = cs.occmap_params(4)
    buf = (C.c_uint8 * 65536)()
    p = (C.addressof(buf) + 63) & ~63
    nb = L.crn_occmap_workspace_bytes(8, C.byref(q))
    assert nb > 0
    # no handle: refused before anything is looked at, whatever else is right or wrong
    assert L.crn_occmap_device(None, p, p, 8, C.byref(q), p, p, p, p, nb, None) == cs.CRN_ERR_ARG
    assert b"crn_occmap_device" in L.crn_last_error()
    assert L.crn_occmap_device(None, p, None, 0, C.byref(q), p, p, None, p, nb, None) == cs.CRN_ERR_ARG
    assert L.crn_occmap_device(None, None, None, -1, None, None, None, None, None, 0, None) == cs.CRN_ERR_ARG
    assert not bytes(buf).strip(b"\0")


def test_workspace_bytes(built):
    L = cs.lib()

    def nb(E, eps=1, duty=500000, first=0, r=(0, 0, 0, 0, 0)):
        q = cs.OccmapParams(epochs_per_stream=eps, first=first, duty_ppm=duty)
        for i, v in enumerate(r):
            q.reserved[i] = v
        return L.crn_occmap_workspace_bytes(E, C.byref(q))
    assert nb(0) > 0 and nb(0, first=1) > 0 and nb(0, eps=1000) > 0
    sizes = [nb(E, eps=E or 1) for E in (0, 1, 2, 64, 65, 6656, 100000)]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    # room for a 32-byte summary per bin of the largest fft_len and chunk of 64 epochs, and the 64 shares of a header
    assert nb(6656, eps=512) >= 13 * 8 * 4096 * 32 + 13 * 64 * 32
    assert nb(6656, eps=104) == cs.occmap_workspace_bytes(6656, 104) and nb(6656, eps=6656) == cs.occmap_workspace_bytes(6656)
    assert nb(6656, duty=1) > 0 and nb(6656, duty=1000000) > 0 and nb(6656, first=7) > 0
    for bad in ({"E": -1}, {"eps": 0}, {"eps": -4}, {"E": 10, "eps": 3}, {"duty": 0}, {"duty": -1}, {"duty": 1000001},
                {"r": (1, 0, 0, 0, 0)}, {"r": (0, 0, 0, 0, 1)}, {"r": (0, 0, -1, 0, 0)}):
        assert nb(**{"E": 6656, **bad}) == -1, bad
    assert L.crn_occmap_workspace_bytes(4, None) == -1
    big = 2 ** 31 - 1                                       # the longest stream the parameters can name: the size is computed in 64 bits
    assert nb(big, eps=big) > big // 64 * 4096 * 32 and nb(2 * big, eps=big) > nb(big, eps=big)
    with pytest.raises(cs.CrnError):
        cs.occmap_workspace_bytes(10, 3)
    with pytest.raises(cs.CrnError):
        cs.occmap_workspace_bytes(10, 10, duty=0.0)


# ---- what the stage buys ----------------------------------------------------------------------------------------------------------
def test_simulation(built):
    """tests/occmap_cases.py, SIM: a floor that falls 6 dB towards the band edges, three carriers switched by two-state chains, the mask
    of the CA-CFAR twin at Pfa 1e-2; the twin of this stage over the 256 rows.  Away from the carriers mean_idle recovers the floor's
    shape bin by bin within 5 / sqrt(K n_idle), the derived bar; a per-row estimate (one number) cannot.  The carriers' bins and their
    CFAR neighbourhood are held to the measured bars of occmap_cases.py."""
    sim = oc.SIM
    k = sim["k"]
    P, det, floor, on = oc.simulate(2051, cs.cfar_alpha(sim["pfa"], k, sim["train"]))
    bins = om.update(None, det, P, sim["rows"], True)
    m = cs.occupancy_map(bins[0])
    away, near = oc.neighbourhood()
    n_idle = (bins["n_epochs"] - bins["n_busy"])[0].astype(float)
    sig = np.abs(m["mean_idle"] / floor - 1.0) * np.sqrt(k * np.maximum(n_idle, 1))
    print(f"away from the carriers ({int(away.sum())} bins): mean_idle / floor - 1 in standard deviations: largest {sig[away].max():.2f}, rms "
          f"{np.sqrt((sig[away] ** 2).mean()):.2f} (bar {oc.FLOOR_SIGMAS}); mean bias {(m['mean_idle'] / floor - 1.0)[away].mean() * 100:+.2f} %; "
          f"fewest idle epochs {int(n_idle[away].min())}")
    assert n_idle[away].min() > 0.9 * sim["rows"] and (sig[away] <= oc.FLOOR_SIGMAS).all()
    # the floor's shape is there: the map spans the 6 dB, one number per row spans nothing
    db = cs.floor_db(bins[0])
    true_db = 10.0 * np.log10(floor)
    edge, middle = db[:32].mean(), db[480:512].mean()
    print(f"floor_db: {middle:+.2f} dB mid-band, {edge:+.2f} dB over the 32 bins at the edge (true {true_db[480:512].mean():+.2f}, {true_db[:32].mean():+.2f})")
    # (a bin's dB figure scatters by 4.34 / sqrt(K n_idle) = 0.09 dB, the mean of 32 by 0.015 dB, the difference of two by 0.02 dB: 0.1 is
    # five of those; the truncation bias is the same at both ends and cancels)
    assert middle - edge == pytest.approx(true_db[480:512].mean() - true_db[:32].mean(), abs=0.1) and middle - edge > 5.0
    print(f"neighbourhoods ({int(near.sum())} bins): largest {sig[near].max():.2f}, rms {np.sqrt((sig[near] ** 2).mean()):.2f} (bar {oc.NEIGH_SIGMAS})")
    assert (sig[near] <= oc.NEIGH_SIGMAS).all()
    for b, st in on.items():
        d, idle = m["duty"][b] - st.mean(), m["mean_idle"][b] / floor[b]
        busy = bins["power"][0, b, 1] / sim["rows"] / (st.mean() * (1 + 10 ** (sim["snr_db"] / 10)) * floor[b])
        print(f"carrier at bin {b}: on in {st.mean():.4f} of the rows, duty {m['duty'][b]:.4f} ({d:+.4f}); mean_idle / floor {idle:.3f}, "
              f"mean_busy / floor {m['mean_busy'][b] / floor[b]:.2f}, busy power over the carrier's {busy:.3f}; rises {int(bins['n_rise'][0, b])}, "
              f"longest busy run {int(bins['run_max'][0, b, 1])}")
        assert oc.DUTY_RANGE[0] <= d <= oc.DUTY_RANGE[1]
        assert oc.CARRIER_IDLE_RANGE[0] <= idle <= oc.CARRIER_IDLE_RANGE[1] and oc.CARRIER_BUSY_RANGE[0] <= busy <= oc.CARRIER_BUSY_RANGE[1]
    # the usual mask at duty 0.5: the carriers that are on more often than off, and nothing else
    st, mask = om.headers(bins, 500000)
    usual = np.flatnonzero(om.unpack_mask(mask, sim["n"])[0]).tolist()
    assert usual == sorted(b for b, s in on.items() if m["duty"][b] >= 0.5) and int(st["usual_bins"][0]) == len(usual)
