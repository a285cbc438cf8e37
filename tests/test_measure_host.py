"""crn_measure_device without a GPU: the twin (tests/measure_f64.py) against a second, brute-force statement of the definition on random and
hand-made rows; the binding; the refusals that need no device; and the simulation whose figures DESIGN.md §5 quotes, with the bars of
tests/measure_cases.py."""
import ctypes as C
import math
import os
import re

import numpy as np

import crnsense as cs
import measure_cases as mc
import measure_f64 as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the twin against a second statement ------------------------------------------------------------------------------------------
def _brute(row, n, lo, width, peak, nm, tail_ppm, ratio):
    """The definition once more, nothing shared with the twin but the fp32 scalars: every prefix sum is summed from scratch, the
    crossings are the minimum and the maximum of the sets the header names, the exponent comes from comparing powers of two."""
    f = np.float32
    peak, nm, ratio = f(peak), f(nm), f(ratio)
    if lo < 0 or lo > n - 1 or width < 1 or width > n or np.isnan(peak) or np.isinf(peak) or peak <= 0:
        return None
    with np.errstate(all="ignore"):
        pq = peak - nm
        thr = ratio * pq
    if not pq > 0:
        return None
    e = -149
    while 2.0 ** (e + 1) <= float(peak):
        e += 1
    q, above = [], []
    with np.errstate(all="ignore"):
        for i in range(width):
            Q = f(row[(lo + i) % n]) - nm
            v = float(Q) * 2.0 ** (30 - e) if Q > 0 else 0.0
            q.append(2 ** 31 - 1 if v >= 2 ** 31 - 1 else int(v))
            if Q > thr:
                above.append(i)
    S0 = sum(q)
    if S0 == 0:
        return None
    T = S0 * tail_ppm // 1000000
    low = min(i for i in range(width) if sum(q[: i + 1]) > T)
    high = max(i for i in range(width) if S0 - sum(q[:i]) > T)
    x = (above[0], above[-1] - above[0] + 1) if above else (0, 0)
    return (low, high - low + 1, x[0], x[1], len(above), f(math.ldexp(S0, e - 30)), f(max(q) * width / S0), f(0))


def _brute_run(P, heads, recs, max_segments, params):
    sub, ppm, ratio = params
    out = np.zeros((P.shape[0], max_segments), np.dtype(mf.MEASURE_DTYPE))
    for e in range(P.shape[0]):
        nm = np.float32(heads["noise_mean"][e])
        nm = nm if sub and np.isfinite(nm) and nm > 0 else np.float32(0)
        for s in range(min(max(int(heads["n_stored"][e]), 0), max_segments)):
            g = recs[e, s]
            r = _brute(P[e], P.shape[1], int(g["lo"]), int(g["width"]), g["peak_power"], nm, ppm, ratio)
            if r is not None:
                out[e, s] = r
    return out


def test_twin_against_brute_force_on_hand_made_rows():
    """N = 512 (the brute force is quadratic in the width), max_segments 1 and 16, Gamma(10) rows and rows quantised to quarters, every
    parameter set of measure_cases.PARAMS: tail_ppm 0 and 499999, xdb_ratio 0 and 0.5 (with quarters, Q == thr occurs and must not
    count)."""
    ties = 0
    for ms in (1, 16):
        for quantised in (False, True):
            P, heads, recs = mc.hand_made(512, ms, quantised)
            for params in mc.PARAMS:
                got, want = mc.measure(P, heads, recs, ms, params), _brute_run(P, heads, recs, ms, params)
                assert got.tobytes() == want.tobytes(), (ms, quantised, params, np.argwhere(got != want)[:4])
                assert (got["obw_width"][got["net_power"] > 0] >= 1).all() and (got["reserved"] == 0).all()
                if params[1] == 0:          # nothing left outside: the occupied span ends on the outermost bins over the noise
                    assert (got["obw_lo"] <= got["xdb_lo"])[got["n_above"] > 0].all()
            if quantised:
                # Q == thr happens in these rows, and is not above
                nm = np.float32(1.0)
                for e in range(P.shape[0]):
                    for s in range(min(int(heads["n_stored"][e]), ms)):
                        g = recs[e, s]
                        Q = P[e, (g["lo"] + np.arange(g["width"])) % 512] - nm
                        ties += int((Q == np.float32(0.5) * (g["peak_power"] - nm)).sum())
    assert ties > 0


def test_twin_on_small_cases_by_hand():
    """Rows a reader can follow: powers of two, so q is Q 2^(30 - e) exactly."""
    n = 512
    row = np.zeros(n, np.float32)
    row[10:18] = [1, 1, 8, 8, 8, 8, 1, 1]                                     # S0 = 36 units of 2^27
    got = mf.segment(row, n, 10, 8, 8.0, 0.0, 0, 0.5)
    assert got[:5] == (0, 8, 2, 4, 4) and got[5] == 36.0 and got[6] == np.float32(8 * 8 / 36)
    # 5 % on each side: T = 1.8 units, the first and the last bin (1 unit each) fall outside, the second does not
    assert mf.segment(row, n, 10, 8, 8.0, 0.0, 50000, 0.5)[:2] == (1, 6)
    assert mf.segment(row, n, 10, 8, 8.0, 0.0, 499999, 0.5)[:2] == (3, 2)     # just under half on each side: the two middle bins
    assert mf.segment(row, n, 10, 8, 8.0, 0.0, 0, 0.125)[2:5] == (2, 4, 4)    # Q == thr is not above
    assert mf.segment(row, n, 10, 8, 8.0, 0.0, 0, 0.0)[2:5] == (0, 8, 8)
    assert mf.segment(row, n, 10, 8, 8.0, 1.0, 0, 0.0)[:6] == (2, 4, 2, 4, 4, np.float32(28.0))   # the ones vanish under the noise
    assert mf.segment(row, n, 8, 12, 8.0, 0.0, 0, 0.0)[:5] == (2, 8, 2, 8, 8)                     # zero bins at the span's ends
    # across the wrap
    row[:] = 0
    row[[510, 511, 0, 1]] = [2, 4, 4, 2]
    assert mf.segment(row, n, 509, 6, 4.0, 0.0, 0, 0.6)[:5] == (1, 4, 2, 2, 2)
    # nothing to measure
    for lo, w, peak, nm in ((-1, 4, 4.0, 0.0), (512, 4, 4.0, 0.0), (0, 0, 4.0, 0.0), (0, 513, 4.0, 0.0), (0, 4, np.nan, 0.0), (0, 4, np.inf, 0.0),
                            (0, 4, 0.0, 0.0), (0, 4, -1.0, 0.0), (0, 4, 4.0, 4.0), (100, 4, 4.0, 0.0)):
        assert mf.segment(row, n, lo, w, peak, nm, 5000, 0.5) is None, (lo, w, peak, nm)
    # a subnormal peak: e = -149 + its highest bit
    tiny = np.float32(2.0 ** -149)
    row[40:43] = [tiny, 3 * tiny, tiny]
    assert mf.exponent(3 * tiny) == -148
    got = mf.segment(row, n, 40, 3, 3 * tiny, 0.0, 0, 0.5)
    assert got[:5] == (0, 3, 1, 1, 1) and got[5] == 5 * tiny and got[6] == np.float32(9 / 5)
    # a bin far above the record's peak_power is clamped, not wrapped
    row[60:62] = [1.0, 1e30]
    assert mf.segment(row, n, 60, 2, 1.0, 0.0, 0, 0.5)[:2] == (0, 2)
    assert mf.integers(row, n, 60, 2, 0.0, 0)[1] == [2 ** 30, 2 ** 31 - 1]


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_structures_and_binding(built):
    L = cs.lib()
    assert "crn_measure_device" in cs.EXPORTS and hasattr(L, "crn_measure_device")
    assert C.sizeof(cs.MeasureParams) == 32 and np.dtype(cs.MEASURE_DTYPE).itemsize == 32
    assert cs.MEASURE_DTYPE == mf.MEASURE_DTYPE and mc.SEGMENT_DTYPE == cs.SEGMENT_DTYPE and mc.SEGMENT_EPOCH_DTYPE == cs.SEGMENT_EPOCH_DTYPE
    hdr = open(os.path.join(ROOT, "include", "crn_sense.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip()
                for f in re.sub(r"^\s*(int32_t|float)\s", "", decl.strip()).split(",")]
    assert fields("crn_measure_params") == [f[0] for f in cs.MeasureParams._fields_]
    assert fields("crn_measure") == [f[0] for f in cs.MEASURE_DTYPE]
    assert "/* 32 bytes */" in hdr[hdr.index("} crn_measure_params;"):][:40] and "/* 32 bytes */" in hdr[hdr.index("} crn_measure;"):][:40]
    assert hdr.index("crn_tcfar_device(") < hdr.index("crn_measure_device(") < hdr.index("crn_sense_reserve_host(")
    assert callable(cs.Sensor.measure_device)
    assert L.crn_abi_version() == cs.CRN_ABI_VERSION == 4     # additive: the ABI version stays
    q = cs.measure_params()
    assert (q.max_segments, q.tail_ppm, q.subtract_noise, list(q.reserved)) == (16, 5000, 1, [0, 0, 0, 0])
    assert q.xdb_ratio == np.float32(10.0 ** -2.6) and cs.xdb_ratio(26.0) == 10.0 ** -2.6 and cs.xdb_ratio(3.0) == 10.0 ** -0.3
    q = cs.measure_params(256, obw_percent=99.9, xdb=6.0, subtract_noise=False)
    assert (q.max_segments, q.tail_ppm, q.subtract_noise) == (256, 500, 0)
    assert cs.measure_params(obw_percent=100.0).tail_ppm == 0 and cs.measure_params(obw_percent=90.0).tail_ppm == 50000


def test_measure_hz():
    """A segment at bins 100 .. 139 of 1024 at 1.024 MHz (1 kHz per bin) around 100 MHz: occupied bins 104 .. 135, x-dB bins 110 .. 119."""
    (f_obw, b_obw), (f_x, b_x) = cs.measure_hz(100, 4, 32, 10, 10, 1024, 1.024e6, 100e6)
    assert (f_obw, b_obw) == (100e6 + 119.5e3, 32e3) and (f_x, b_x) == (100e6 + 114.5e3, 10e3)
    # across the wrap: bins 1020 .. 1023, 0 .. 3 centre on fc - 0.5 bin
    assert cs.measure_hz(1016, 4, 8, 0, 0, 1024, 1.024e6, 100e6)[0] == (100e6 - 0.5e3, 8e3)
    assert cs.measure_hz(1016, 4, 8, 0, 0, 1024, 1.024e6, 100e6)[1][1] == 0.0


def test_no_handle_is_refused_before_anything_is_looked_at(built):
    L = cs.lib()
    q = cs.measure_params()
    buf = (C.c_uint8 * 65536)()
    p = (C.addressof(buf) + 63) & ~63
    assert L.crn_measure_device(None, p, 8, C.byref(q), p, p, p, None) == cs.CRN_ERR_ARG
    assert b"crn_measure_device" in L.crn_last_error()
    assert L.crn_measure_device(None, None, -1, None, None, None, None, None) == cs.CRN_ERR_ARG
    assert not bytes(buf).strip(b"\0")


# ---- the simulation -------------------------------------------------------------------------------------------------------------
def test_simulation():
    """N = 1024, K = 10, 400 rows of Gamma(10) noise; the segment is an 84-bin span around a 64-bin flat emitter at +10 dB per bin, around a
    carrier at +30 dB, and around a comb of 8 carriers at +20 dB.  99 % occupied bandwidth and the -26 dB rule with the noise
    subtracted, and the occupied width once more without.  The bars and their rules are in tests/measure_cases.py."""
    q = (1, 5000, mc.XDB26)
    fig = {}
    for kind in ("flat", "carrier", "comb"):
        P, heads, recs = mc.simulate(2041, kind)
        obw, xdb, fill, crest = mc.figures(mc.measure(P, heads, recs, 1, q))
        fig[kind] = (obw, xdb, fill, crest)
        print(f"{kind}: occupied width {obw.mean():.2f} bins (sd {obw.std():.2f}, {obw.min():.0f} .. {obw.max():.0f}); -26 dB width {xdb.mean():.2f} "
              f"(sd {xdb.std():.2f}, max {xdb.max():.0f}); fill {fill.mean():.3f} (sd {fill.std():.3f}); crest {crest.mean():.1f} (sd {crest.std():.1f})")
    P, heads, recs = mc.simulate(2041, "flat")
    raw = mc.figures(mc.measure(P, heads, recs, 1, (0, 5000, mc.XDB26)))[0]
    print(f"flat, noise not subtracted: occupied width {raw.mean():.2f} bins ({raw.min():.0f} .. {raw.max():.0f})")
    ew = mc.SIM["emitter"][1]
    obw = fig["flat"][0]
    assert abs(obw.mean() - ew) <= mc.OBW_MEAN_WITHIN, obw.mean()
    assert ew + mc.OBW_ROW_RANGE[0] <= obw.min() and obw.max() <= ew + mc.OBW_ROW_RANGE[1], (obw.min(), obw.max())
    assert raw.mean() > obw.mean() + 5.0                       # without subtraction the noise of the 20 bins around widens it
    assert fig["carrier"][1].mean() <= mc.CARRIER_XDB_MEAN, fig["carrier"][1].mean()
    assert fig["flat"][2].mean() >= mc.FILL_FLAT_MIN and fig["comb"][2].mean() <= mc.FILL_COMB_MAX, (fig["flat"][2].mean(), fig["comb"][2].mean())
    assert fig["carrier"][3].mean() >= mc.CREST_CARRIER_MIN and fig["flat"][3].mean() <= mc.CREST_FLAT_MAX
