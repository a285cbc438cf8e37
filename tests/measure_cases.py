"""What tests/test_measure_host.py and tests/test_measure_gpu.py share: the hand-made rows and records both feed to the twin (and the GPU
test to the kernel), the parameter sets, the simulation and the bars."""
import numpy as np

import measure_f64 as mf

SEGMENT_DTYPE = [("lo", "<i4"), ("width", "<i4"), ("peak_bin", "<i4"), ("n_detected", "<i4"), ("power", "<f4"), ("peak_power", "<f4"),
                 ("centroid", "<f4"), ("reserved", "<f4")]
SEGMENT_EPOCH_DTYPE = [("n_found", "<i4"), ("n_stored", "<i4"), ("noise_bins", "<i4"), ("noise_mean", "<f4")]

XDB26 = float(np.float32(10.0 ** -2.6))
# (subtract_noise, tail_ppm, xdb_ratio): every value of each, and the pairs that matter (quarters with 0.5: Q == thr happens)
PARAMS = ((1, 5000, XDB26), (0, 0, 0.0), (1, 499999, 0.5), (0, 5000, 0.5), (1, 0, XDB26), (0, 499999, 0.0))


def rows(seed, epochs, n, quantised=False):
    """Gamma(10) rows of mean 1; quantised to quarters (0 included) so that Q == thr and Q == 0 happen all the time."""
    rng = np.random.default_rng(seed)
    P = rng.gamma(10.0, 0.1, (epochs, n))
    if quantised:
        P = np.round(P * 4.0) / 4.0
    return P.astype(np.float32)


def record(row, lo, width):
    """The record crn_segments_device would store for the span (lo, width) of `row`."""
    n = row.size
    idx = (lo + np.arange(width)) % n
    with np.errstate(all="ignore"):
        arg = int(np.argmax(np.nan_to_num(row[idx], nan=-1.0)))
        power = np.float32(row[idx].astype(np.float64).sum())
    return (lo, width, int(idx[arg]), width, power, row[idx][arg], np.float32(0), np.float32(0))


def spans(n, rng):
    """The spans every size is tried with: the widths around the 64-bin chunks, the whole row, one across the wrap."""
    out = [(int(rng.integers(0, n)), w) for w in (1, 2, 63, 64, 65, 127, 128, 129)]
    out += [(int(rng.integers(0, n)), n - 1), (0, n), (n - 10, 40), (n - 1, 2), (n - 200, 321)]
    return out


def hand_made(n, max_segments, quantised=False, seed=7):
    """(P [E][n] float32, headers [E], records [E][max_segments]): epochs with n_stored 0, 1 and max_segments, every span of spans() with
    the peak where the row has it, at the span's first bin and at its last, a span whose every bin is <= noise_mean, a row with a NaN
    inside a span, and a row of subnormals.  Slots beyond n_stored hold 0xFF bytes: nobody may take them for records."""
    rng = np.random.default_rng(seed + n + max_segments)
    todo = []                                                     # per epoch: (kind, [(lo, width, where the peak goes)])
    todo.append(("plain", []))
    todo.append(("plain", [(int(rng.integers(0, n)), 5, None)]))
    full = [(int(rng.integers(0, n)), int(rng.integers(1, 9)), None) for _ in range(max_segments)]
    todo.append(("plain", full))
    special = [(lo, w, where) for where in (None, "first", "last") for lo, w in spans(n, rng)]
    for i in range(0, len(special), min(max_segments, 13)):
        todo.append(("plain", special[i: i + min(max_segments, 13)]))
    todo.append(("below", [(100, 70, None)]))
    todo.append(("nan", [(200, 150, None)][:max_segments] + [(260, 3, None)][: max_segments - 1]))
    todo.append(("subnormal", [(n - 30, 100, None)]))
    E = len(todo)
    P = rows(seed + n, E, n, quantised)
    heads = np.zeros(E, np.dtype(SEGMENT_EPOCH_DTYPE))
    recs = np.frombuffer(b"\xff" * (E * max_segments * 32), np.dtype(SEGMENT_DTYPE)).reshape(E, max_segments).copy()
    for e, (kind, segs) in enumerate(todo):
        noise = np.float32(1.0)
        if kind == "below":
            lo, w, _ = segs[0]
            P[e, lo: lo + w] = np.minimum(P[e, lo: lo + w], np.float32(1.0))
            P[e, lo + 3] = np.float32(1.0)                          # Q == 0 exactly
        if kind == "nan":
            P[e, 260] = np.nan
        if kind == "subnormal":
            P[e] = (P[e].astype(np.float64) * 2.0 ** -140).astype(np.float32)     # subnormal fp32 values
            noise = np.float32(2.0 ** -140)
        for lo, w, where in segs:
            if where == "first":
                P[e, lo] = np.float32(40.0)
            if where == "last":
                P[e, (lo + w - 1) % n] = np.float32(41.0)
        heads[e] = (len(segs), len(segs), n, noise)
        for s, (lo, w, _) in enumerate(segs):
            recs[e, s] = record(P[e], lo, w)
    return P, heads, recs


# ---- the simulation ---------------------------------------------------------------------------------------------------------------
SIM = {"n": 1024, "k": 10, "rows": 400, "lo": 300, "width": 84, "emitter": (310, 64), "db": 10.0, "carrier_db": 30.0, "comb_db": 20.0}

# The bars, from the run of tests/test_measure_host.py::test_simulation with seed 2041 (DESIGN.md §5 quotes it), each widened by the
# spread that run shows.
# Occupied width (99 %, noise subtracted) of the flat 64-bin emitter: the run's mean is 64.06 bins with a standard deviation of 0.48 over
# the rows, every row within 64 .. 69 (77.7 without the subtraction).  Rule: the mean within three standard deviations of 64, the
# deviation rounded up to half a bin (1.5 bins); every row within the run's own range widened by as much again on either side (the
# run reaches + 5: 64 - 5 .. 64 + 10).
OBW_MEAN_WITHIN = 1.5
OBW_ROW_RANGE = (-5, 10)
# The -26 dB width of the carrier: 1 bin in every row of the run.  Rule: were one stray bin above the line in a tenth of the rows, as
# far away as the span allows, the mean would be at most 1 + 0.1 x 84 = 9.4; the bar is a mean of 3 bins, a third of that and a
# twentieth of the flat emitter's 81.
CARRIER_XDB_MEAN = 3.0
# The fill n_above / xdb_width: the run gives 0.889 for the flat emitter (standard deviation 0.028 over the rows) and 0.294 for the comb
# (0.044).  Rule: each mean may move by three of its deviations, 0.80 and 0.43, which still leaves the comb far below the flat one.
FILL_FLAT_MIN = 0.80
FILL_COMB_MAX = 0.43
# The crest: near the span's width for the carrier, near width / emitter width for the flat one (the run: 83.1 and 2.4, deviation 0.2
# both).  Rule: the deviations are too small to set a bar; the bars sit at the geometric middle of the two kinds, sqrt(83 x 2.4) = 14,
# moved towards each kind by a factor of 3.5: 4 and 50.
CREST_CARRIER_MIN = 50.0
CREST_FLAT_MAX = 4.0


def simulate(seed, kind, sim=SIM):
    """(P [rows][n] float32, headers, records [rows][1]): Gamma(k) noise of mean 1 everywhere; in every row one span of `width` bins is the
    segment.  kind "flat": the emitter's bins carry `db` dB over the noise, Gamma(k) as well; "carrier": one bin at the emitter's
    centre, carrier_db over the noise per bin, constant amplitude under complex noise; "comb": 8 such carriers 8 bins apart at comb_db.
    noise_mean is the mean of the bins outside the span, as the segment stage has it."""
    n, k, R = sim["n"], sim["k"], sim["rows"]
    rng = np.random.default_rng(seed)
    P = rng.gamma(float(k), 1.0 / k, (R, n))
    lo, width = sim["lo"], sim["width"]
    e0, ew = sim["emitter"]

    def cw(db):
        noise = (rng.normal(0, np.sqrt(0.5), (R, k)) + 1j * rng.normal(0, np.sqrt(0.5), (R, k)))
        return (np.abs(10.0 ** (db / 20.0) + noise) ** 2).mean(axis=1)
    if kind == "flat":
        P[:, e0: e0 + ew] += 10.0 ** (sim["db"] / 10.0) * rng.gamma(float(k), 1.0 / k, (R, ew))
    elif kind == "carrier":
        P[:, e0 + ew // 2] = cw(sim["carrier_db"])
    else:
        for b in range(e0 + 4, e0 + ew, 8):
            P[:, b] = cw(sim["comb_db"])
    P = P.astype(np.float32)
    heads = np.zeros(R, np.dtype(SEGMENT_EPOCH_DTYPE))
    recs = np.zeros((R, 1), np.dtype(SEGMENT_DTYPE))
    outside = np.ones(n, bool)
    outside[lo: lo + width] = False
    for r in range(R):
        heads[r] = (1, 1, n - width, np.float32(P[r, outside].astype(np.float64).mean()))
        recs[r, 0] = record(P[r], lo, width)
    return P, heads, recs


def figures(m):
    """Of the records m [rows] of one simulated kind: occupied widths, x-dB widths, fills, crests."""
    m = m.reshape(-1)
    return m["obw_width"].astype(float), m["xdb_width"].astype(float), m["n_above"] / np.maximum(m["xdb_width"], 1), m["crest"].astype(float)


def measure(P, heads, recs, max_segments, params):
    sub, ppm, ratio = params
    return mf.run(P, heads, recs, max_segments, ppm, ratio, sub)
