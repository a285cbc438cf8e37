"""The float64 / integer twin of crn_channels_device, written from the definition in include/crn_sense.h (plain numpy and Python, one
epoch after the other: the sequential rule, nothing of the kernels' chunks and joins):

  per epoch and channel   n_det = set mask bits inside the span (bins (lo + i) mod N, 0 <= i < width); busy = n_det >= min_bins;
                          power = the sum of P over the span's bins in float64 (0 without a spectrum)
  per stream and channel  if first: R = all zero; then for each epoch in time order, s the busy bit and p the fp32 power:
                              if R.n_epochs > 0:
                                  a = R.state & 1; R.n_trans[a][s] += 1
                                  if s != a: the run (a, R.run) is complete: n_runs, run_sum, run_max, idle_hist (a = 0); R.run = 0
                              R.state = s; R.run += 1; R.n_epochs += 1; R.n_busy += s; R.power[s] += p

`epochs` gives (n_det, busy words, powers in float64); `update` steps records (crnsense.CHANNEL_STATS_DTYPE) through busy words and fp32
powers (run_sequence is the rule itself); `forecast` is crn_channel_forecast's closed form."""
import numpy as np

from mask_bits import pack_mask, unpack_mask  # noqa: F401  (one definition of the mask layout; the tests take the two names from here)

STATS = np.dtype([("n_epochs", "<i8"), ("n_busy", "<i8"), ("n_trans", "<i8", (2, 2)), ("n_runs", "<i8", (2,)), ("run_sum", "<i8", (2,)),
                  ("run_max", "<i8", (2,)), ("run", "<i8"), ("state", "<i4"), ("reserved", "<i4"), ("power", "<f8", (2,)),
                  ("idle_hist", "<i4", (16,))])
INT_FIELDS = ("n_epochs", "n_busy", "n_trans", "n_runs", "run_sum", "run_max", "run", "state", "reserved", "idle_hist")
REL_TOL = 2.0 ** -22     # d_power: fp64 accumulation rounded to fp32 once, against the twin's float64 value (tests/segments_f64.py)


def span_bins(lo, width, n):
    return (lo + np.arange(width)) % n


def epochs(det, spectrum, spans, min_bins):
    """det [E][N] bool, spectrum [E][N] or None, spans [(lo, width)].  Returns (n_det [E][C] int, busy [E] uint64, power [E][C] float64)."""
    det = np.asarray(det, bool)
    E, n = det.shape
    n_det = np.zeros((E, len(spans)), np.int64)
    power = np.zeros((E, len(spans)), np.float64)
    for c, (lo, width) in enumerate(spans):
        idx = span_bins(lo, width, n)
        n_det[:, c] = det[:, idx].sum(axis=1)
        if spectrum is not None:
            power[:, c] = np.asarray(spectrum, np.float64)[:, idx].sum(axis=1)
    busy = np.zeros(E, np.uint64)
    for c in range(len(spans)):
        busy |= (n_det[:, c] >= min_bins).astype(np.uint64) << np.uint64(c)
    return n_det, busy, power


def hist_bin(run):
    return min(max(int(run), 1).bit_length() - 1, 15)


def run_sequence(R, bits, powers):
    """The rule, epoch after epoch, on one record: R a dict of plain Python values (lists for the arrays), changed in place."""
    for s, p in zip(bits, powers):
        if R["n_epochs"] > 0:
            a = R["state"] & 1
            R["n_trans"][a][s] += 1
            if s != a:
                R["n_runs"][a] += 1
                R["run_sum"][a] += R["run"]
                R["run_max"][a] = max(R["run_max"][a], R["run"])
                if a == 0:
                    R["idle_hist"][hist_bin(R["run"])] += 1
                R["run"] = 0
        R["state"] = s
        R["run"] += 1
        R["n_epochs"] += 1
        R["n_busy"] += s
        R["power"][s] += p


def _to_dict(rec):
    return {f: rec[f].tolist() for f in STATS.names}


def _from_dict(rec, R):
    for f in STATS.names:
        rec[f] = R[f]


def update(stats, busy, power, epochs_per_stream, first, n_channels=None):
    """stats [n_streams][C] STATS (may be None with first), busy [E] uint64, power [E][C] fp32 values or None.  Returns the new records."""
    busy = np.asarray(busy, np.uint64)
    n_streams = busy.size // epochs_per_stream
    if first:
        C_ = n_channels if n_channels is not None else power.shape[1] if power is not None else stats.shape[1]
        stats = np.zeros((n_streams, C_), STATS)
    else:
        stats = stats.copy()
    for st in range(stats.shape[0]):
        sl = slice(st * epochs_per_stream, (st + 1) * epochs_per_stream)
        for c in range(stats.shape[1]):
            bits = ((busy[sl] >> np.uint64(c)) & np.uint64(1)).astype(np.int64).tolist()
            pw = [0.0] * len(bits) if power is None else np.asarray(power[sl, c], np.float64).tolist()
            R = _to_dict(stats[st, c])
            run_sequence(R, bits, pw)
            _from_dict(stats[st, c], R)
    return stats


def sequence(bits):
    """One stream, one channel, no power: the record after the 0 / 1 sequence `bits`."""
    rec = np.zeros(1, STATS)
    R = _to_dict(rec[0])
    bits = [int(b) for b in bits]
    run_sequence(R, bits, [0.0] * len(bits))
    _from_dict(rec[0], R)
    return rec[0]


def forecast(R, horizon, prior):
    t = R["n_trans"].astype(np.float64)

    def leave(a):
        den = t[a][0] + t[a][1] + 2.0 * prior
        return (t[a][1 - a] + prior) / den if den > 0 else 0.5
    p01, p10 = leave(0), leave(1)
    return p01, p10, (p10 * (1.0 - p01) ** (horizon - 1) if int(R["state"]) & 1 else (1.0 - p01) ** horizon)


def compare(got, want, what=""):
    """Every integer field equal; power[] within 1e-9 relative (an fp64 sum of the same fp32 values in another order)."""
    for f in INT_FIELDS:
        assert (got[f] == want[f]).all(), (what, f, np.argwhere(got[f] != want[f])[:6], got[f][got[f] != want[f]][:6], want[f][got[f] != want[f]][:6])
    err = np.abs(got["power"] - want["power"])
    assert (err <= 1e-9 * np.abs(want["power"])).all(), (what, "power", float(err.max()))


def compare_power(got, want):
    """d_power against the twin's float64 sums: REL_TOL relative, exact zeros.  Returns the largest relative error."""
    got = np.asarray(got, np.float64)
    err = np.abs(got - want) / np.maximum(np.abs(want), 1e-300)
    err = np.where(want == 0, np.where(got == 0, 0.0, np.inf), err)
    assert (err <= REL_TOL).all(), (float(err.max()), np.argwhere(err > REL_TOL)[:6])
    return float(err.max()) if err.size else 0.0
