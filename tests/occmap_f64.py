"""The twin of crn_occmap_device, written from the definition in include/crn_sense.h: the sequential rule, one epoch after the other,
nothing of the kernels' chunks and joins.  For stream j, bin k, epoch t: s = bit k of the mask row, P the `spectrum` value (0 without
one), u its bit pattern as uint32 (0 without one); sat(x) = min(x, 2^31 - 1):

    R = the carried record; all zero when first or R.n_epochs <= 0;  R.run = max(R.run, 0)
    for each epoch of the stream in time order:
        if R.n_epochs > 0:
            a = R.state & 1
            if s != a: n_rise or n_fall = sat(.. + 1); R.run_max[a] = max(R.run_max[a], R.run); R.run = 0
            R.max_hold = umax(R.max_hold, u); R.min_hold = umin(R.min_hold, u)
        else:
            R.max_hold = R.min_hold = u
        R.state = s; R.run = sat(R.run + 1); R.n_epochs = sat(R.n_epochs + 1); R.n_busy = sat(R.n_busy + s); R.power[s] += P

`column` is that rule on one column in plain Python.  `update` is the same rule for a batch, the loop over the epochs kept and every
statement of it applied to all columns at once with numpy (int64, then narrowed); tests/test_occmap_host.py holds the two against each
other.  power[] is math.fsum of the carried sum and the column's terms: the exactly rounded sum, whatever the order."""
import math

import numpy as np

from mask_bits import pack_mask, unpack_mask  # noqa: F401  (one definition of the mask layout; the tests take the two names from here)

BIN = np.dtype([("n_epochs", "<i4"), ("n_busy", "<i4"), ("n_rise", "<i4"), ("n_fall", "<i4"), ("run", "<i4"), ("state", "<i4"),
                ("run_max", "<i4", (2,)), ("max_hold", "<f4"), ("min_hold", "<f4"), ("reserved", "<i4", (2,)), ("power", "<f8", (2,))])
STREAM = np.dtype([("busy_sum", "<i8"), ("n_epochs", "<i4"), ("usual_bins", "<i4"), ("clear_bins", "<i4"), ("busy_now", "<i4"),
                   ("reserved", "<i4", (2,))])
INT_FIELDS = ("n_epochs", "n_busy", "n_rise", "n_fall", "run", "state", "run_max", "reserved")
SAT = 2 ** 31 - 1


def sat(x):
    return min(x, SAT)


def bits_of(P):
    """float32 values -> their bit patterns as uint32."""
    return np.ascontiguousarray(P, np.float32).view(np.uint32)


def _fsum(terms):
    """math.fsum, which refuses inf - inf and NaN mixes that IEEE addition answers with NaN."""
    try:
        return math.fsum(terms)
    except (ValueError, OverflowError):
        return float(np.sum(np.asarray(terms, np.float64)))


def column(R, s_seq, P_seq, first=False):
    """The rule on one record: R a dict of plain Python values (max_hold and min_hold as uint32 bit patterns, run_max and power lists);
    s_seq the 0 / 1 states, P_seq float32 values or None.  Returns the new dict."""
    R = {k: (list(v) if isinstance(v, list) else v) for k, v in R.items()}
    if first or R["n_epochs"] <= 0:
        R = {"n_epochs": 0, "n_busy": 0, "n_rise": 0, "n_fall": 0, "run": 0, "state": 0, "run_max": [0, 0], "max_hold": 0, "min_hold": 0,
             "reserved": [0, 0], "power": [0.0, 0.0]}
    R["run"] = max(R["run"], 0)
    terms = ([R["power"][0]], [R["power"][1]])
    for t, s in enumerate(s_seq):
        s = int(s)
        P = 0.0 if P_seq is None else float(P_seq[t])
        u = 0 if P_seq is None else int(np.float32(P_seq[t]).view(np.uint32))
        if R["n_epochs"] > 0:
            a = R["state"] & 1
            if s != a:
                if a == 0:
                    R["n_rise"] = sat(R["n_rise"] + 1)
                else:
                    R["n_fall"] = sat(R["n_fall"] + 1)
                R["run_max"][a] = max(R["run_max"][a], R["run"])
                R["run"] = 0
            R["max_hold"] = max(R["max_hold"], u)
            R["min_hold"] = min(R["min_hold"], u)
        else:
            R["max_hold"] = R["min_hold"] = u
        R["state"] = s
        R["run"] = sat(R["run"] + 1)
        R["n_epochs"] = sat(R["n_epochs"] + 1)
        R["n_busy"] = sat(R["n_busy"] + s)
        terms[s].append(P)
    R["power"] = [_fsum(terms[0]), _fsum(terms[1])]
    R["reserved"] = [0, 0]
    return R


def to_dict(rec):
    R = {f: rec[f].tolist() for f in BIN.names}
    R["max_hold"] = int(np.float32(rec["max_hold"]).view(np.uint32))
    R["min_hold"] = int(np.float32(rec["min_hold"]).view(np.uint32))
    return R


def from_dict(R):
    rec = np.zeros((), BIN)
    for f in BIN.names:
        if f not in ("max_hold", "min_hold"):
            rec[f] = R[f]
    rec["max_hold"] = np.uint32(R["max_hold"]).view(np.float32)
    rec["min_hold"] = np.uint32(R["min_hold"]).view(np.float32)
    return rec


def update(bins, det, spectrum, epochs_per_stream, first):
    """bins [S][N] BIN (may be None with first), det [E][N] bool, spectrum [E][N] float32 values or None.  Returns the new records."""
    det = np.asarray(det, bool)
    E, n = det.shape
    T = int(epochs_per_stream)
    S = E // T
    det = det.reshape(S, T, n)
    P = None if spectrum is None else np.ascontiguousarray(spectrum, np.float32).reshape(S, T, n)
    old = np.zeros((S, n), BIN) if bins is None else np.asarray(bins).reshape(S, n).copy()
    empty = np.full((S, n), True) if first else old["n_epochs"] <= 0
    old[empty] = np.zeros((), BIN)
    i64 = {f: old[f].astype(np.int64) for f in ("n_epochs", "n_busy", "n_rise", "n_fall", "run", "state")}
    rm = old["run_max"].astype(np.int64)
    hi, lo = bits_of(old["max_hold"]).copy(), bits_of(old["min_hold"]).copy()
    i64["run"] = np.maximum(i64["run"], 0)
    for t in range(T):
        s = det[:, t].astype(np.int64)
        u = np.zeros((S, n), np.uint32) if P is None else bits_of(P[:, t])
        seen = i64["n_epochs"] > 0
        a = i64["state"] & 1
        flip = seen & (s != a)
        i64["n_rise"] = np.where(flip & (a == 0), np.minimum(i64["n_rise"] + 1, SAT), i64["n_rise"])
        i64["n_fall"] = np.where(flip & (a == 1), np.minimum(i64["n_fall"] + 1, SAT), i64["n_fall"])
        for st in (0, 1):
            rm[..., st] = np.where(flip & (a == st), np.maximum(rm[..., st], i64["run"]), rm[..., st])
        i64["run"] = np.where(flip, 0, i64["run"])
        hi = np.where(seen, np.maximum(hi, u), u)
        lo = np.where(seen, np.minimum(lo, u), u)
        i64["state"] = s
        i64["run"] = np.minimum(i64["run"] + 1, SAT)
        i64["n_epochs"] = np.minimum(i64["n_epochs"] + 1, SAT)
        i64["n_busy"] = np.minimum(i64["n_busy"] + s, SAT)
    out = np.zeros((S, n), BIN)
    for f, v in i64.items():
        out[f] = v
    out["run_max"] = rm
    out["max_hold"], out["min_hold"] = hi.view(np.float32), lo.view(np.float32)
    out["power"] = old["power"]
    if P is not None:
        P64 = P.astype(np.float64)
        for st in (0, 1):
            terms = np.where(det == bool(st), P64, 0.0)                    # a term of +0.0 changes no sum
            cols = np.concatenate([old["power"][:, None, :, st], terms], axis=1).transpose(0, 2, 1).tolist()
            out["power"][..., st] = [[_fsum(c) for c in row] for row in cols]
    return out


def headers(bins, duty_ppm):
    """(streams [S] STREAM, usual mask [S][N / 32] uint32) of the records as a call leaves them."""
    bins = np.asarray(bins)
    S, n = bins.shape
    ne, nb = bins["n_epochs"].astype(np.int64), bins["n_busy"].astype(np.int64)
    usual = (ne > 0) & (nb * 10 ** 6 >= int(duty_ppm) * ne)
    st = np.zeros(S, STREAM)
    st["busy_sum"] = nb.sum(axis=1)
    st["n_epochs"] = bins["n_epochs"][:, 0]
    st["usual_bins"] = usual.sum(axis=1)
    st["clear_bins"] = (nb == 0).sum(axis=1)
    st["busy_now"] = ((bins["state"] & 1) != 0).sum(axis=1)
    return st, pack_mask(usual)


def exact_bytes(bins):
    """The fields that must be the same bytes whatever the cut: everything but power[]."""
    bins = np.asarray(bins)
    return b"".join(np.ascontiguousarray(bins[f]).tobytes() for f in INT_FIELDS + ("max_hold", "min_hold"))


def compare(got, want, what=""):
    """Every integer field equal, max_hold and min_hold the same bits; power[] within n_epochs 2^-52 relative of the twin's exactly
    rounded sum (the bound of an fp64 sum of n non-negative terms in any order: n - 1 additions of relative error 2^-53 each, and the
    twin's own rounding), NaN and inf exactly where the twin has them.  Returns the largest error in units of that bound."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    for f in INT_FIELDS:
        bad = got[f] != want[f]
        assert not bad.any(), (what, f, np.argwhere(bad)[:6].tolist(), got[f][bad][:6], want[f][bad][:6])
    for f in ("max_hold", "min_hold"):
        bad = bits_of(got[f]) != bits_of(want[f])
        assert not bad.any(), (what, f, np.argwhere(bad)[:6].tolist(), got[f][bad][:6], want[f][bad][:6])
    g, w = got["power"], want["power"]
    odd = ~np.isfinite(w)
    assert (np.isnan(g) == np.isnan(w)).all() and (g[odd & ~np.isnan(w)] == w[odd & ~np.isnan(w)]).all(), (what, "power: NaN / inf")
    assert np.isfinite(g[~odd]).all(), (what, "power: NaN / inf where the twin has a number")
    bound = np.maximum(want["n_epochs"], 1).astype(np.float64)[..., None] * 2.0 ** -52 * np.abs(w)
    err = np.where(odd, 0.0, np.abs(np.where(odd, 0.0, g) - np.where(odd, 0.0, w)))
    bad = err > bound
    assert not bad.any(), (what, "power", np.argwhere(bad)[:6].tolist(), g[bad][:6], w[bad][:6])
    with np.errstate(all="ignore"):
        return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0), initial=0.0))
