"""The float64 twin of crn_holes_device, written from the definition in include/crn_sense.h (plain numpy; the age goes epoch after epoch,
the holes bin after bin):

  1. blocked  b_t[k] = OR of d_t[(k + i) mod N] over |i| <= guard.
  2. age      a = first ? 0 : max(d_age[k], 0); per epoch in time order a = b_t[k] ? 0 : min(a + 1, 2^31 - 1).
  3. free     f[k] = age[k] >= min_age; free_bins counts them before any width filter.
  4. holes    the maximal circular runs of ones in f (all ones: lo = 0, width = N); width < min_width dropped; n_found counts the rest; the
              first min(n_found, max_holes) by ascending lo are stored; widest_* names the widest found hole, ties to the smallest lo.
  5. fields   age / age_max the smallest / largest age inside; Pbar[k] = fl32(sum of the last A = min(avg_epochs, T) rows in fp64, in
              time order, / A); peak_bin / peak_power the largest Pbar (ties: the smallest offset); power the fp64 sum of Pbar over the
              hole; floor_mean the fp64 sum of Pbar over the free bins / free_bins.  Without a spectrum the floats are 0, peak_bin = lo.

`run` gives the arrays in the kernel's layout (crnsense.HOLE_STREAM_DTYPE / HOLE_DTYPE) with `power` and `floor_mean` kept in float64, so
that a comparison can bound them."""
import numpy as np

from mask_bits import pack_mask, unpack_mask  # noqa: F401  (one definition of the mask layout; the tests take the two names from here)

AGE_MAX = 2 ** 31 - 1
STREAM_F64 = np.dtype([("n_found", "<i4"), ("n_stored", "<i4"), ("free_bins", "<i4"), ("widest_lo", "<i4"), ("widest_width", "<i4"),
                       ("widest_age", "<i4"), ("floor_mean", "<f8")])
HOLE_F64 = np.dtype([("lo", "<i4"), ("width", "<i4"), ("age", "<i4"), ("age_max", "<i4"), ("peak_bin", "<i4"), ("power", "<f8"),
                     ("peak_power", "<f4")])
STREAM_INTS = ("n_found", "n_stored", "free_bins", "widest_lo", "widest_width", "widest_age")
HOLE_INTS = ("lo", "width", "age", "age_max", "peak_bin")
REL_TOL = 2.0 ** -22     # power, floor_mean: fp64 accumulation rounded to fp32 once, against the twin's float64 value


def dilate(d, guard):
    """Step 1: the blocked bins of the boolean mask d, one epoch [N] or several [T][N] (circular along the bins)."""
    d = np.asarray(d, bool)
    b = d.copy()
    for i in range(1, guard + 1):
        b |= np.roll(d, i, axis=-1) | np.roll(d, -i, axis=-1)
    return b


def ages(det, guard, start=None):
    """Step 2 for one stream, epoch after epoch: det [T][N] bool, start [N] (None: first != 0).  Returns int32 [N]."""
    det = np.asarray(det, bool)
    a = np.zeros(det.shape[1], np.int64) if start is None else np.maximum(np.asarray(start, np.int64), 0)
    for b in dilate(det, guard):
        a = np.where(b, 0, np.minimum(a + 1, AGE_MAX))
    return a.astype(np.int32)


def ages_closed(det, guard, start=None):
    """The closed form of step 2: T - 1 - t* where the bin was blocked last in epoch t*, min(start + T, 2^31 - 1) where it never was."""
    det = np.asarray(det, bool)
    T, n = det.shape
    a0 = np.zeros(n, np.int64) if start is None else np.maximum(np.asarray(start, np.int64), 0)
    out = np.minimum(a0 + T, AGE_MAX)
    b = dilate(det, guard)
    for k in range(n):
        hit = np.flatnonzero(b[:, k])
        if hit.size:
            out[k] = T - 1 - hit[-1]
    return out.astype(np.int32)


def runs_of(f):
    """Step 4, bin after bin: [(lo, width)] of the maximal circular runs of ones, ascending lo."""
    f = [bool(x) for x in f]
    n = len(f)
    if all(f):
        return [(0, n)]
    out = []
    for k in range(n):
        if f[k] and not f[k - 1]:
            w = 1
            while f[(k + w) % n]:
                w += 1
            out.append((k, w))
    return out


def pbar(P, avg_epochs):
    """Pbar of one stream's rows P [T][N]: the fp64 sum of the last A rows in time order, over A, rounded to fp32."""
    P = np.asarray(P, np.float32)
    A = min(avg_epochs, P.shape[0])
    s = np.zeros(P.shape[1], np.float64)
    for t in range(P.shape[0] - A, P.shape[0]):
        s = s + P[t].astype(np.float64)
    return (s / float(A)).astype(np.float32)


def stream(age, pb, min_age, min_width, max_holes):
    """Steps 3 to 5 of one stream from its ages [N] and Pbar [N] (or None): (free [N] bool, header dict, list of hole dicts)."""
    age = np.asarray(age, np.int64)
    n = age.size
    f = age >= min_age
    free_bins = int(f.sum())
    found = [r for r in runs_of(f) if r[1] >= min_width]
    hdr = {"n_found": len(found), "n_stored": min(len(found), max_holes), "free_bins": free_bins, "widest_lo": 0, "widest_width": 0,
           "widest_age": 0, "floor_mean": 0.0}
    if pb is not None and free_bins:
        hdr["floor_mean"] = float(pb[f].astype(np.float64).sum() / free_bins)
    for lo, w in found:
        if w > hdr["widest_width"]:                      # ascending lo: the first of equal widths stays
            hdr["widest_lo"], hdr["widest_width"] = lo, w
            hdr["widest_age"] = int(age[(lo + np.arange(w)) % n].min())
    holes = []
    for lo, w in found[:max_holes]:
        idx = (lo + np.arange(w)) % n
        h = {"lo": lo, "width": w, "age": int(age[idx].min()), "age_max": int(age[idx].max()), "peak_bin": lo, "power": 0.0, "peak_power": 0.0}
        if pb is not None:
            p = pb[idx]
            i = int(np.argmax(p))                        # the first of equal maxima
            h["peak_bin"], h["peak_power"], h["power"] = int(idx[i]), p[i], float(p.astype(np.float64).sum())
        holes.append(h)
    return f, hdr, holes


def run(det, P, eps, guard=0, min_age=1, min_width=1, max_holes=16, avg_epochs=1, age=None):
    """A batch: det [S eps][N] bool, P [S eps][N] or None, age [S][N] the carry (None: first != 0).
    Returns (age [S][N] int32, free [S][N] bool, streams [S] STREAM_F64, holes [S][max_holes] HOLE_F64, zero-filled)."""
    det = np.asarray(det, bool)
    E, n = det.shape
    S = E // eps
    out_age = np.zeros((S, n), np.int32)
    free = np.zeros((S, n), bool)
    streams = np.zeros(S, STREAM_F64)
    holes = np.zeros((S, max_holes), HOLE_F64)
    for s in range(S):
        out_age[s] = ages(det[s * eps: (s + 1) * eps], guard, None if age is None else age[s])
        pb = None if P is None else pbar(P[s * eps: (s + 1) * eps], avg_epochs)
        free[s], hdr, hs = stream(out_age[s], pb, min_age, min_width, max_holes)
        for k, v in hdr.items():
            streams[s][k] = v
        for j, h in enumerate(hs):
            for k, v in h.items():
                holes[s, j][k] = v
    return out_age, free, streams, holes


def compare(got_streams, got_holes, want_streams, want_holes, what=""):
    """The exact comparison: every integer field and peak_bin equal, peak_power the same bits, the slots beyond n_stored all zero bytes,
    power and floor_mean within REL_TOL of the twin's float64.  got_*: the kernel's arrays (crnsense dtypes; got_holes may be None).
    Returns the largest relative error seen."""
    worst = 0.0
    for f in STREAM_INTS:
        assert (got_streams[f] == want_streams[f]).all(), (what, f, np.flatnonzero(got_streams[f] != want_streams[f])[:8],
                                                           got_streams[f][:4], want_streams[f][:4])
    assert (got_streams["reserved"] == 0).all(), (what, "reserved")

    def rel(got, want, name):
        nonlocal worst
        err = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)
        err = np.where(want == 0, np.where(got == 0, 0.0, np.inf), err)
        if err.size:
            worst = max(worst, float(err.max()))
        assert (err <= REL_TOL).all(), (what, name, float(err.max()), np.argwhere(err > REL_TOL)[:8])
    rel(got_streams["floor_mean"], want_streams["floor_mean"], "floor_mean")
    if got_holes is None:
        return worst
    for f in HOLE_INTS:
        assert (got_holes[f] == want_holes[f]).all(), (what, f, np.argwhere(got_holes[f] != want_holes[f])[:8])
    assert (got_holes["peak_power"].view(np.uint32) == want_holes["peak_power"].view(np.uint32)).all(), (what, "peak_power")
    assert (got_holes["reserved"] == 0).all(), (what, "reserved")
    used = np.arange(got_holes.shape[1])[None, :] < want_streams["n_stored"][:, None]
    assert not np.frombuffer(got_holes[~used].tobytes(), np.uint8).any(), (what, "slots beyond n_stored are not zero")
    rel(got_holes["power"], want_holes["power"], "power")
    return worst
