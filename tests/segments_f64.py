"""The float64 twin of crn_segments_device, written from the definition in include/crn_sense.h (plain numpy, one epoch at a time):

  1. closing   no bit set: no segments.  Otherwise every maximal circular run of zero bits of length <= merge_gap joins the closed mask c.
  2. segments  the maximal circular runs of ones in c; c all ones: one segment, lo = 0, width = N.
  3. noise     before any filtering: noise_bins = bins with c = 0, noise_mean = the mean of P over them (0 when there are none).
  4. filter    width < min_width dropped; n_found counts the rest; the first min(n_found, max_segments) by ascending lo are stored.
  5. stored    lo, width, n_detected, peak_bin (ties: the smallest offset), peak_power, power, centroid = sum(i P) / sum(P).

`run` gives the two arrays in the kernel's layout (crnsense.SEGMENT_EPOCH_DTYPE / SEGMENT_DTYPE) with the float fields kept in float64,
so that a comparison can round or bound them as it needs."""
import numpy as np

from mask_bits import pack_mask, unpack_mask  # noqa: F401  (one definition of the mask layout; the tests take the two names from here)

EPOCH_F64 = np.dtype([("n_found", "<i4"), ("n_stored", "<i4"), ("noise_bins", "<i4"), ("noise_mean", "<f8")])
SEGMENT_F64 = np.dtype([("lo", "<i4"), ("width", "<i4"), ("peak_bin", "<i4"), ("n_detected", "<i4"),
                        ("power", "<f8"), ("peak_power", "<f8"), ("centroid", "<f8")])


def close_mask(d, merge_gap):
    """Step 1 for one epoch: the closed mask c of the boolean mask d (circular)."""
    d = np.asarray(d, bool)
    n = d.size
    c = d.copy()
    ones = np.flatnonzero(d)
    if ones.size == 0 or merge_gap <= 0:
        return c
    # the zero run behind each set bit reaches to the next set bit, circularly (the last one's run wraps to the first)
    nxt = np.roll(ones, -1)
    gaps = (nxt - ones - 1) % n
    if ones.size == 1:
        gaps[:] = n - 1
    for k, gap in zip(ones, gaps):
        if 0 < gap <= merge_gap:
            c[(k + 1 + np.arange(gap)) % n] = True
    return c


def runs_of(c):
    """Step 2: [(lo, width)] of the maximal circular runs of ones, ascending lo."""
    c = np.asarray(c, bool)
    n = c.size
    if c.all():
        return [(0, n)]
    starts = np.flatnonzero(c & ~np.roll(c, 1))
    zeros = np.flatnonzero(~c)
    out = []
    for lo in starts:
        # the first zero at or after lo, circularly
        j = np.searchsorted(zeros, lo)
        end = zeros[j] if j < zeros.size else zeros[0] + n
        out.append((int(lo), int(end - lo)))
    return out


def epoch(d, P, merge_gap=0, min_width=1, max_segments=16):
    """One epoch: (header dict, list of segment dicts), every float in float64."""
    d = np.asarray(d, bool)
    P = np.asarray(P, np.float64)
    n = d.size
    c = close_mask(d, merge_gap)
    noise_bins = int(n - c.sum())
    hdr = {"noise_bins": noise_bins, "noise_mean": float(P[~c].sum() / noise_bins) if noise_bins else 0.0}
    runs = [r for r in (runs_of(c) if d.any() else []) if r[1] >= min_width]
    hdr["n_found"] = len(runs)
    runs = runs[:max_segments]
    hdr["n_stored"] = len(runs)
    segs = []
    for lo, w in runs:
        idx = (lo + np.arange(w)) % n
        p = P[idx]
        s0 = float(p.sum())
        i = int(np.argmax(p))                      # the first of equal maxima
        segs.append({"lo": lo, "width": w, "peak_bin": int(idx[i]), "n_detected": int(d[idx].sum()), "power": s0,
                     "peak_power": float(p[i]), "centroid": float((np.arange(w) * p).sum() / s0) if s0 > 0 else 0.0})
    return hdr, segs


def run(det, spectrum, merge_gap=0, min_width=1, max_segments=16):
    """A batch: det [E][N] bool, spectrum [E][N].  Returns (epochs [E] EPOCH_F64, segments [E][max_segments] SEGMENT_F64, zero-filled)."""
    det = np.asarray(det, bool)
    E = det.shape[0]
    eps = np.zeros(E, EPOCH_F64)
    segs = np.zeros((E, max_segments), SEGMENT_F64)
    for e in range(E):
        h, ss = epoch(det[e], spectrum[e], merge_gap, min_width, max_segments)
        for k, v in h.items():
            eps[e][k] = v
        for j, s in enumerate(ss):
            for k, v in s.items():
                segs[e, j][k] = v
    return eps, segs


REL_TOL = 2.0 ** -22     # power, centroid, noise_mean: fp64 accumulation rounded to fp32 once, against the twin's float64 value


def compare(got_epochs, got_segments, want_epochs, want_segments):
    """The exact comparison: every integer field equal, peak_power the same bits, unused slots zero, the three fp64-accumulated
    floats within REL_TOL.  got_*: the kernel's arrays (crnsense dtypes; got_segments may be None); want_*: from run().
    Returns the largest relative error seen."""
    worst = 0.0
    for f in ("n_found", "n_stored", "noise_bins"):
        assert (got_epochs[f] == want_epochs[f]).all(), (f, np.flatnonzero(got_epochs[f] != want_epochs[f])[:8])

    def rel(got, want, what):
        nonlocal worst
        err = np.abs(got.astype(np.float64) - want) / np.maximum(np.abs(want), 1e-300)
        err = np.where(want == 0, np.where(got == 0, 0.0, np.inf), err)
        if err.size:
            worst = max(worst, float(err.max()))
        assert (err <= REL_TOL).all(), (what, float(err.max()), np.argwhere(err > REL_TOL)[:8])
    rel(got_epochs["noise_mean"], want_epochs["noise_mean"], "noise_mean")
    if got_segments is None:
        return worst
    for f in ("lo", "width", "peak_bin", "n_detected"):
        assert (got_segments[f] == want_segments[f]).all(), (f, np.argwhere(got_segments[f] != want_segments[f])[:8])
    assert (got_segments["peak_power"].view(np.uint32) == want_segments["peak_power"].astype(np.float32).view(np.uint32)).all(), "peak_power"
    assert (got_segments["reserved"].view(np.uint32) == 0).all()
    used = np.arange(got_segments.shape[1])[None, :] < want_epochs["n_stored"][:, None]
    assert not np.frombuffer(got_segments[~used].tobytes(), np.uint8).any(), "unused slots are not zero"
    rel(got_segments["power"], want_segments["power"], "power")
    rel(got_segments["centroid"], want_segments["centroid"], "centroid")
    return worst
