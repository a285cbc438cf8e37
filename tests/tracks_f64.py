"""The float64 twin of crn_tracks_device, written from the definition in include/crn_sense.h (a plain union-find over the links, numpy
for the per-member sums):

  1. nodes    the stored segments, node (e, s), s < n_stored[e]; stream e // epochs_per_stream, time t = e % epochs_per_stream.
  2. links    (e, a) and (e + d, b) of one stream, 1 <= d <= max_miss + 1, when
              ((lo_b - lo_a) mod N) < width_a + slack_bins  or  ((lo_a - lo_b) mod N) < width_b + slack_bins.
  3. tracks   the connected components; the root is the smallest node index e * max_segments + s.
  4. filter   n_epochs_hit = distinct epochs with a member; components below min_epochs are dropped; per stream the rest are numbered
              by ascending root and the first max_tracks stored, the other slots zero.
  5. stored   first_t / last_t, first_slot / last_slot (the lowest slot among the members of that epoch), n_segments, lo_off / hi_off with
              off_m = ((lo_m - lo_root + N / 2) mod N) - N / 2, width_sum, power_sum, peak_power,
              centre = (lo_root + sum(P_m (off_m + centroid_m)) / sum(P_m)) mod N, flags (bit 0: first_t <= max_miss, bit 1:
              last_t >= epochs_per_stream - 1 - max_miss).
  6. labels   track_of[e][s] = the node's track number within its stream, -1 for empty slots and members of dropped components.

`run` gives the three arrays in the kernel's layout with the float fields kept in float64."""
import numpy as np

STREAM_F64 = np.dtype([("n_found", "<i4"), ("n_stored", "<i4"), ("n_nodes", "<i4"), ("reserved", "<i4")])
TRACK_F64 = np.dtype([("first_t", "<i4"), ("last_t", "<i4"), ("first_slot", "<i4"), ("last_slot", "<i4"), ("n_epochs_hit", "<i4"),
                      ("n_segments", "<i4"), ("lo_off", "<i4"), ("hi_off", "<i4"), ("width_sum", "<i8"), ("power_sum", "<f8"),
                      ("peak_power", "<f8"), ("centre", "<f8"), ("flags", "<i4")])
INT_FIELDS = ("first_t", "last_t", "first_slot", "last_slot", "n_epochs_hit", "n_segments", "lo_off", "hi_off", "width_sum", "flags")


def linked(lo_a, w_a, lo_b, w_b, n, slack_bins):
    """Step 2's condition (scalars or broadcastable integer arrays)."""
    return ((lo_b - lo_a) % n < w_a + slack_bins) | ((lo_a - lo_b) % n < w_b + slack_bins)


def union_find(n_nodes):
    """(find, union) over the nodes 0 .. n_nodes - 1, each its own component at first; the root of a component is its smallest node."""
    parent = list(range(n_nodes))

    def find(x):
        r = x
        while parent[r] != r:
            r = parent[r]
        while parent[x] != r:
            parent[x], x = r, parent[x]
        return r

    def union(a, b):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return find, union


def components(n_stored, lo, width, n, epochs_per_stream, slack_bins, max_miss):
    """Steps 1-3: root[E][S], the root's node index for every stored node and -1 for the empty slots."""
    E, S = lo.shape
    find, union = union_find(E * S)
    for d in range(1, max_miss + 2):
        for e in range(E - d):
            na, nb = int(n_stored[e]), int(n_stored[e + d])
            if e % epochs_per_stream + d >= epochs_per_stream or na == 0 or nb == 0:
                continue
            hit = linked(lo[e, :na, None], width[e, :na, None], lo[e + d, None, :nb], width[e + d, None, :nb], n, slack_bins)
            for a, b in np.argwhere(hit):
                union(e * S + int(a), (e + d) * S + int(b))
    root = np.full((E, S), -1, np.int64)
    for e in range(E):
        for s in range(int(n_stored[e])):
            root[e, s] = find(e * S + s)
    return root


def run(epochs, segments, n, epochs_per_stream, slack_bins=1, max_miss=0, min_epochs=1, max_tracks=64, root=None):
    """epochs [E] and segments [E][S] as crn_segments_device wrote them (any dtype with the fields n_stored, lo, width, power,
    peak_power, centroid); root: what components() gave for the same lists, slack_bins and max_miss, to save the work.
    Returns (streams [n_streams] STREAM_F64, tracks [n_streams][max_tracks] TRACK_F64, track_of [E][S] int32)."""
    E, S = segments.shape
    eps = epochs_per_stream
    assert eps >= 1 and E % eps == 0
    n_streams = E // eps
    n_stored = np.clip(np.asarray(epochs["n_stored"], np.int64), 0, S)
    lo, width = segments["lo"].astype(np.int64), segments["width"].astype(np.int64)
    streams = np.zeros(n_streams, STREAM_F64)
    tracks = np.zeros((n_streams, max_tracks), TRACK_F64)
    track_of = np.full((E, S), -1, np.int32)
    streams["n_nodes"] = n_stored.reshape(n_streams, eps).sum(axis=1)
    if root is None:
        root = components(n_stored, lo, width, n, eps, slack_bins, max_miss)
    e_m, s_m = np.nonzero(root >= 0)                    # the members, ascending node index
    if e_m.size == 0:
        return streams, tracks, track_of
    roots, inv = np.unique(root[e_m, s_m], return_inverse=True)     # ascending root
    R = roots.size
    t_m = e_m % eps
    off = (lo[e_m, s_m] - lo.reshape(-1)[roots][inv] + n // 2) % n - n // 2
    P = segments["power"].astype(np.float64)[e_m, s_m]

    def reduce_at(ufunc, values, init, dtype=np.int64, sel=None):
        out = np.full(R, init, dtype)
        ufunc.at(out, inv if sel is None else inv[sel], values if sel is None else values[sel])
        return out
    big = np.iinfo(np.int64).max
    first_t, last_t = reduce_at(np.minimum, t_m, big), reduce_at(np.maximum, t_m, -1)
    first_slot = reduce_at(np.minimum, s_m, big, sel=t_m == first_t[inv])
    last_slot = reduce_at(np.minimum, s_m, big, sel=t_m == last_t[inv])
    hits = np.bincount(np.unique(inv * E + e_m) // E, minlength=R)
    nseg = np.bincount(inv, minlength=R)
    lo_off = reduce_at(np.minimum, off, big)
    hi_off = reduce_at(np.maximum, off + width[e_m, s_m] - 1, -big)
    width_sum = reduce_at(np.add, width[e_m, s_m], 0)
    power = reduce_at(np.add, P, 0.0, np.float64)
    moment = reduce_at(np.add, P * (off + segments["centroid"].astype(np.float64)[e_m, s_m]), 0.0, np.float64)
    peak = reduce_at(np.maximum, segments["peak_power"].astype(np.float64)[e_m, s_m], -np.inf, np.float64)
    centre = (lo.reshape(-1)[roots] + np.where(power > 0, moment / np.where(power > 0, power, 1.0), 0.0)) % n
    flags = (first_t <= max_miss) * 1 + (last_t >= eps - 1 - max_miss) * 2
    keep = hits >= min_epochs
    stream_of = roots // S // eps
    number = np.full(R, -1, np.int64)
    for st in range(n_streams):
        mine = np.flatnonzero(keep & (stream_of == st))
        number[mine] = np.arange(mine.size)
        streams["n_found"][st] = mine.size
        streams["n_stored"][st] = min(mine.size, max_tracks)
        for k, r in enumerate(mine[:max_tracks]):
            tr = tracks[st, k]
            for name, v in (("first_t", first_t), ("last_t", last_t), ("first_slot", first_slot), ("last_slot", last_slot), ("n_epochs_hit", hits),
                            ("n_segments", nseg), ("lo_off", lo_off), ("hi_off", hi_off), ("width_sum", width_sum), ("power_sum", power),
                            ("peak_power", peak), ("centre", centre), ("flags", flags)):
                tr[name] = v[r]
    track_of[e_m, s_m] = number[inv]
    return streams, tracks, track_of


POWER_TOL = 2.0 ** -22      # power_sum, relative: fp64 accumulation rounded to fp32 once (the bound of tests/segments_f64.py, same reason)
CENTRE_TOL = 2.0 ** -23     # centre, in units of N bins, circular: the fp32 spacing of a value below N plus the fp64 sums' error


def compare(got_streams, got_tracks, got_track_of, want_streams, want_tracks, want_track_of, n):
    """The exact comparison: headers, every integer field, flags, the labels equal; peak_power the same bits; unused slots zero;
    power_sum within POWER_TOL relative, centre within n * CENTRE_TOL bins on the circle.  got_*: the kernel's arrays (crnsense dtypes;
    got_track_of may be None), want_*: from run().  Returns (worst relative power error, worst centre error in bins)."""
    for f in ("n_found", "n_stored", "n_nodes", "reserved"):
        assert (got_streams[f] == want_streams[f]).all(), (f, np.flatnonzero(got_streams[f] != want_streams[f])[:8], got_streams[f][:8], want_streams[f][:8])
    for f in INT_FIELDS:
        assert (got_tracks[f] == want_tracks[f]).all(), (f, np.argwhere(got_tracks[f] != want_tracks[f])[:8])
    assert (got_tracks["peak_power"].view(np.uint32) == want_tracks["peak_power"].astype(np.float32).view(np.uint32)).all(), "peak_power"
    assert not got_tracks["reserved"].any()
    used = np.arange(got_tracks.shape[1])[None, :] < want_streams["n_stored"][:, None]
    assert not np.frombuffer(got_tracks[~used].tobytes(), np.uint8).any(), "unused slots are not zero"
    if got_track_of is not None:
        assert (got_track_of == want_track_of).all(), np.argwhere(got_track_of != want_track_of)[:8]
    want_p, got_p = want_tracks["power_sum"][used], got_tracks["power_sum"][used].astype(np.float64)
    perr = np.where(want_p == 0, np.where(got_p == 0, 0.0, np.inf), np.abs(got_p - want_p) / np.maximum(np.abs(want_p), 1e-300))
    assert (perr <= POWER_TOL).all(), ("power_sum", float(perr.max()))
    dc = np.abs(got_tracks["centre"][used].astype(np.float64) - want_tracks["centre"][used])
    cerr = np.minimum(dc, n - dc)
    assert (got_tracks["centre"][used] >= 0).all() and (got_tracks["centre"][used] < n).all(), "centre outside [0, N)"
    assert (cerr <= n * CENTRE_TOL).all(), ("centre", float(cerr.max()), n * CENTRE_TOL)
    return (float(perr.max()) if perr.size else 0.0), (float(cerr.max()) if cerr.size else 0.0)


def make_lists(E, S, per_epoch):
    """Hand-made input: per_epoch[e] = [(lo, width) or (lo, width, power, centroid, peak_power), ...] in the order they are stored.
    Returns (epochs, segments) as float64-field structured arrays that run() accepts (power 1, centroid (width - 1) / 2, peak 1 by
    default)."""
    eps = np.zeros(E, np.dtype([("n_found", "<i4"), ("n_stored", "<i4")]))
    segs = np.zeros((E, S), np.dtype([("lo", "<i4"), ("width", "<i4"), ("power", "<f8"), ("peak_power", "<f8"), ("centroid", "<f8")]))
    for e, lst in per_epoch.items():
        eps[e] = (len(lst), min(len(lst), S))
        for s, g in enumerate(lst[:S]):
            lo, w = g[0], g[1]
            segs[e, s] = (lo, w, g[2] if len(g) > 2 else 1.0, g[4] if len(g) > 4 else 1.0, g[3] if len(g) > 3 else (w - 1) / 2.0)
    return eps, segs
