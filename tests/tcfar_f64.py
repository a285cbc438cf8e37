"""Twin of crn_tcfar_device (include/crn_sense.h, "ordered-statistic CFAR along time, per bin"), written from the header's text: it walks
a stream epoch by epoch with an explicit ring of H = cells + guard_epochs rows, the row of global epoch n in slot n mod H.

    n = seen + t;  for n >= H the cells of (n, k) are P_(n-g-i)[k], i = 1..D;  det <=> at least `rank` cells with fl32(alpha c) < P_n[k]
    out = det | or_mask;  header: n_detected = bits of out, n_new = bits of det not in or_mask, n_cells = D (0 while n < H)

The rule is an fp32 product and an fp32 compare, which numpy's float32 makes exactly: there is no rounding freedom, and the GPU tests
compare every bin byte for byte.  brute() restates the rule on a whole stream without a ring, for the host test to hold run() against.
The name follows the other twins'; nothing here needs float64."""
import numpy as np

from mask_bits import pack_mask, unpack_mask  # noqa: F401  (one definition of the mask layout; the tests take the two names from here)

ROW_DTYPE = [("n_detected", "<i4"), ("n_new", "<i4"), ("n_cells", "<i4"), ("reserved", "<i4")]
SEEN_MAX = 2 ** 62


def new_state(n_streams, n, cells, guard, fill=0.0):
    """(hist [S, H, N] float32, seen [S] int64) as a caller allocates them; `fill` is what the untouched slots hold."""
    return np.full((n_streams, cells + guard, n), fill, np.float32), np.zeros(n_streams, np.int64)


def run_ranks(P, eps, cells, guard, ranks, alpha, hist, seen, first, or_mask=None):
    """One call, decided for every rank of `ranks` from one count: the rows P [S eps, N] of S streams in time order; hist and seen are the
    caller's carry and are updated in place.  Returns {rank: (mask [S eps, N] bool, rows [S eps] ROW_DTYPE)}."""
    P = np.asarray(P, np.float32)
    e_n, n = P.shape
    d, g, h = int(cells), int(guard), int(cells) + int(guard)
    assert e_n % eps == 0 and hist.shape == (e_n // eps, h, n) and hist.dtype == np.float32 and seen.dtype == np.int64
    a = np.float32(alpha)
    scaled = a * hist                                            # float32 x float32: fl32(alpha c), kept beside the ring
    assert scaled.dtype == np.float32
    out = {r: (np.zeros((e_n, n), bool), np.zeros(e_n, ROW_DTYPE)) for r in ranks}
    for s in range(e_n // eps):
        start = 0 if first else min(max(int(seen[s]), 0), SEEN_MAX)
        for t in range(eps):
            e = s * eps + t
            gl = start + t
            row = P[e]
            om = np.zeros(n, bool) if or_mask is None else np.asarray(or_mask[e], bool)
            below = None
            if gl >= h:
                lo = (gl - g - d) % h                            # the cells' slots (gl - g - i) mod h, i = d .. 1, are consecutive around the ring
                below = (scaled[s, lo: lo + d] < row[None, :]).sum(axis=0)
                if lo + d > h:
                    below += (scaled[s, : lo + d - h] < row[None, :]).sum(axis=0)
            for r, (mask, rows) in out.items():
                det = below >= r if below is not None else np.zeros(n, bool)
                mask[e] = det | om
                rows[e] = (mask[e].sum(), (det & ~om).sum(), d if below is not None else 0, 0)
            hist[s, gl % h] = row                                # the slot of epoch gl - h, whose row was a cell for the last time just now
            scaled[s, gl % h] = a * row
        seen[s] = start + eps
    return out


def run(P, eps, cells, guard, rank, alpha, hist, seen, first, or_mask=None):
    """run_ranks for one rank: (mask, rows)."""
    return run_ranks(P, eps, cells, guard, [rank], alpha, hist, seen, first, or_mask)[rank]


def brute(stream_rows, cells, guard, rank, alpha):
    """The header's rule on one whole stream [T, N] from epoch 0, without a ring: det [T, N] bool."""
    P = np.asarray(stream_rows, np.float32)
    a = np.float32(alpha)
    det = np.zeros(P.shape, bool)
    for gl in range(cells + guard, P.shape[0]):
        for k in range(P.shape[1]):
            below = 0
            for i in range(1, cells + 1):
                below += bool(np.float32(a * P[gl - guard - i, k]) < P[gl, k])
            det[gl, k] = below >= rank
    return det


def written_slots(seen_after, cells, guard):
    """The slots of one stream's ring that hold rows after a call: those of the last min(H, seen) epochs."""
    h = cells + guard
    return sorted({gl % h for gl in range(max(0, int(seen_after) - h), int(seen_after))})

