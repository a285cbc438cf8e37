"""Float64 twin of crn_lad_device (include/crn_sense.h, "wideband detection against an excised noise floor"), written from the header's
text by the sorted forward search; the kernel finds the same floor without a sort, which fixed_point() restates in numpy so that the
host test can hold the two against each other.

    per block of M = N / n_blocks bins:  x_(1) <= .. <= x_(M), C_n = sum of x_(i) over i <= n (float64, ascending),
        n0 = max(1, M init_percent / 100), n* = the smallest n in n0 .. M with n == M or x_(n+1) n > t_cme C_n, floor = C_n* / n*
    lower[k] = P[k] n* > t_lower C_n*, upper[k] likewise with t_upper
    det = the union of the maximal circular runs of `lower` that hold an `upper` bin;  out = det | or_mask

run() also reports, per row, the smallest |lhs / rhs - 1| over every comparison it made: the header calls a row decided when that is
above 2^-36, and only decided rows are compared byte for byte.  A comparison whose two sides are both 0 is exact in any order of
summation and counts as decided.  factor() and excised_mean() restate crn_lad_factor with an incomplete gamma function of their own."""
import math

import numpy as np

from mask_bits import pack_mask, unpack_mask  # noqa: F401  (one definition of the mask layout; the tests take the two names from here)

ROW_DTYPE = [("n_lower", "<i4"), ("n_upper", "<i4"), ("n_detected", "<i4"), ("n_clusters", "<i4"), ("n_rejected", "<i4"), ("n_clean", "<i4"),
             ("floor_min", "<f4"), ("floor_max", "<f4")]
ROW_INTS = ("n_lower", "n_upper", "n_detected", "n_clusters", "n_rejected", "n_clean")
DECIDED = 2.0 ** -36


def _margin(lhs, rhs):
    """The smallest |lhs / rhs - 1|; a pair of zeros, and a zero rhs under a positive lhs, are as decided as can be."""
    lhs, rhs = np.atleast_1d(lhs), np.atleast_1d(rhs)
    ok = rhs != 0
    if not ok.any():
        return np.inf
    return float(np.abs(lhs[ok] / rhs[ok] - 1.0).min())


def n0_of(m, init_percent):
    return max(1, m * init_percent // 100)


def floor_of(block, init_percent, t_cme):
    """(n*, C_n*, margin) of one block by the forward search on the sorted values."""
    xs = np.sort(np.asarray(block, np.float32)).astype(np.float64)
    m = xs.size
    cs = np.cumsum(xs)                                   # cs[n - 1] = C_n, added in ascending order
    n0 = n0_of(m, init_percent)
    n = np.arange(n0, m)                                 # the comparisons at n = n0 .. M - 1 look at x_(n+1) = xs[n]
    lhs, rhs = xs[n] * n, np.float64(np.float32(t_cme)) * cs[n - 1]
    stop = lhs > rhs
    if stop.any():
        j = int(np.argmax(stop))
        return n0 + j, cs[n0 + j - 1], _margin(lhs[: j + 1], rhs[: j + 1])
    return m, cs[m - 1], _margin(lhs, rhs)


def fixed_point(block, init_percent, t_cme):
    """(n*, passes) by the iteration the kernel runs: from the n0 smallest values, take every value with x n <= t_cme C, until the
    set no longer grows.  No sort is needed for it; one is used here only to pick the n0 smallest."""
    x = np.asarray(block, np.float32).astype(np.float64)
    m = x.size
    n = n0_of(m, init_percent)
    c = np.sort(x)[:n].sum()
    t = np.float64(np.float32(t_cme))
    passes = 0
    while n < m:
        passes += 1
        take = ~(x * n > t * c)
        if take.sum() <= n:
            break
        n, c = int(take.sum()), x[take].sum()
    return n, passes


def clusters(lower, upper):
    """(det, kept, rejected) of one row: the circular runs of `lower`, kept where they hold an `upper` bin."""
    n = lower.size
    if lower.all():
        kept = bool(upper.any())
        return (np.ones(n, bool) if kept else np.zeros(n, bool)), int(kept), int(not kept)
    if not lower.any():
        return np.zeros(n, bool), 0, 0
    z = int(np.flatnonzero(~lower)[0])                   # cut the circle at a zero
    lw, up = np.roll(lower, -z), np.roll(upper & lower, -z)
    d = np.diff(np.concatenate(([0], lw.astype(np.int8), [0])))
    starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
    cu = np.concatenate(([0], np.cumsum(up)))
    has = cu[ends] > cu[starts]
    mark = np.zeros(n + 1, np.int64)
    np.add.at(mark, starts[has], 1)
    np.add.at(mark, ends[has], -1)
    return np.roll(np.cumsum(mark)[:n] > 0, z), int(has.sum()), int((~has).sum())


def run(P, n_blocks, init_percent, t_cme, t_lower, t_upper, or_mask=None):
    """(mask [E, N] bool, rows [E] ROW_DTYPE, floors [E, n_blocks] float32, margin [E]) for the rows P [E, N]."""
    P = np.asarray(P, np.float32)
    e_n, n = P.shape
    m = n // n_blocks
    tl, tu = np.float64(np.float32(t_lower)), np.float64(np.float32(t_upper))
    mask = np.zeros((e_n, n), bool)
    rows = np.zeros(e_n, ROW_DTYPE)
    floors = np.zeros((e_n, n_blocks), np.float32)
    margin = np.full(e_n, np.inf)
    for e in range(e_n):
        lower, upper = np.zeros(n, bool), np.zeros(n, bool)
        clean = 0
        for b in range(n_blocks):
            blk = P[e, b * m: (b + 1) * m]
            ns, c, mg = floor_of(blk, init_percent, t_cme)
            floors[e, b] = np.float32(c / ns)
            lhs = blk.astype(np.float64) * ns
            lower[b * m: (b + 1) * m] = lhs > tl * c
            upper[b * m: (b + 1) * m] = lhs > tu * c
            margin[e] = min(margin[e], mg, _margin(lhs, np.full(m, tl * c)), _margin(lhs, np.full(m, tu * c)))
            clean += ns
        det, kept, rejected = clusters(lower, upper)
        mask[e] = det if or_mask is None else det | np.asarray(or_mask[e], bool)
        rows[e] = (lower.sum(), upper.sum(), mask[e].sum(), kept, rejected, clean, floors[e].min(), floors[e].max())
    return mask, rows, floors, margin


def compare(got_mask, got_rows, got_floors, want, what="", max_undecided=1):
    """The kernel's outputs against run()'s on the decided rows, byte for byte; either of the three may be None.  Returns the number of
    undecided rows, which it skips; more than max_undecided is a failure of the test's own inputs."""
    w_mask, w_rows, w_floors, margin = want
    ok = margin > DECIDED
    assert (~ok).sum() <= max_undecided, (what, "undecided rows", np.flatnonzero(~ok)[:8], margin[~ok][:8])
    if got_mask is not None:
        bad = np.flatnonzero((np.asarray(got_mask, np.uint32) != pack_mask(w_mask)).any(axis=1) & ok)
        assert bad.size == 0, (what, "mask, rows", bad[:8])
    if got_rows is not None:
        for f in ROW_INTS:
            bad = np.flatnonzero((got_rows[f] != w_rows[f]) & ok)
            assert bad.size == 0, (what, f, bad[:8], got_rows[f][bad[:8]], w_rows[f][bad[:8]])
        for f in ("floor_min", "floor_max"):
            bad = np.flatnonzero((got_rows[f].view(np.uint32) != w_rows[f].view(np.uint32)) & ok)
            assert bad.size == 0, (what, f, bad[:8], got_rows[f][bad[:8]], w_rows[f][bad[:8]])
    if got_floors is not None:
        bad = np.flatnonzero((np.asarray(got_floors, np.float32).view(np.uint32) != w_floors.view(np.uint32)).any(axis=1) & ok)
        assert bad.size == 0, (what, "d_floor, rows", bad[:8])
    return int((~ok).sum())


# -- crn_lad_factor restated -----------------------------------------------------------------------------------------------------

def gamma_p(a, x):
    """The regularised lower incomplete gamma P(a, x) by its power series (every term positive; fine for the x / a met here)."""
    if x <= 0.0:
        return 0.0
    term = total = 1.0 / a
    k = a
    for _ in range(100000):
        k += 1.0
        term *= x / k
        total += term
        if term < 1e-18 * total:
            break
    return total * math.exp(a * math.log(x) - x - math.lgamma(a))


def quantile(k, pfa):
    """G_K^-1(1 - pfa) of the unit-scale Gamma(K) law, by bisection on 1 - P(K, q) = pfa."""
    lo, hi = 0.0, 1.0
    while 1.0 - gamma_p(k, hi) > pfa:
        lo, hi = hi, 2.0 * hi
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if 1.0 - gamma_p(k, mid) > pfa:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def excised_mean(k, t_cme):
    """The mean FCME converges to in Gamma(K) noise of mean 1: the fixed point of m = P(K + 1, K t m) / P(K, K t m) from m = 1."""
    m = 1.0
    for _ in range(10000):
        nxt = gamma_p(k + 1.0, k * t_cme * m) / gamma_p(k, k * t_cme * m)
        if abs(nxt - m) <= 1e-16 * m:
            return nxt
        m = nxt
    return m


def factor(pfa, k, t_cme=0.0):
    return quantile(k, pfa) / k / (excised_mean(k, t_cme) if t_cme > 0.0 else 1.0)
