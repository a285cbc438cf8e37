"""crn_measure_device as include/crn_sense.h states it, with plain loops and Python integers: the twin of csrc/crn_measure.hip.  fp32
operations are numpy float32 scalars (one operation, one rounding); every sum is a Python int."""
import math

import numpy as np

MEASURE_DTYPE = [("obw_lo", "<i4"), ("obw_width", "<i4"), ("xdb_lo", "<i4"), ("xdb_width", "<i4"), ("n_above", "<i4"), ("net_power", "<f4"),
                 ("crest", "<f4"), ("reserved", "<f4")]
F32 = np.float32
QMAX = 2 ** 31 - 1


def exponent(peak):
    """e with 2^e <= peak < 2^(e+1), peak finite and > 0 (a subnormal fp32 is a normal Python float)."""
    return math.frexp(float(peak))[1] - 1


def integers(row, n, lo, width, nm, e):
    """(Q [width] float32, q [width] Python ints): steps 2 and 3."""
    Q, q = [], []
    with np.errstate(all="ignore"):
        for i in range(width):
            x = F32(row[(lo + i) % n]) - F32(nm)
            Q.append(x)
            if not x > 0:
                q.append(0)
            elif math.isinf(float(x)):
                q.append(QMAX)
            else:
                q.append(min(int(math.trunc(float(x) * 2.0 ** (30 - e))), QMAX))
    return Q, q


def segment(row, n, lo, width, peak, nm, tail_ppm, ratio):
    """One record as a tuple in MEASURE_DTYPE's order, or None where there is nothing to measure (step 7)."""
    lo, width, peak = int(lo), int(width), F32(peak)
    if not 0 <= lo <= n - 1 or not 1 <= width <= n or not math.isfinite(float(peak)) or not peak > 0:
        return None
    with np.errstate(all="ignore"):
        pq = peak - F32(nm)
        if not pq > 0:
            return None
        thr = F32(ratio) * pq
    e = exponent(peak)
    Q, q = integers(row, n, lo, width, nm, e)
    S0 = 0
    for x in q:
        S0 += x
    if S0 == 0:
        return None
    T = (S0 * int(tail_ppm)) // 10 ** 6
    C, obw_lo = 0, None
    for i in range(width):
        C += q[i]
        if C > T:
            obw_lo = i
            break
    C, last = 0, None                       # C[i - 1]
    for i in range(width):
        if S0 - C > T:
            last = i
        C += q[i]
    above = [i for i in range(width) if Q[i] > thr]
    xdb_lo, xdb_width = (above[0], above[-1] - above[0] + 1) if above else (0, 0)
    net_power = F32(float(S0) * 2.0 ** (e - 30))
    crest = F32(float(max(q) * width) / float(S0))
    return obw_lo, last - obw_lo + 1, xdb_lo, xdb_width, len(above), net_power, crest, F32(0)


def run(P, epochs, segments, max_segments, tail_ppm, ratio, subtract_noise):
    """[E][max_segments] MEASURE_DTYPE from the rows P [E][N] float32, the headers [E] and the records [E][max_segments] as
    crn_segments_device writes them (numpy structured arrays)."""
    E, n = P.shape
    out = np.zeros((E, max_segments), np.dtype(MEASURE_DTYPE))
    ratio = F32(ratio)
    for e in range(E):
        nm = F32(epochs["noise_mean"][e])
        if not (subtract_noise and math.isfinite(float(nm)) and nm > 0):
            nm = F32(0)
        for s in range(min(max(int(epochs["n_stored"][e]), 0), max_segments)):
            g = segments[e, s]
            r = segment(P[e], n, g["lo"], g["width"], g["peak_power"], nm, tail_ppm, ratio)
            if r is not None:
                out[e, s] = r
    return out
