"""Float64 twin of the CFAR detector family (include/crn_sense.h, crn_sense_set_cfar_ex), on the definitions of cfar_f64.py.

    L[k], R[k] = means of the W cells (k - i) and (k + i) mod N, g < i <= g + W
    CA  Z = (L + R) / 2     GO  Z = max(L, R)     SO  Z = min(L, R)     OS  Z = the rank-th smallest of the 2W cells (np.sort)
    det[k] = P[k] > alpha Z[k]; band_bins, occupancy and decision as in cfar_f64.
"""
import numpy as np

import cfar_f64 as cf
import ref_f64

METHODS = {"ca": 0, "go": 1, "so": 2, "os": 3}


def cells(P, guard, train):
    """[..., N, 2W]: the left cells (distance g + W down to g + 1), then the right ones (g + 1 up to g + W), circular."""
    P = np.asarray(P, np.float64)
    left = [np.roll(P, i, axis=-1) for i in range(guard + train, guard, -1)]
    right = [np.roll(P, -i, axis=-1) for i in range(guard + 1, guard + train + 1)]
    return np.stack(left + right, axis=-1)


def noise_estimate(P, guard, train, method="ca", rank=None):
    if method == "ca":
        return cf.noise_estimate(P, guard, train)
    if method == "os":
        return np.sort(cells(P, guard, train), axis=-1)[..., rank - 1]
    P = np.asarray(P, np.float64)
    lm = sum(np.roll(P, i, axis=-1) for i in range(guard + 1, guard + train + 1)) / train
    rm = sum(np.roll(P, -i, axis=-1) for i in range(guard + 1, guard + train + 1)) / train
    return np.maximum(lm, rm) if method == "go" else np.minimum(lm, rm)


def ratio(P, guard, train, alpha, method="ca", rank=None):
    """P / (alpha Z): > 1 is a detection."""
    return np.asarray(P, np.float64) / (alpha * noise_estimate(P, guard, train, method, rank))


def os_count_f32(x, guard, train, alpha, rank):
    """OS decided as the kernel decides it, in fp32: at least `rank` cells c with fl32(alpha c) < x (x: the K-frame sums)."""
    x = np.asarray(x, np.float32)
    c = cells(x, guard, train).astype(np.float32)
    scaled = np.float32(alpha) * c
    return (scaled < x[..., None]).sum(axis=-1) >= rank


def run(plan, iq, n_epochs, guard, train, alpha, min_bins, method="ca", rank=None, L=None, epoch_stride=0, P=None):
    """Every CFAR output in float64 (P: a precomputed ref_f64.spectrum)."""
    if P is None:
        P = ref_f64.spectrum(plan, iq, n_epochs, L=L, epoch_stride=epoch_stride)
    r = ratio(P, guard, train, alpha, method, rank)
    det = r > 1.0
    bb, occ, dec = cf.decide(plan.runs, det, min_bins)
    return {"spectrum": P, "ratio": r, "det": det, "band_bins": bb, "occupancy": occ, "decision": dec,
            "features": ref_f64.band_sums(plan, P)}
