"""Float64 twin of the per-bin CA-CFAR detector (include/crn_sense.h, crn_sense_set_cfar), built on ref_f64.spectrum.

    Z[k]   = (1 / 2W) sum P[(k + i) mod N] over g < |i| <= g + W
    det[k] = P[k] > alpha Z[k]
    band_bins[b] = detected bins over band b's segments, occupancy[b] = band_bins[b] >= min_bins, decision = sum of occupancy
"""
import numpy as np

import ref_f64
from mask_bits import pack_mask, unpack_mask  # noqa: F401  (one definition of the mask layout; the tests take the two names from here)

WINDOWS = {0: "rect", 1: "hann", 2: "bh"}


def plan_of(cfg):
    """ref_f64.Plan of an energy-mode crn_cfg (its segments grouped by band in listing order)."""
    runs = {b: [] for b in range(cfg.n_bands)}
    for s in range(cfg.n_segs):
        g = cfg.segs[s]
        runs[g.band].append((g.lo, g.hi))
    return ref_f64.Plan(n=cfg.fft_len, k=cfg.frames_per_epoch, hop=0 if cfg.hop == cfg.fft_len else cfg.hop, mode="energy",
                        window=WINDOWS[cfg.window], runs={b: tuple(r) for b, r in runs.items()}, decide="none")


def noise_estimate(P, guard, train):
    """Z [n_epochs, N]: the mean of the 2 W training cells around every bin, circular."""
    P = np.asarray(P, np.float64)
    z = np.zeros_like(P)
    for i in range(guard + 1, guard + train + 1):
        z += np.roll(P, -i, axis=-1) + np.roll(P, i, axis=-1)
    return z / (2 * train)


def ratio(P, guard, train, alpha):
    """P / (alpha Z): > 1 is a detection."""
    return np.asarray(P, np.float64) / (alpha * noise_estimate(P, guard, train))


def band_bins(runs, det):
    out = np.zeros((det.shape[0], len(runs)), np.int64)
    for b, rr in runs.items():
        for lo, hi in rr:
            out[:, b] += det[:, lo:hi].sum(axis=1)
    return out


def decide(runs, det, min_bins):
    bb = band_bins(runs, det)
    occ = bb >= min_bins
    return bb, occ, occ.sum(axis=1)


def run(plan, iq, n_epochs, guard, train, alpha, min_bins, L=None, epoch_stride=0, P=None):
    """Every CFAR output in float64 (P: a precomputed ref_f64.spectrum)."""
    if P is None:
        P = ref_f64.spectrum(plan, iq, n_epochs, L=L, epoch_stride=epoch_stride)
    r = ratio(P, guard, train, alpha)
    det = r > 1.0
    bb, occ, dec = decide(plan.runs, det, min_bins)
    return {"spectrum": P, "ratio": r, "det": det, "band_bins": bb, "occupancy": occ, "decision": dec,
            "features": ref_f64.band_sums(plan, P)}
