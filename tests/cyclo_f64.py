"""crn_cyclo_device in float64, written from the definition in include/crn_sense.h ("what a segment is: the symbol rate from the cyclic
spectrum") and from nothing else: the clamps, the central max_width bins, the cells and which of them are tested, C by a DFT over the
frames, rho, S as an fp64 mean rounded to fp32 once, z in fp64 from the fp32 S, the record's order of ties and the profile.  A plain
module, not collected."""
import numpy as np

CYCLO_DTYPE = [("a", "<i4"), ("q", "<i4"), ("n_pairs", "<i4"), ("n_over", "<i4"), ("stat", "<f4"), ("stat_lo", "<f4"), ("stat_hi", "<f4"),
               ("z", "<f4")]


def span(n, lo, width, max_width):
    """(lo', w): the central w = min(width, max_width) bins of the clamped segment."""
    lo, width = int(lo) % n, min(max(int(width), 0), n)
    w = min(width, max_width)
    return (lo + (width - w) // 2) % n, w


def z_scale(frames, n_pairs):
    return np.sqrt(np.asarray(n_pairs, np.float64) * (frames + 1) / (frames - 1))


def cells(X, lo, width, a_lo, n_a, max_width, min_pairs):
    """(S [n_a][F] float32, z [n_a][F] float32, tested [n_a] bool, n_pairs [n_a]) of one segment; X [F][N] complex, the epoch's frames.
    S and z are 0 where the cell is not tested."""
    F, n = X.shape
    X = X.astype(np.complex128)
    P = (X.real ** 2 + X.imag ** 2).sum(axis=0)
    lo2, w = span(n, lo, width, max_width)
    S, z = np.zeros((n_a, F), np.float32), np.zeros((n_a, F), np.float32)
    pairs = w - (a_lo + np.arange(n_a))
    tested = pairs >= min_pairs
    for j in np.flatnonzero(tested):
        a, npairs = a_lo + int(j), int(pairs[j])
        k = (lo2 + np.arange(npairs)) % n
        k2 = (lo2 + np.arange(npairs) + a) % n
        C = np.fft.fft(X[:, k2] * np.conj(X[:, k]), axis=0)            # sum over f of . e^(-j 2 pi q f / F)
        den = P[k2] * P[k]
        rho = np.divide(C.real ** 2 + C.imag ** 2, den[None, :], out=np.zeros(C.shape), where=den[None, :] != 0)
        S[j] = (rho.sum(axis=1) / npairs).astype(np.float32)
        z[j] = ((F * S[j].astype(np.float64) - 1.0) * z_scale(F, npairs)).astype(np.float32)
    return S, z, tested, pairs


def record(S, z, tested, pairs, a_lo, z_min):
    """The 32-byte record of one segment from its cells: a tuple in CYCLO_DTYPE's order, all zero without a tested cell."""
    if not tested.any():
        return (0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0)
    zt = np.where(tested[:, None], z.astype(np.float64), -np.inf)
    j, q = np.unravel_index(int(np.argmax(zt)), zt.shape)               # the first maximum in row-major order: smallest a, then smallest q
    lo = S[j - 1, q] if j >= 1 and tested[j - 1] else np.float32(0)
    hi = S[j + 1, q] if j + 1 < S.shape[0] and tested[j + 1] else np.float32(0)
    n_over = int((zt >= np.float32(z_min)).sum())
    return (a_lo + int(j), int(q), int(pairs[j]), n_over, S[j, q], lo, hi, z[j, q])


def run(X, heads, recs, max_segments, frames, a_lo, n_a, max_width, min_pairs, z_min, want_cells=False):
    """X [E][F][N] complex; heads and recs as crn_segments_device writes them.  Returns (records [E][max_segments] CYCLO_DTYPE, profile
    [E][max_segments][n_a][F] float32) and, if asked, {(e, s): (S, z, tested, pairs)} of the stored slots."""
    E = X.shape[0]
    assert X.shape[1] == frames
    out = np.zeros((E, max_segments), np.dtype(CYCLO_DTYPE))
    prof = np.zeros((E, max_segments, n_a, frames), np.float32)
    kept = {}
    for e in range(E):
        for s in range(min(max(int(heads["n_stored"][e]), 0), max_segments)):
            c = cells(X[e], recs["lo"][e, s], recs["width"][e, s], a_lo, n_a, max_width, min_pairs)
            out[e, s] = record(*c, a_lo, z_min)
            prof[e, s] = c[0]
            if want_cells:
                kept[(e, s)] = c
    return (out, prof, kept) if want_cells else (out, prof)
