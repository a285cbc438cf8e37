"""The float64 twin of crn_fuse_device, written from the definition in include/crn_sense.h, bin by bin in numpy and with the same orders
of summation:

  batch       n_epochs = G M T: group j is the streams j M .. j M + M - 1, fused row j T + t comes from the epochs (j M + m) T + t
  active      member m takes part when weight[m] > 0; the others are never looked at
  fused row   F[k] = fl32( sum over the active m, ascending, of (double)w_m (double)P_m[k] )
  VOTE        fused bit k = at least `votes` active members have bit k set
  SOFT        L = sum over i = g + 1 .. g + W, ascending, of (double)F[(k - i) mod N], R the same with k + i, T = L + R;
              bin k detected <=> (double)F[k] 2W > (double)alpha T.  (A loop over i that adds rolled rows is that order.)
  header      n_detected (fused mask), n_any / n_all (bins set in any / all active members' masks, 0 without masks), n_active

`fuse` returns (fused det [G T][N] bool, fused row [G T][N] float32 or None, headers [G T] ROW)."""
import numpy as np

from mask_bits import pack_mask, unpack_mask  # noqa: F401  (one definition of the mask layout; the tests take the two names from here)

ROW = np.dtype([("n_detected", "<i4"), ("n_any", "<i4"), ("n_all", "<i4"), ("n_active", "<i4")])
VOTE, SOFT = 0, 1


def equal_gain(m):
    return [np.float32(1.0) / np.float32(m)] * m


def soft_detect(F, guard, train, alpha):
    """CA-CFAR of the definition on rows F [..][N] (fp32 values): (det, T) with T the fp64 sum of the 2 W training cells."""
    Fd = np.asarray(F, np.float32).astype(np.float64)
    L, R = np.zeros_like(Fd), np.zeros_like(Fd)
    for i in range(guard + 1, guard + train + 1):
        L += np.roll(Fd, i, axis=-1)        # element k: F[(k - i) mod N]
        R += np.roll(Fd, -i, axis=-1)
    T = L + R
    return Fd * float(2 * train) > np.float64(np.float32(alpha)) * T, T


def fuse(det, spectrum, group_size, epochs_per_stream, weights, rule, votes=0, guard=0, train=0, alpha=0.0, want_row=True):
    """det [E][N] bool or None, spectrum [E][N] float32 or None, weights one fp32 value per member."""
    M, T = int(group_size), int(epochs_per_stream)
    w = np.asarray(weights, np.float32)
    assert w.shape == (M,)
    active = [m for m in range(M) if w[m] > 0]
    E, n = (det if det is not None else spectrum).shape
    G = E // (M * T)
    assert G * M * T == E and active
    F = None
    if spectrum is not None and (want_row or rule == SOFT):
        P = np.asarray(spectrum, np.float32).reshape(G, M, T, n)
        acc = np.zeros((G, T, n), np.float64)
        for m in active:
            acc += np.float64(w[m]) * P[:, m].astype(np.float64)
        F = acc.astype(np.float32).reshape(G * T, n)
    rows = np.zeros(G * T, ROW)
    rows["n_active"] = len(active)
    if det is not None:
        d = np.asarray(det, bool).reshape(G, M, T, n)[:, active]
        count = d.sum(axis=1).reshape(G * T, n)
        rows["n_any"] = (count >= 1).sum(axis=1)
        rows["n_all"] = (count == len(active)).sum(axis=1)
    if rule == VOTE:
        fused = count >= votes
    else:
        fused = soft_detect(F, guard, train, alpha)[0]
    rows["n_detected"] = fused.sum(axis=1)
    return fused, (F if want_row else None), rows
