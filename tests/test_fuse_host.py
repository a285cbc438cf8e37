"""Cooperative sensing without a GPU: crn_fuse_member_pfa, the refusals of crn_fuse_device that need no device, and the definition itself
(tests/fuse_f64.py, the twin) against the statistics it promises: the asked false-alarm rate with alpha = cfar_alpha(pfa, M K, W), the gain
of a group over one sensor, and the identities of the voting rule."""
import ctypes as C
from fractions import Fraction
from math import comb

import numpy as np
import pytest

import crnsense as cs
import fuse_f64 as fu

K, G_, W_, N = 10, 2, 16, 512


def _tail(p, n, k):
    """P(at least k of n) at the double p, in exact rational arithmetic."""
    p = Fraction(p)
    return float(sum(comb(n, j) * p ** j * (1 - p) ** (n - j) for j in range(k, n + 1)))


def test_member_pfa(built):
    assert cs.fuse_member_pfa(1e-3, 1, 1) == 1e-3 and cs.fuse_member_pfa(0.25, 1, 1) == 0.25
    p = 1e-3
    assert abs(cs.fuse_member_pfa(1.0 - (1.0 - p) ** 4, 4, 1) / p - 1.0) <= 1e-12
    worst = 0.0
    for n in (1, 2, 5, 32):
        for k in range(1, n + 1):
            for want in (1e-6, 1e-3, 1e-2, 0.3):
                got = _tail(cs.fuse_member_pfa(want, n, k), n, k)
                worst = max(worst, abs(got / want - 1.0))
                assert abs(got / want - 1.0) <= 1e-12, (n, k, want, got)
    print(f"round trips through the binomial tail: worst relative error {worst:.2e}")
    # majority of 8 needs a far less strict sensor than OR of 8 for the same fused rate
    assert cs.fuse_member_pfa(1e-3, 8, 1) < 1e-3 / 7.9 and cs.fuse_member_pfa(1e-3, 8, 4) > 0.05


def test_member_pfa_refusals(built):
    L = cs.lib()
    out = C.c_double(-7.0)
    for pfa, n, k in ((1e-3, 0, 1), (1e-3, 33, 1), (1e-3, 4, 0), (1e-3, 4, 5), (0.0, 4, 1), (1.0, 4, 1), (-0.1, 4, 1), (1.5, 4, 1),
                      (float("nan"), 4, 1)):
        assert L.crn_fuse_member_pfa(pfa, n, k, C.byref(out)) == cs.CRN_ERR_ARG, (pfa, n, k)
        assert b"crn_fuse_member_pfa" in L.crn_last_error() and out.value == -7.0
    assert L.crn_fuse_member_pfa(1e-3, 4, 1, None) == cs.CRN_ERR_ARG
    with pytest.raises(cs.CrnError):
        cs.fuse_member_pfa(1e-3, 4, 5)


def test_null_handle_and_params_are_refused(built):
    """Decided before any device call: this machine needs no GPU for it."""
    L = cs.lib()
    q = cs.fuse_params(cs.FUSE_VOTE, 2, 1, votes=1)
    assert C.sizeof(cs.FuseParams) == 168 and C.sizeof(cs.FuseRow) == 16 and np.dtype(cs.FUSE_ROW_DTYPE).itemsize == 16
    assert np.dtype(cs.FUSE_ROW_DTYPE) == fu.ROW
    assert list(q.weight) == [0.5, 0.5] + [0.0] * 30
    buf = C.c_void_p(4096)      # never dereferenced: both calls are refused first
    assert L.crn_fuse_device(None, buf, buf, 2, C.byref(q), buf, buf, buf, None) == cs.CRN_ERR_ARG
    assert b"crn_fuse_device" in L.crn_last_error()
    assert L.crn_fuse_device(buf, buf, buf, 2, None, buf, buf, buf, None) == cs.CRN_ERR_ARG
    assert b"crn_fuse_device" in L.crn_last_error()


def _noise(rng, M, T, scale=None):
    """M sensors x T epochs of Gamma(K) rows of mean 1 (the K-frame mean of white noise), stream after stream."""
    P = rng.gamma(K, 1.0 / K, (M, T, N))
    if scale is not None:
        P = P * scale
    return P.astype(np.float32).reshape(M * T, N)


@pytest.mark.parametrize("M", [1, 4, 8])
@pytest.mark.parametrize("pfa", [1e-2, 1e-3])
def test_twin_false_alarm_rate(built, M, pfa):
    """Noise only, equal gain, alpha = cfar_alpha(pfa, M K, W): the mean of M independent K-frame means is Gamma(M K), so the measured
    rate over 4000 x 512 bins must be the asked one, within the 15 % test_false_alarm_rate_noise_only allows for the same statistic."""
    T = 4000
    rng = np.random.default_rng(1000 * M + int(1 / pfa))
    alpha = cs.cfar_alpha(pfa, M * K, W_)
    det, _, rows = fu.fuse(None, _noise(rng, M, T), M, T, fu.equal_gain(M), fu.SOFT, guard=G_, train=W_, alpha=alpha)
    rate = det.mean()
    print(f"M={M} pfa={pfa:g}: alpha {alpha:.4f}, measured {rate:.3e} over {det.size} bins")
    assert rows["n_detected"].sum() == det.sum() and (rows["n_active"] == M).all() and not rows["n_any"].any()
    assert abs(rate / pfa - 1.0) <= 0.15, (rate, pfa)


def test_twin_cooperative_gain(built):
    """A flat 8-bin emitter at 0 dB per bin (Gaussian: the bins' K-frame means are Gamma(K) of mean 2 over a floor of mean 1), 8 sensors,
    2000 epochs, Pfa 1e-3.  One sensor finds under 0.3 of the emitter's bins, soft combining of the 8 over 0.9.  The false-alarm rates
    of the voting rules are counted on the bins the emitter cannot reach (further than guard + train from it, so that no training window
    holds one of its bins): OR of 8 within 15 % of 1 - (1 - p)^8, majority (4 of 8) below p."""
    M, T, pfa = 8, 2000, 1e-3
    rng = np.random.default_rng(8)
    band = np.arange(200, 208)
    scale = np.ones(N)
    scale[band] = 2.0
    P = _noise(rng, M, T, scale)
    a1 = cs.cfar_alpha(pfa, K, W_)
    single = fu.soft_detect(P, G_, W_, a1)[0]                                   # every sensor's own detector, [M T][N]
    soft, _, _ = fu.fuse(None, P, M, T, fu.equal_gain(M), fu.SOFT, guard=G_, train=W_, alpha=cs.cfar_alpha(pfa, M * K, W_))
    pd_single, pd_soft = single[:, band].mean(), soft[:, band].mean()
    far = np.ones(N, bool)
    far[(np.arange(band[0] - G_ - W_, band[-1] + G_ + W_ + 1)) % N] = False
    votes = {k: fu.fuse(single, None, M, T, fu.equal_gain(M), fu.VOTE, votes=k)[0] for k in (1, 4)}
    fa_single, fa_or, fa_maj, fa_soft = single[:, far].mean(), votes[1][:, far].mean(), votes[4][:, far].mean(), soft[:, far].mean()
    print(f"Pd one sensor {pd_single:.3f}, OR of 8 {votes[1][:, band].mean():.3f}, soft {pd_soft:.3f}; false alarms on {int(far.sum())} x {T} far bins: "
          f"one sensor {fa_single:.3e}, OR {fa_or:.3e} (1 - (1 - p)^8 = {1 - (1 - pfa) ** 8:.3e}), majority {fa_maj:.3e}, soft {fa_soft:.3e}")
    assert pd_single < 0.3 and pd_soft > 0.9
    assert abs(fa_or / (1.0 - (1.0 - pfa) ** M) - 1.0) <= 0.15
    assert fa_maj < pfa
    assert abs(fa_soft / pfa - 1.0) <= 0.15


def test_twin_identities(built):
    rng = np.random.default_rng(3)
    T = 5
    # one member with weight 1 under OR: the mask and the row come back bit for bit
    det = rng.random((T, N)) < 0.1
    P = _noise(rng, 1, T)
    fused, F, rows = fu.fuse(det, P, 1, T, [1.0], fu.VOTE, votes=1)
    assert (fused == det).all() and F.tobytes() == P.tobytes()
    assert (rows["n_detected"] == det.sum(axis=1)).all() and (rows["n_any"] == rows["n_all"]).all() and (rows["n_all"] == rows["n_detected"]).all()
    # a permutation of the members, with their weights, leaves the voted mask alone; n_all <= n_detected <= n_any for every k
    M = 5
    det = (rng.random((M, T, N)) < np.array([0.02, 0.3, 0.5, 0.7, 0.98])[:, None, None])
    w = rng.uniform(0.1, 2.0, M).astype(np.float32)
    w[3] = 0.0
    perm = rng.permutation(M)
    for k in range(1, 5):
        a = fu.fuse(det.reshape(M * T, N), None, M, T, w, fu.VOTE, votes=k)
        b = fu.fuse(det[perm].reshape(M * T, N), None, M, T, w[perm], fu.VOTE, votes=k)
        assert (a[0] == b[0]).all() and a[2].tobytes() == b[2].tobytes() and (a[2]["n_active"] == 4).all()
    for k in range(1, M + 1):
        rows = fu.fuse(det.reshape(M * T, N), None, M, T, fu.equal_gain(M), fu.VOTE, votes=k)[2]
        assert (rows["n_all"] <= rows["n_detected"]).all() and (rows["n_detected"] <= rows["n_any"]).all()
        if k == 1:
            assert (rows["n_detected"] == rows["n_any"]).all()
        if k == M:
            assert (rows["n_detected"] == rows["n_all"]).all()
