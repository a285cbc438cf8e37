"""CA-CFAR without a GPU: the alpha helper (crn_cfar_alpha) against the F distribution, its argument checks, and known answers of the
float64 twin (tests/cfar_f64.py) that the GPU tests compare the kernel with."""
import ctypes as C

import numpy as np
import pytest

import cfar_f64 as cf
import crnsense as cs


@pytest.mark.parametrize("train", [1, 4, 16, 64])
@pytest.mark.parametrize("pfa", [1e-1, 1e-3, 1e-6])
def test_alpha_k1_matches_closed_form(built, train, pfa):
    """K = 1: P / Z is F(2, 4W) and Pfa = (1 + alpha / 2W)^(-2W), so alpha = 2W (Pfa^(-1 / 2W) - 1)."""
    want = 2 * train * (pfa ** (-1.0 / (2 * train)) - 1.0)
    got = cs.cfar_alpha(pfa, 1, train)
    assert abs(got / want - 1) < 1e-9, (got, want)


@pytest.mark.parametrize("K", [4, 10])
def test_alpha_tail_of_f_distribution(built, K):
    """For K > 1 the tail of numpy's F(2K, 4WK) at alpha is the requested Pfa, within 5 sigma of 10^6 seeded draws."""
    W, pfa, n = 16, 1e-2, 1_000_000
    a = cs.cfar_alpha(pfa, K, W)
    x = np.random.default_rng(1234 + K).f(2 * K, 4 * W * K, n)
    hits = int((x > a).sum())
    sigma = np.sqrt(n * pfa * (1 - pfa))
    assert abs(hits - n * pfa) < 5 * sigma, (hits, n * pfa, sigma)


def test_alpha_is_monotone_in_pfa(built):
    a = [cs.cfar_alpha(p, 10, 16) for p in (1e-1, 1e-2, 1e-3, 1e-4, 1e-6)]
    assert all(x < y for x, y in zip(a, a[1:])), a


@pytest.mark.parametrize("pfa,K,W", [(0.0, 1, 16), (1.0, 1, 16), (-1e-3, 1, 16), (float("nan"), 1, 16), (1e-3, 0, 16),
                                     (1e-3, 1, 0), (1e-3, 1, 65)])
def test_alpha_refuses_bad_arguments(built, pfa, K, W):
    a = C.c_double()
    assert cs.lib().crn_cfar_alpha(pfa, K, W, C.byref(a)) == cs.CRN_ERR_ARG
    assert cs.lib().crn_cfar_alpha(1e-3, 1, 16, None) == cs.CRN_ERR_ARG


N, G, W = 512, 2, 16
RUNS = {0: ((0, 128),), 1: ((128, 256),), 2: ((256, 512),)}


def test_twin_tone_in_flat_noise():
    """One strong tone over flat noise: detected at its bin, not at its guard cells; the mask packs and unpacks."""
    rng = np.random.default_rng(7)
    P = rng.exponential(1.0, (4, N))
    P[:, 200] = 1e4
    alpha = 2 * W * (1e-6 ** (-1 / (2 * W)) - 1)    # K = 1, Pfa = 1e-6
    r = cf.ratio(P, G, W, alpha)
    det = r > 1
    assert det[:, 200].all()
    for d in range(1, G + 1):
        assert not det[:, 200 - d].any() and not det[:, 200 + d].any()
    bb, occ, dec = cf.decide(RUNS, det, 1)
    assert (bb[:, 1] >= 1).all() and occ[:, 1].all()
    assert (dec == occ.sum(axis=1)).all()
    assert (cf.unpack_mask(cf.pack_mask(det), N) == det).all()


def test_twin_wraps_at_dc():
    """The training cells of bin 0 are bins N-1-g.. and 1+g..: a floor raised only around the wrap still reads as the local floor."""
    P = np.ones((1, N))
    P[0, :G + W + 1] = 100.0
    P[0, N - G - W - 1:] = 100.0
    z = cf.noise_estimate(P, G, W)
    assert z[0, 0] == pytest.approx(100.0)
    P[0, 0] = 100.0 * 50
    assert (cf.ratio(P, G, W, 20.0)[0] > 1).nonzero()[0].tolist() == [0]


def test_twin_step_floor_no_false_alarms_away_from_the_step():
    """A 10 dB step in the noise floor: no false alarms more than g + W bins from either edge of the step."""
    rng = np.random.default_rng(11)
    K = 10
    floor = np.where(np.arange(N) < N // 2, 1.0, 10.0)
    P = floor * rng.gamma(K, 1.0 / K, (200, N))
    alpha = 2 * W * (1e-6 ** (-1 / (2 * W)) - 1)    # K = 1's alpha: conservative at K = 10
    det = cf.ratio(P, G, W, alpha) > 1
    k = np.arange(N)
    dist = np.minimum.reduce([np.abs(k - N // 2), np.abs(k - N), k])
    assert not det[:, dist > G + W].any()

