"""GO-, SO- and OS-CFAR without a GPU: the alpha helper (crn_cfar_alpha_ex) against closed forms, the F distribution and Monte Carlo,
its argument checks, and known answers of the float64 twin (tests/cfar_methods_f64.py) on the masking and clutter-edge scenarios the
detectors exist for."""
import ctypes as C
from math import comb

import numpy as np
import pytest

import cfar_methods_f64 as cm
import crnsense as cs


def alpha_ex(method, pfa, K, W, rank=0):
    a = C.c_double()
    rc = cs.lib().crn_cfar_alpha_ex(cm.METHODS[method], pfa, K, W, rank, C.byref(a))
    assert rc == 0, cs.lib().crn_last_error()
    return a.value


def pfa_so_k1(alpha, W):
    return 2 * sum(comb(W - 1 + i, i) * (2 + alpha / W) ** -(W + i) for i in range(W))


@pytest.mark.parametrize("W", [4, 16])
@pytest.mark.parametrize("pfa", [1e-2, 1e-4, 1e-6])
def test_os_k1_closed_form(built, W, pfa):
    """K = 1: P(P > alpha X_(r)) = prod_{i < r} (2W - i) / (2W - i + alpha)."""
    for r in sorted({1, W, 3 * 2 * W // 4, 2 * W}):
        a = alpha_ex("os", pfa, 1, W, r)
        got = np.prod([(2 * W - i) / (2 * W - i + a) for i in range(r)])
        assert abs(got / pfa - 1) < 1e-9, (r, a, got)


@pytest.mark.parametrize("W", [1, 4, 16, 64])
@pytest.mark.parametrize("pfa", [1e-2, 1e-4, 1e-6])
def test_go_so_k1_closed_forms(built, W, pfa):
    """K = 1: Pfa_SO = 2 sum_{i<W} C(W-1+i, i) (2 + alpha/W)^-(W+i), Pfa_GO = 2 (1 + alpha/W)^-W - Pfa_SO."""
    a = alpha_ex("so", pfa, 1, W)
    assert abs(pfa_so_k1(a, W) / pfa - 1) < 1e-9, a
    a = alpha_ex("go", pfa, 1, W)
    assert abs((2 * (1 + a / W) ** -W - pfa_so_k1(a, W)) / pfa - 1) < 1e-9, a


@pytest.mark.parametrize("K", [1, 4, 10])
def test_go_plus_so_is_twice_the_f_tail(built, K):
    """Pfa_GO(alpha) + Pfa_SO(alpha) = 2 P(F(2K, 2WK) > alpha): the SO alpha for 2 sf(alpha_GO) - Pfa_GO is alpha_GO."""
    stats = pytest.importorskip("scipy.stats")
    W = 16
    for pfa in (1e-2, 1e-4):
        a = alpha_ex("go", pfa, K, W)
        back = alpha_ex("so", 2 * stats.f.sf(a, 2 * K, 2 * W * K) - pfa, K, W)
        assert abs(back / a - 1) < 1e-9, (pfa, a, back)


def test_monte_carlo_go_and_os_k10(built):
    """K = 10, W = 16, Pfa 1e-2: the seeded tail at the returned alpha is within 5 sigma (GO: 10^6 draws, OS rank 24: 4 x 10^5)."""
    K, W, pfa = 10, 16, 1e-2
    rng = np.random.default_rng(4321)
    n = 1_000_000
    a = alpha_ex("go", pfa, K, W)
    P, L, R = rng.gamma(K, size=n), rng.gamma(W * K, size=n), rng.gamma(W * K, size=n)
    hits = int((P > a / W * np.maximum(L, R)).sum())
    assert abs(hits - n * pfa) < 5 * np.sqrt(n * pfa * (1 - pfa)), (hits, n * pfa)
    r = 24
    a = alpha_ex("os", pfa, K, W, r)
    hits, n = 0, 400_000
    for _ in range(4):
        c = rng.gamma(K, size=(n // 4, 2 * W))
        x = np.partition(c, r - 1, axis=1)[:, r - 1]
        hits += int((rng.gamma(K, size=n // 4) > a * x).sum())
    assert abs(hits - n * pfa) < 5 * np.sqrt(n * pfa * (1 - pfa)), (hits, n * pfa)


@pytest.mark.parametrize("K,W", [(1, 16), (10, 16), (10, 4)])
def test_ca_through_ex_is_crn_cfar_alpha(built, K, W):
    for pfa in (1e-1, 1e-3, 1e-6):
        assert alpha_ex("ca", pfa, K, W) == cs.cfar_alpha(pfa, K, W)


@pytest.mark.parametrize("method,rank", [("go", 0), ("so", 0), ("os", 1), ("os", 24), ("os", 32)])
def test_alpha_is_monotone_in_pfa(built, method, rank):
    a = [alpha_ex(method, p, 10, 16, rank) for p in (1e-1, 1e-2, 1e-3, 1e-4, 1e-6)]
    assert all(x < y for x, y in zip(a, a[1:])), a


def test_python_helper_defaults(built):
    """cfar_alpha(..., method="os") takes rank 3/4 of 2W by default; "ca" is crn_cfar_alpha."""
    assert cs.cfar_os_rank(16) == 24
    assert cs.cfar_alpha(1e-3, 10, 16, method="os") == alpha_ex("os", 1e-3, 10, 16, 24)
    assert cs.cfar_alpha(1e-3, 10, 16, method="go") == alpha_ex("go", 1e-3, 10, 16)
    assert cs.cfar_alpha(1e-3, 10, 16, method="ca") == cs.cfar_alpha(1e-3, 10, 16)
    with pytest.raises(ValueError):
        cs.cfar_alpha(1e-3, 10, 16, method="median")


@pytest.mark.parametrize("method,pfa,K,W,rank", [(-1, 1e-3, 10, 16, 0), (4, 1e-3, 10, 16, 0), (3, 1e-3, 10, 16, 0), (3, 1e-3, 10, 16, 33),
                                                 (1, 1e-3, 10, 16, 1), (2, 1e-3, 10, 16, -1), (1, 0.0, 10, 16, 0), (1, 1.0, 10, 16, 0),
                                                 (3, float("nan"), 10, 16, 24), (1, 1e-3, 0, 16, 0), (1, 1e-3, 10, 0, 0),
                                                 (3, 1e-3, 10, 65, 24), (0, 1e-3, 10, 16, 1)])
def test_alpha_ex_refuses_bad_arguments(built, method, pfa, K, W, rank):
    a = C.c_double()
    assert cs.lib().crn_cfar_alpha_ex(method, pfa, K, W, rank, C.byref(a)) == cs.CRN_ERR_ARG
    assert cs.lib().crn_cfar_alpha_ex(1, 1e-3, 10, 16, 0, None) == cs.CRN_ERR_ARG


N, G, W, K = 4096, 2, 16, 10


def _frames(rng, E, pw, tones):
    """K-frame sums of |X|^2 built in the frequency domain: noise of power pw per bin plus on-grid tones (bin, amplitude)."""
    X = (rng.normal(size=(E, K, N)) + 1j * rng.normal(size=(E, K, N))) * np.sqrt(pw / 2)
    for b, amp in tones:
        X[:, :, b] += amp * np.exp(2j * np.pi * rng.uniform(size=(E, K)))
    return (np.abs(X) ** 2).sum(axis=1)


def test_twin_masking(built):
    """A tone 20 dB over the floor 8 bins from one at +45 dB, Pfa 1e-6: OS (rank 24) finds both in every epoch; CA misses the weak one."""
    P = _frames(np.random.default_rng(17), 40, np.ones(N), [(1000, np.sqrt(10 ** 4.5)), (1008, 10.0)])
    d_os = cm.ratio(P, G, W, alpha_ex("os", 1e-6, K, W, 24), "os", 24) > 1
    d_ca = cm.ratio(P, G, W, cs.cfar_alpha(1e-6, K, W)) > 1
    assert d_os[:, 1000].all() and d_os[:, 1008].all()
    assert d_ca[:, 1000].all() and d_ca[:, 1008].mean() <= 0.1


def test_twin_clutter_edge(built):
    """A 10 dB step of the floor at N/2 (and back at the wrap), Pfa 1e-3: in the g + W bins on the high side of each edge GO's
    false-alarm rate stays <= 1e-2, CA's is >= 3e-2."""
    pw = np.where(np.arange(N) < N // 2, 1.0, 10.0)
    P = _frames(np.random.default_rng(23), 200, pw, [])
    hi = np.r_[N // 2:N // 2 + G + W, N - G - W:N]
    go = (cm.ratio(P, G, W, alpha_ex("go", 1e-3, K, W), "go") > 1)[:, hi].mean()
    ca = (cm.ratio(P, G, W, cs.cfar_alpha(1e-3, K, W)) > 1)[:, hi].mean()
    assert go <= 1e-2 and ca >= 3e-2, (go, ca)


def test_twin_os_count_matches_sort():
    """The fp32 counting rule equals the sorted rank-th cell wherever the float64 ratio is not within 1e-6 of 1."""
    rng = np.random.default_rng(3)
    x = rng.gamma(1.0, size=(8, 512)).astype(np.float32)
    for r in (1, 10, 24, 32):
        rr = cm.ratio(x, G, W, 7.5, "os", r)
        cnt = cm.os_count_f32(x, G, W, 7.5, r)
        far = np.abs(rr - 1) > 1e-6
        assert ((rr > 1) == cnt)[far].all()
