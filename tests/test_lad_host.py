"""crn_lad_device on the host: the twin (tests/lad_f64.py) by hand, the kernel's fixed point against the sorted forward search, the C ABI
and crn_lad_factor without a GPU, and the two simulations that state what the design claims (DESIGN.md §5 quotes their printed numbers):
the false-alarm rate in noise, and the emitter bins per-bin CA-CFAR and this detector see of a band-filling emitter."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import cfar_f64
import crnsense as cs
import lad_cases as lc
import lad_f64 as lf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q10 = lc.params(10)


def _one(row, n_blocks=1, init_percent=10, or_mask=None, **q):
    q = {**Q10, **q}
    mask, rows, floors, margin = lf.run(np.asarray(row, np.float32)[None, :], n_blocks, init_percent, q["t_cme"], q["t_lower"], q["t_upper"],
                                        or_mask=None if or_mask is None else or_mask[None, :])
    return mask[0], rows[0], floors[0], margin[0]


# ---- the twin by hand -----------------------------------------------------------------------------------------------------------
def test_all_equal_and_all_zero_rows():
    for n_blocks in (1, 2):
        mask, r, floors, margin = _one(np.full(512, 2.5), n_blocks)
        assert not mask.any() and r["n_clean"] == 512 and r["n_lower"] == 0 and r["n_clusters"] == 0 and (floors == 2.5).all()
        assert margin > lf.DECIDED
        mask, r, floors, margin = _one(np.zeros(512), n_blocks)
        assert not mask.any() and r["n_clean"] == 512 and r["n_detected"] == 0 and (floors == 0).all() and r["floor_max"] == 0
        assert margin > lf.DECIDED                           # 0 > 0 is exact in any order of summation


def test_one_cluster_across_the_wrap():
    p = np.ones(512)
    p[[509, 510, 511, 0, 1]] = 3.0                            # over both thresholds
    mask, r, floors, _ = _one(p)
    assert sorted(np.flatnonzero(mask)) == [0, 1, 509, 510, 511]
    assert (r["n_clusters"], r["n_rejected"], r["n_lower"], r["n_upper"], r["n_detected"], r["n_clean"]) == (1, 0, 5, 5, 5, 507)
    assert floors[0] == 1.0 and r["floor_min"] == r["floor_max"] == 1.0


def test_a_cluster_across_a_block_edge_with_two_floors():
    p = np.ones(512)
    p[256:] = 4.0                                             # the second block's floor is four times the first's
    p[250:256] = 2.2                                          # lower only against the floor 1
    p[256:260] = 12.0                                         # upper against the floor 4
    mask, r, floors, _ = _one(p, n_blocks=2)
    assert list(floors) == [1.0, 4.0] and (r["floor_min"], r["floor_max"]) == (1.0, 4.0)
    assert sorted(np.flatnonzero(mask)) == list(range(250, 260)) and (r["n_clusters"], r["n_rejected"]) == (1, 0)
    assert (r["n_lower"], r["n_upper"], r["n_clean"]) == (10, 4, 250 + 252)
    # with one floor for the row the 4.0 half is itself over the thresholds
    mask1, r1, _, _ = _one(p, n_blocks=1)
    assert mask1[256:].all() and r1["n_clean"] == 250


def test_a_lower_run_without_an_upper_bin_is_rejected_and_counted():
    p = np.ones(512)
    p[100:104] = 2.2                                          # between the thresholds: 1.90 and 2.65 times the floor
    p[105:108] = 2.2
    p[106] = 3.0
    mask, r, _, _ = _one(p)
    assert sorted(np.flatnonzero(mask)) == [105, 106, 107]
    assert (r["n_clusters"], r["n_rejected"], r["n_lower"], r["n_upper"], r["n_detected"]) == (1, 1, 7, 1, 3)


def test_lower_all_ones_is_one_cluster_of_width_n():
    p = np.ones(512)
    p[300] = 2.0
    q = {"t_cme": 4.0, "t_lower": 0.5, "t_upper": 1.5}       # every bin is over half the floor
    mask, r, _, _ = _one(p, **q)
    assert mask.all() and (r["n_clusters"], r["n_rejected"], r["n_lower"], r["n_upper"], r["n_detected"]) == (1, 0, 512, 1, 512)
    p[300] = 1.0
    mask, r, _, _ = _one(p, **q)
    assert not mask.any() and (r["n_clusters"], r["n_rejected"], r["n_lower"], r["n_upper"]) == (0, 1, 512, 0)


def test_or_mask():
    p = np.ones(512)
    p[40:44] = 3.0
    om = np.zeros(512, bool)
    om[[7, 41, 511]] = True
    mask, r, _, _ = _one(p, or_mask=om)
    assert sorted(np.flatnonzero(mask)) == [7, 40, 41, 42, 43, 511]
    assert r["n_detected"] == 6 and r["n_lower"] == 4 and r["n_clusters"] == 1


def test_init_percent_1_and_50():
    rng = np.random.default_rng(3)
    p = rng.gamma(10.0, 0.1, 512)
    assert lf.n0_of(512, 1) == 5 and lf.n0_of(512, 50) == 256 and lf.n0_of(256, 1) == 2 and lf.n0_of(64, 1) == 1
    a, b = _one(p, init_percent=1), _one(p, init_percent=50)
    assert a[1]["n_clean"] == b[1]["n_clean"] > 256          # both walk on to the same stop in noise
    # more than half of the row under an emitter: from 50 % the search starts on the emitter's own bins and goes on
    p[: 512 * 6 // 10] += 20.0
    assert _one(p, init_percent=1)[1]["n_clean"] <= 512 * 4 // 10 < _one(p, init_percent=50)[1]["n_clean"]
    # a t_cme under 1 stops the search where it starts
    assert _one(p, init_percent=10, t_cme=0.5)[1]["n_clean"] == 51


def test_fixed_point_equals_forward_search():
    """The iteration the kernel runs against the sorted search: equal n* on random rows with emitters of random width and level."""
    rng = np.random.default_rng(11)
    most, total, rows = 0, 0, 0
    for it in range(300):
        m = int(rng.choice([256, 512, 1024, 4096]))
        k = int(rng.choice([1, 10]))
        x = rng.gamma(k, 1.0 / k, m)
        for _ in range(int(rng.integers(0, 4))):
            w, lo = int(rng.integers(1, m)), int(rng.integers(0, m))
            x[(lo + np.arange(w)) % m] += 10.0 ** rng.uniform(-1.0, 4.0) * rng.gamma(k, 1.0 / k, w)
        if it % 10 == 0:
            x = np.round(x * 4.0) / 4.0                        # ties
        x = x.astype(np.float32)
        ip = int(rng.choice([1, 10, 50]))
        t = float(rng.choice([lf.factor(1e-2, k), lf.factor(1e-3, k), 0.7, 1.0, 1.3]))
        n_fwd, _, margin = lf.floor_of(x, ip, t)
        n_fix, passes = lf.fixed_point(x, ip, t)
        if margin > lf.DECIDED:
            assert n_fix == n_fwd, (it, m, k, ip, t, n_fix, n_fwd)
            most, total, rows = max(most, passes), total + passes, rows + 1
    print(f"fixed point against forward search: {rows} decided rows, 0 differences, {total / rows:.1f} passes on average, {most} at most")


def test_the_gpu_tests_rows_are_decided():
    """tests/test_lad_gpu.py compares decided rows only and allows itself one undecided row per test: its synthetic rows have none."""
    for n in lc.SIZES:
        P, names = lc.batch(n)
        for n_blocks in lc.blocks_allowed(n):
            for ip in lc.INIT_PERCENTS:
                margin = lf.run(P, n_blocks, ip, **Q10)[3]
                assert (margin > lf.DECIDED).all(), (n, n_blocks, ip, [names[i] for i in np.flatnonzero(margin <= lf.DECIDED)])


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_structures_and_binding(built):
    L = cs.lib()
    for name in ("crn_lad_device", "crn_lad_factor"):
        assert name in cs.EXPORTS and hasattr(L, name)
    assert C.sizeof(cs.LadParams) == 32 and np.dtype(cs.LAD_ROW_DTYPE).itemsize == 32
    assert cs.LAD_ROW_DTYPE == lf.ROW_DTYPE
    hdr = open(os.path.join(ROOT, "include", "crn_sense.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip()
                for f in re.sub(r"^\s*(int32_t|float)\s", "", decl.strip()).split(",")]
    assert fields("crn_lad_params") == [f[0] for f in cs.LadParams._fields_]
    assert fields("crn_lad_row") == [f[0] for f in cs.LAD_ROW_DTYPE]
    assert "/* 32 bytes */" in hdr[hdr.index("} crn_lad_params;"):][:40] and "/* 32 bytes */" in hdr[hdr.index("} crn_lad_row;"):][:40]
    assert callable(cs.Sensor.lad_device)
    assert L.crn_abi_version() == cs.CRN_ABI_VERSION == 4     # additive: the ABI version stays
    # the engine directory's copy of the header is the header
    assert open(os.path.join(ROOT, "cognitive-radio-network_amd", "cognitive_engines", "CE_Predictive_Node_GPU", "crn_sense.h")).read() == hdr


def test_no_handle_is_refused_before_anything_is_looked_at(built):
    L = cs.lib()
    q = cs.lad_params(1, 10, **Q10)
    buf = (C.c_uint8 * 65536)()
    p = (C.addressof(buf) + 63) & ~63
    assert L.crn_lad_device(None, p, 8, C.byref(q), p, p, p, p, None) == cs.CRN_ERR_ARG
    assert b"crn_lad_device" in L.crn_last_error()
    assert L.crn_lad_device(None, p, 0, C.byref(q), None, p, None, None, None) == cs.CRN_ERR_ARG
    assert L.crn_lad_device(None, None, -1, None, None, None, None, None, None) == cs.CRN_ERR_ARG
    assert not bytes(buf).strip(b"\0")


def test_lad_factor_refusals(built):
    L = cs.lib()
    f = C.c_double(-7.0)
    assert L.crn_lad_factor(1e-3, 10, 0.0, C.byref(f)) == 0 and f.value > 1.0
    f.value = -7.0
    for pfa, k, t in ((0.0, 10, 0.0), (1.0, 10, 0.0), (-1e-3, 10, 0.0), (1.5, 10, 0.0), (math.nan, 10, 0.0), (1e-3, 0, 0.0), (1e-3, -1, 0.0),
                      (1e-3, 10, -1.0), (1e-3, 10, math.inf), (1e-3, 10, math.nan)):
        assert L.crn_lad_factor(pfa, k, t, C.byref(f)) == cs.CRN_ERR_ARG, (pfa, k, t)
        assert b"crn_lad_factor" in L.crn_last_error() and f.value == -7.0
    assert L.crn_lad_factor(1e-3, 10, 0.0, None) == cs.CRN_ERR_ARG
    with pytest.raises(cs.CrnError):
        cs.lad_factor(2.0, 10)


# scipy's answers (the issue's table): (K, pfa, t_cme, factor)
KNOWN = [(10, 1e-2, 0.0, 1.8783117393), (10, 1e-3, 0.0, 2.2657373309), (10, 1e-4, 0.0, 2.6192986637), (10, 1e-3, 1.8783117393, 2.2926711714),
         (1, 1e-3, 4.605170186, 7.3273132457)]
KNOWN_MEAN = [(10, 1.8783117393, 0.9882522008), (1, 4.605170186, 0.9427405445)]


def test_lad_factor_known_answers(built):
    for k, pfa, t, want in KNOWN:
        assert abs(cs.lad_factor(pfa, k, t) - want) < 1e-9, (k, pfa, t, cs.lad_factor(pfa, k, t))
        assert abs(lf.factor(pfa, k, t) - want) < 1e-9, (k, pfa, t, lf.factor(pfa, k, t))
    for pfa in (0.5, 1e-2, 1e-3, 1e-6):
        assert abs(cs.lad_factor(pfa, 1) + math.log(pfa)) < 1e-9 * -math.log(pfa)
    for k, t, want in KNOWN_MEAN:
        assert abs(lf.excised_mean(k, t) - want) < 1e-9
        # the library's m is the ratio of its two factors
        assert abs(cs.lad_factor(1e-3, k, 0.0) / cs.lad_factor(1e-3, k, t) - want) < 1e-9
    # the twin's restatement over a wider range
    for k in (1, 2, 10, 40):
        for pfa in (1e-1, 1e-2, 1e-4):
            t = cs.lad_factor(pfa, k)
            assert abs(t / lf.factor(pfa, k) - 1) < 1e-9
            for p2 in (1e-2, 1e-5):
                assert abs(cs.lad_factor(p2, k, t) / lf.factor(p2, k, t) - 1) < 1e-9, (k, pfa, p2)


# ---- the simulations ------------------------------------------------------------------------------------------------------------
def _rate(rng, k, m, rows, pfa_cme, pfa_lower, pfa_upper, corrected=True):
    t = lf.factor(pfa_cme, k)
    tl, tu = lf.factor(pfa_lower, k, t if corrected else 0.0), lf.factor(pfa_upper, k, t if corrected else 0.0)
    P = rng.gamma(float(k), 1.0 / k, (rows, m)).astype(np.float32)
    mask, r, _, _ = lf.run(P, 1, 10, t, tl, tu)
    return mask.sum() / mask.size, r["n_clean"].mean() / m


def test_false_alarm_rate_in_noise():
    """Noise only, M = 4096, one threshold at 1e-3 over an FCME at 1e-2: the rate lies within 10 % of 1e-3 for K = 1 and K = 10 (the
    binomial sigma over 1.6 million bins is 2.5 %).  Smaller blocks, the uncorrected factor and the double threshold are printed."""
    rng = np.random.default_rng(2024)
    for k in (1, 10):
        rate, clean = _rate(rng, k, 4096, 400, 1e-2, 1e-3, 1e-3)
        print(f"noise only, M = 4096, K = {k}: FCME at 1e-2 keeps {clean:.4f} of the bins; rate at 1e-3 {rate:.3e} over {400 * 4096} bins")
        assert 0.9e-3 <= rate <= 1.1e-3, (k, rate)
    for k in (1, 10):
        for m in (64, 256, 1024, 4096):
            rows = 1600000 // m // 4
            single, _ = _rate(rng, k, m, rows, 1e-2, 1e-3, 1e-3)
            plain, _ = _rate(rng, k, m, rows, 1e-2, 1e-3, 1e-3, corrected=False)
            double, _ = _rate(rng, k, m, rows, 1e-2, 1e-2, 1e-4)
            print(f"K = {k:2d}, M = {m:4d}: rate at 1e-3 {single:.2e} (factor not corrected for the excision: {plain:.2e}); "
                  f"double threshold (1e-2, 1e-4) {double:.2e}")


EMITTERS = ((512, 30), (4096, 240))
DBS = (0, 3, 6, 10)


def test_band_filling_emitter_cfar_against_lad(built):
    """A flat emitter of the reference transmitters' widths over Gamma(10) noise, 200 rows: the fraction of its bins that CA-CFAR (guard
    2, train 16, Pfa 1e-3) and this detector (FCME and lower at 1e-2, upper at 1e-4, one block) set.  The end-to-end GPU test takes its
    bars from here: at +10 dB CFAR sees at most 0.2 of the emitter, LAD at least 0.98."""
    k, rows = 10, 200
    alpha = cs.cfar_alpha(1e-3, k, 16)
    rng = np.random.default_rng(77)
    for n, width in EMITTERS:
        lo = n // 3
        line = []
        for db in DBS:
            P = rng.gamma(float(k), 1.0 / k, (rows, n))
            P[:, lo: lo + width] += 10.0 ** (db / 10.0) * rng.gamma(float(k), 1.0 / k, (rows, width))
            P = P.astype(np.float32)
            cfar = (cfar_f64.ratio(P, 2, 16, alpha) > 1.0)[:, lo: lo + width].mean()
            mask, _, _, margin = lf.run(P, 1, 10, **Q10)
            lad = mask[:, lo: lo + width].mean()
            outside = (mask.sum() - mask[:, lo: lo + width].sum()) / (rows * (n - width))
            line.append((db, cfar, lad, outside))
            assert (margin > lf.DECIDED).all()
        print(f"N = {n}, emitter {width} bins wide: " + "; ".join(f"+{db} dB CFAR {c:.3f} LAD {d:.3f} (outside {o:.1e})" for db, c, d, o in line))
        assert line[-1][1] <= 0.2 and line[-1][2] >= 0.98, line[-1]


def test_occupancy_limit():
    """The floor needs noise to stand on: the detected share of an emitter that fills 50 .. 95 % of the row, at +3 and +10 dB, printed
    for DESIGN.md.  How far it holds depends on the level: the search stops where the sorted values jump by more than t_cme over their
    mean, so an emitter only 3 dB up fades once it fills more than half of the row and is gone at 90 %, while one 10 dB up is still seen
    whole at 90 %."""
    rng = np.random.default_rng(5)
    n, k = 512, 10
    got = {}
    for db in (3, 10):
        for share in (50, 70, 80, 90, 95):
            w = n * share // 100
            P = rng.gamma(float(k), 1.0 / k, (50, n))
            P[:, :w] += 10.0 ** (db / 10.0) * rng.gamma(float(k), 1.0 / k, (50, w))
            got[db, share] = lf.run(P.astype(np.float32), 1, 10, **Q10)[0][:, :w].mean()
        print(f"emitter bins detected at +{db} dB by the share of the row it fills:", ", ".join(f"{s} % {got[db, s]:.3f}" for s in (50, 70, 80, 90, 95)))
    assert got[10, 50] >= 0.98 and got[10, 80] >= 0.98 and got[3, 90] <= 0.5
