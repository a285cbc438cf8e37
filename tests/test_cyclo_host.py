"""crn_cyclo_device without a GPU: the twin (tests/cyclo_f64.py) against answers known in closed form, the threshold helper against
simulated noise, the symbol rate of simulated RRC-QPSK carriers, and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crnsense as cs
import cyclo_cases as cc
import cyclo_f64 as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the twin ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames,q0", [(8, 3), (16, 1), (32, 5), (64, 0)])
def test_chain_known_answer(frames, q0):
    """X_f[lo + i] = u_i e^(j 2 pi q0 i f / F): every pair of the span is perfectly coherent at q = q0 a mod F and at no other q."""
    n, lo, width, a_lo, n_a = 512, 37, 40, 2, 12
    X = cc.chain(np.random.default_rng(frames), n, frames, lo, width, q0).astype(np.complex128)
    S, z, tested, pairs = cf.cells(X, lo, width, a_lo, n_a, 1024, 4)
    assert tested.all() and (pairs == width - a_lo - np.arange(n_a)).all()
    want = np.zeros((n_a, frames))
    want[np.arange(n_a), (q0 * (a_lo + np.arange(n_a))) % frames] = 1.0
    # S is rounded to fp32 once: the twin's fp64 mean is checked to 1e-12 through the exact values 0 and 1
    assert np.abs(S.astype(np.float64) - want).max() <= 1e-12
    rec = cf.record(S, z, tested, pairs, a_lo, 3.0)
    # z grows with n_pairs: the smallest a wins; its cell is the chain's
    assert rec[:4] == (a_lo, (q0 * a_lo) % frames, width - a_lo, n_a) and rec[4] == 1.0
    assert rec[5] == 0.0 and rec[6] == (1.0 if q0 == 0 else 0.0)      # a - 1 is outside the range; (a + 1, q) answers only when q0 = 0


def test_wrap_crossing_span_and_central_window():
    n, F = 512, 16
    rng = np.random.default_rng(7)
    X = cc.noise_spectra(rng, n, F, 1)[0]
    # a span across the wrap is the same span of the rolled spectra
    a = cf.cells(X, 500, 40, 3, 8, 1024, 4)
    b = cf.cells(np.roll(X, 30, axis=1), 18, 40, 3, 8, 1024, 4)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[0].max() > 0
    # lo is taken modulo N, width clamped to 0 .. N
    assert (cf.cells(X, 500 - 512, 40, 3, 8, 1024, 4)[0] == a[0]).all() and (cf.cells(X, 500 + 1024, 40, 3, 8, 1024, 4)[0] == a[0]).all()
    assert cf.span(n, 5, 600, 1024) == (5, 512) and cf.span(n, 5, -3, 1024) == (5, 0)
    # the central max_width bins: integer division
    assert cf.span(n, 100, 43, 20) == (111, 20) and cf.span(n, 505, 43, 20) == (4, 20) and cf.span(n, 100, 20, 20) == (100, 20)
    c = cf.cells(X, 100, 43, 3, 8, 20, 4)
    d = cf.cells(X, 111, 20, 3, 8, 1024, 4)
    assert (c[0] == d[0]).all() and (c[3] == 20 - 3 - np.arange(8)).all()


def test_untested_cells_ties_and_zero_power():
    n, F = 512, 8
    rng = np.random.default_rng(11)
    X = cc.noise_spectra(rng, n, F, 1)[0]
    # width 20, a = 10 .. 17, min_pairs 6: n_pairs 10 .. 3, tested while a <= 14
    S, z, tested, pairs = cf.cells(X, 60, 20, 10, 8, 1024, 6)
    assert tested.tolist() == [True] * 5 + [False] * 3 and (S[5:] == 0).all() and (z[5:] == 0).all() and (S[:5] > 0).all()
    # an untested neighbour reads as 0, and is neither chosen nor counted however large its z
    z2 = z.copy()
    z2[4, 2], z2[6, 1] = 50.0, 99.0
    rec = cf.record(S, z2, tested, pairs, 10, -1e9)
    assert rec[:4] == (14, 2, 6, 5 * F) and rec[4] == S[4, 2] and rec[5] == S[3, 2] and rec[6] == 0.0
    # none tested: all zero
    assert cf.record(*cf.cells(X, 60, 15, 10, 8, 1024, 6), 10, 0.0) == (0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0)
    assert cf.record(*cf.cells(X, 60, 16, 10, 8, 1024, 6), 10, -1e9)[:4][2:] == (6, F)     # exactly one separation tested
    # ties: the smallest a, then the smallest q
    z3 = np.zeros_like(z)
    z3[2, 5] = z3[2, 3] = z3[1, 7] = z3[3, 0] = 4.0
    assert cf.record(S, z3, tested, pairs, 10, 4.0)[:4] == (11, 7, 9, 4)
    z3[1, 7] = 3.0
    assert cf.record(S, z3, tested, pairs, 10, 4.0)[:2] == (12, 3)
    # columns of zero power: rho = 0 for their pairs, nothing else changes and nothing is NaN
    Xz = X.copy()
    Xz[:, 64] = 0
    Sz = cf.cells(Xz, 60, 20, 10, 8, 1024, 6)[0]
    assert np.isfinite(Sz).all() and (Sz[:5] > 0).all() and not (Sz == S).all()
    Xz[:, 60:80] = 0
    assert (cf.cells(Xz, 60, 20, 10, 8, 1024, 6)[0] == 0).all()
    # S lies in [0, 1]
    assert S.min() >= 0 and S.max() <= 1


def test_run_fills_slots_and_profile():
    n, F, ms = 512, 8, 3
    X = cc.noise_spectra(np.random.default_rng(3), n, F, 2)
    heads, recs = cc.records(2, ms, {0: [(10, 40), (500, 30)], 1: []})
    heads["n_stored"][1] = -4
    out, prof = cf.run(X, heads, recs, ms, F, 4, 6, 64, 5, 2.0)
    assert (out["n_pairs"][0, :2] > 0).all() and not out[0, 2].tobytes().strip(b"\0") and not out[1].tobytes().strip(b"\0")
    assert (prof[0, :2] > 0).all() and (prof[0, 2] == 0).all() and (prof[1] == 0).all()
    heads["n_stored"][0] = ms + 7            # clamped; the 0xFF record is lo = -1, width = -1: no cell
    out2, _ = cf.run(X, heads, recs, ms, F, 4, 6, 64, 5, 2.0)
    assert out2.tobytes() == out.tobytes()


# ---- the threshold ----------------------------------------------------------------------------------------------------------------
def test_zmin_is_monotone_and_refuses(built):
    L = cs.lib()
    zs = [cs.cyclo_zmin(p, 32, 16) for p in (0.5, 1e-1, 1e-2, 1e-3, 1e-6, 1e-9)]
    assert all(a < b for a, b in zip(zs, zs[1:])) and abs(zs[0]) < 0.2 and 2.0 < zs[2] < 3.5
    # more pairs: nearer the normal quantile 2.326
    assert cs.cyclo_zmin(1e-2, 32, 16) > cs.cyclo_zmin(1e-2, 32, 256) > 2.326
    z = C.c_double(7.0)
    for pfa, frames, pairs in ((0.0, 32, 16), (1.0, 32, 16), (-0.1, 32, 16), (float("nan"), 32, 16), (1e-2, 12, 16), (1e-2, 0, 16), (1e-2, 128, 16),
                               (1e-2, 32, 0), (1e-2, 32, -3)):
        assert L.crn_cyclo_zmin(pfa, frames, pairs, C.byref(z)) == cs.CRN_ERR_ARG, (pfa, frames, pairs)
        assert b"crn_cyclo_zmin" in L.crn_last_error()
    assert L.crn_cyclo_zmin(1e-2, 32, 16, None) == cs.CRN_ERR_ARG and z.value == 7.0


@pytest.mark.parametrize("frames", [16, 32, 64])
def test_zmin_realised_exceedance_in_noise(built, frames):
    """White noise at N = 512, 5 epochs of 8 disjoint 62-bin segments, a = 8 .. 39 (54 .. 23 pairs), every q: 20 480 F / 16 cells, each
    against crn_cyclo_zmin(1e-2, F, its own n_pairs).  The bar of the header's approximation: 0.6 .. 1.3 x nominal."""
    n, pfa, a_lo, n_a = 512, 1e-2, 8, 32
    X = cc.noise_spectra(np.random.default_rng(100 + frames), n, frames, 5)
    thr = np.array([cs.cyclo_zmin(pfa, frames, 62 - a) for a in range(a_lo, a_lo + n_a)], np.float32)
    over = total = 0
    for e in range(5):
        for g in range(8):
            S, z, tested, pairs = cf.cells(X[e], 64 * g, 62, a_lo, n_a, 1024, 1)
            over += int((z >= thr[:, None]).sum())
            total += z.size
    ratio = over / total / pfa
    print(f"F={frames}: {over} of {total} cells over z_min, {ratio:.3f} x nominal")
    assert total >= 20000 and 0.6 <= ratio <= 1.3, ratio


def test_noise_statistic_has_unit_mean():
    """S F has mean 1 at every cell under white noise (rho is Beta(1, F - 1)), z mean 0 and variance 1."""
    n, F = 512, 32
    X = cc.noise_spectra(np.random.default_rng(5), n, F, 4)
    S, z = [], []
    for e in range(4):
        for g in range(8):
            c = cf.cells(X[e], 64 * g, 62, 8, 32, 1024, 1)
            S.append(c[0])
            z.append(c[1])
    S, z = np.array(S, np.float64), np.array(z, np.float64)
    assert abs(S.mean() * F - 1.0) < 0.01 and abs(z.mean()) < 0.05 and abs(z.var() - 1.0) < 0.1, (S.mean() * F, z.mean(), z.var())


# ---- the symbol rate --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,snr_db,epochs", [(60 / 1.35, 38.0, 6), (60 / 1.35, 6.0, 6), (51.77, 38.0, 5), (30.5, 10.0, 5)])
def test_qpsk_symbol_rate(built, rate, snr_db, epochs):
    """N = 1024, 32 frames, roll-off 0.35, the carrier off the grid at bin 300.3; the segment is the carrier's (1 + roll-off) rate bins.
    cyclo_bins must be within 1 / frames of the true rate in every epoch."""
    n, F, centre = 1024, 32, 300.3
    X = cc.qpsk_spectra(np.random.default_rng(int(rate * 100 + snr_db)), n, F, epochs, rate, centre, snr_db)
    width = int(round(rate * (1 + cc.ROLLOFF)))
    lo = int(round(centre - width / 2))
    heads, recs = cc.records(epochs, 1, {e: [(lo, width)] for e in range(epochs)})
    q = cs.cyclo_params(1, F, a_lo=8, n_a=64, max_width=256, min_pairs=8, pfa=1e-3 / (64 * F))
    out, _ = cf.run(X, heads, recs, 1, F, q.a_lo, q.n_a, q.max_width, q.min_pairs, q.z_min)
    est = np.array([cs.cyclo_bins(out[e, 0], F) for e in range(epochs)])
    print(f"rate {rate:.3f} bins at {snr_db:+.0f} dB: cells {sorted(set(zip(out['a'][:, 0].tolist(), out['q'][:, 0].tolist())))}, "
          f"largest error {np.abs(est - rate).max():.4f} bins (bar {1 / F:.4f}); z {out['z'].min():.1f} .. {out['z'].max():.1f}, z_min {q.z_min:.2f}")
    assert (np.abs(est - rate) <= 1.0 / F).all(), est - rate
    assert (out["z"][:, 0] >= q.z_min).all() and (out["n_over"][:, 0] >= 1).all()
    assert cs.cyclo_hz(out[0, 0], F, n, 1.024e6) == cs.cyclo_bins(out[0, 0], F) * 1e3


def test_cyclo_bins_by_hand():
    rec = cs.Cyclo(a=44, q=14, n_pairs=16, n_over=1, stat=0.5, stat_lo=0.0, stat_hi=0.4, z=30.0)
    assert cs.cyclo_bins(rec, 32) == 44 + 14 / 32                  # a^ = 44.44: the nearest value of the q / 32 family
    rec.stat_lo, rec.stat_hi = 0.4, 0.0                            # a^ = 43.56, q = 18: 43.5625
    rec.q = 18
    assert cs.cyclo_bins(rec, 32) == 43 + 18 / 32
    rec.q = 0
    assert cs.cyclo_bins(rec, 32) == 44.0
    assert cs.cyclo_bins({"a": 0, "q": 0, "n_pairs": 0, "stat": 0.0, "stat_lo": 0.0, "stat_hi": 0.0}, 32) == 0.0
    assert cs.cyclo_hz(rec, 32, 1024, 2.048e6) == 88e3


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_structures_and_binding(built):
    L = cs.lib()
    for name in ("crn_cyclo_device", "crn_cyclo_zmin"):
        assert name in cs.EXPORTS and hasattr(L, name)
    assert callable(cs.Sensor.cyclo_device)
    assert C.sizeof(cs.CycloParams) == 36 and C.sizeof(cs.Cyclo) == 32 and np.dtype(cs.CYCLO_DTYPE).itemsize == 32
    assert cs.CYCLO_DTYPE == cf.CYCLO_DTYPE and cc.SEGMENT_DTYPE == cs.SEGMENT_DTYPE and cc.SEGMENT_EPOCH_DTYPE == cs.SEGMENT_EPOCH_DTYPE
    hdr = open(os.path.join(ROOT, "include", "crn_sense.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip()
                for f in re.sub(r"^\s*(int32_t|float)\s", "", decl.strip()).split(",")]
    assert fields("crn_cyclo_params") == [f[0] for f in cs.CycloParams._fields_]
    assert fields("crn_cyclo") == [f[0] for f in cs.Cyclo._fields_] == [f[0] for f in cs.CYCLO_DTYPE]
    assert "/* 36 bytes */" in hdr[hdr.index("} crn_cyclo_params;"):][:40] and "/* 32 bytes */" in hdr[hdr.index("} crn_cyclo;"):][:40]
    assert hdr.index("crn_measure_device(") < hdr.index("crn_cyclo_device(") < hdr.index("crn_cyclo_zmin(") < hdr.index("crn_sense_reserve_host(")
    engine = os.path.join(ROOT, "cognitive-radio-network_amd", "cognitive_engines", "CE_Predictive_Node_GPU", "crn_sense.h")
    assert open(engine).read() == hdr
    assert L.crn_abi_version() == cs.CRN_ABI_VERSION == 4     # additive: the ABI version stays
    q = cs.cyclo_params()
    assert (q.max_segments, q.frames, q.a_lo, q.n_a, q.max_width, q.min_pairs, list(q.reserved)) == (16, 32, 8, 64, 256, 16, [0, 0])
    assert q.z_min == np.float32(cs.cyclo_zmin(1e-6, 32, 16)) and cs.cyclo_params(z_min=2.5).z_min == 2.5


def test_no_handle_is_refused_before_anything_is_looked_at(built):
    L = cs.lib()
    q = cs.cyclo_params()
    buf = (C.c_uint8 * 65536)()
    p = (C.addressof(buf) + 63) & ~63
    assert L.crn_cyclo_device(None, p, 8, C.byref(q), p, p, p, p, None) == cs.CRN_ERR_ARG
    assert b"crn_cyclo_device" in L.crn_last_error()
    assert L.crn_cyclo_device(None, None, -1, None, None, None, None, None, None) == cs.CRN_ERR_ARG
    assert not bytes(buf).strip(b"\0")
