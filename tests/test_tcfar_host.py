"""crn_tcfar_device on the host: the twin (tests/tcfar_f64.py) against a brute-force restatement of the header's rule, ties included; the
twin's independence of cuts; the C ABI and every refusal of crn_tcfar_hist_bytes without a GPU; and the simulation that states what the
design claims (DESIGN.md §5 quotes its printed numbers): a receiver whose floor is not flat and that has a spur and a DC spike, against
the excised-floor detector on the same rows."""
import ctypes as C
import math
import os
import re

import numpy as np

import crnsense as cs
import lad_f64 as lf
import tcfar_cases as tc
import tcfar_f64 as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _whole(P, eps, cells, guard, rank, alpha, or_mask=None, fill=0.0):
    hist, seen = tf.new_state(P.shape[0] // eps, P.shape[1], cells, guard, fill)
    mask, rows = tf.run(P, eps, cells, guard, rank, alpha, hist, seen, True, or_mask)
    return mask, rows, hist, seen


# ---- the twin -------------------------------------------------------------------------------------------------------------------
def test_twin_against_brute_force():
    """Tiny streams, quantised to quarters with alpha = 2 so that fl32(alpha c) == P occurs (and must not count), and unquantised."""
    rng = np.random.default_rng(1)
    ties = 0
    for cells, guard, rank, T in ((2, 0, 1, 7), (2, 0, 2, 5), (4, 2, 1, 15), (4, 2, 3, 13), (6, 1, 6, 20), (8, 0, 4, 9), (8, 3, 2, 11)):
        for quantised, alpha in ((True, 2.0), (False, 1.7), (True, 1.0)):
            P = rng.gamma(10.0, 0.1, (T, 8))
            if quantised:
                P = np.maximum(np.round(P * 4.0), 1.0) / 4.0
            P = P.astype(np.float32)
            mask, rows, _, seen = _whole(P, T, cells, guard, rank, alpha, fill=np.nan)
            want = tf.brute(P, cells, guard, rank, alpha)
            assert (mask == want).all(), (cells, guard, rank, T, quantised)
            H = cells + guard
            assert not mask[:H].any() and (rows["n_cells"][:H] == 0).all() and (rows["n_cells"][H:] == cells).all()
            assert (rows["n_detected"] == want.sum(axis=1)).all() and (rows["n_new"] == rows["n_detected"]).all() and seen[0] == T
            if quantised:
                for gl in range(H, T):
                    ties += int((np.float32(alpha) * P[gl - guard - cells: gl - guard] == P[gl]).sum())
    assert ties > 100, ties                                   # the equality case was met


def test_a_tie_is_not_below_by_hand():
    """One bin, D = 2, g = 0, alpha = 1.  Epoch 2 is 1.5 over the cells (1.5, 1.0): 1.0 < 1.5 counts, the tie 1.5 < 1.5 does not.  Epoch 3
    is 1.0 over (1.5, 1.5): nothing below.  Epoch 4 is 9.0 over (1.0, 1.5): both."""
    Q = np.array([[1.0], [1.5], [1.5], [1.0], [9.0]], np.float32)
    m1 = _whole(Q, 5, 2, 0, 1, 1.0)[0][:, 0]
    m2 = _whole(Q, 5, 2, 0, 2, 1.0)[0][:, 0]
    assert list(m1.astype(int)) == [0, 0, 1, 0, 1]
    assert list(m2.astype(int)) == [0, 0, 0, 0, 1]


def test_or_mask_and_header():
    rng = np.random.default_rng(2)
    P = tc.gamma_rows(3, 40, 64)
    om = rng.random((40, 64)) < 0.1
    plain = _whole(P, 40, 4, 1, 1, 1.2)
    both = _whole(P, 40, 4, 1, 1, 1.2, or_mask=om)
    assert (both[0] == (plain[0] | om)).all()
    assert (both[1]["n_detected"] == (plain[0] | om).sum(axis=1)).all() and (both[1]["n_new"] == (plain[0] & ~om).sum(axis=1)).all()
    assert plain[0].any() and (both[1]["n_new"] < plain[1]["n_new"]).any()


def test_cut_independence_of_the_twin():
    """Two streams in one call, and cut anywhere into several (first = 1, then 0) over a NaN-filled ring: the same masks, headers, seen
    and written slots; the slots of epochs never seen stay NaN."""
    S, T, n = 2, 37, 32
    P = tc.gamma_rows(4, S * T, n, quantised=True)
    for cells, guard in ((2, 0), (4, 2), (8, 3), (30, 7)):
        H = cells + guard
        whole = _whole(P, T, cells, guard, 2, 2.0, fill=np.nan)
        for cuts in ([1], [1, 3, H - 1 + 3] if H + 2 < T else [2], list(range(1, T)), [T - 1]):
            edges = [0] + sorted(set(c for c in cuts if 0 < c < T)) + [T]
            hist, seen = tf.new_state(S, n, cells, guard, np.nan)
            masks, rows = np.zeros((S * T, n), bool), np.zeros(S * T, tf.ROW_DTYPE)
            for i, (a, b) in enumerate(zip(edges[:-1], edges[1:])):
                idx = np.concatenate([s * T + np.arange(a, b) for s in range(S)])
                masks[idx], rows[idx] = tf.run(P[idx], b - a, cells, guard, 2, 2.0, hist, seen, i == 0)
            assert (masks == whole[0]).all() and (rows == whole[1]).all() and (seen == whole[3]).all() and (seen == T).all()
            assert hist.tobytes() == whole[2].tobytes()       # NaN slots compare as bytes
        if T < H:
            assert np.isnan(whole[2][:, T:]).all() and not np.isnan(whole[2][:, :T]).any()
        assert tf.written_slots(T, cells, guard) == list(range(min(H, T)))


def test_seen_is_clamped_and_first_ignores_the_state():
    P = tc.gamma_rows(5, 12, 16)
    for start, want in ((-5, 0), (tf.SEEN_MAX + 9, tf.SEEN_MAX), (7, 7)):
        hist, seen = tf.new_state(1, 16, 2, 1)
        seen[0] = start
        tf.run(P, 12, 2, 1, 1, 1.5, hist, seen, False)
        assert seen[0] == want + 12
        seen[0] = start
        tf.run(P, 12, 2, 1, 1, 1.5, hist, seen, True)
        assert seen[0] == 12


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_structures_and_binding(built):
    L = cs.lib()
    for name in ("crn_tcfar_device", "crn_tcfar_hist_bytes"):
        assert name in cs.EXPORTS and hasattr(L, name)
    assert C.sizeof(cs.TcfarParams) == 32 and C.sizeof(cs.TcfarRow) == 16 and np.dtype(cs.TCFAR_ROW_DTYPE).itemsize == 16
    assert cs.TCFAR_ROW_DTYPE == tf.ROW_DTYPE == [(f[0], "<i4") for f in cs.TcfarRow._fields_]
    hdr = open(os.path.join(ROOT, "include", "crn_sense.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip()
                for f in re.sub(r"^\s*(int32_t|float)\s", "", decl.strip()).split(",")]
    assert fields("crn_tcfar_params") == [f[0] for f in cs.TcfarParams._fields_]
    assert fields("crn_tcfar_row") == [f[0] for f in cs.TCFAR_ROW_DTYPE]
    assert "/* 32 bytes */" in hdr[hdr.index("} crn_tcfar_params;"):][:40] and "/* 16 bytes */" in hdr[hdr.index("} crn_tcfar_row;"):][:40]
    assert callable(cs.Sensor.tcfar_device)
    assert L.crn_abi_version() == cs.CRN_ABI_VERSION == 4     # additive: the ABI version stays
    assert open(os.path.join(ROOT, "cognitive-radio-network_amd", "cognitive_engines", "CE_Predictive_Node_GPU", "crn_sense.h")).read() == hdr
    q = cs.tcfar_params(100, 64, 16, 1.5, guard_epochs=1, first=True)
    assert (q.epochs_per_stream, q.first, q.cells, q.guard_epochs, q.rank, q.alpha, list(q.reserved)) == (100, 1, 64, 1, 16, 1.5, [0, 0])


def test_alpha_is_the_ordered_statistic_cfars(built):
    for pfa, k, cells, rank in ((1e-3, 10, 64, 16), (1e-2, 1, 2, 1), (1e-4, 4, 128, 96)):
        assert cs.tcfar_alpha(pfa, k, cells, rank) == cs.cfar_alpha(pfa, k, cells // 2, method="os", rank=rank) > 0.0


def test_hist_bytes_and_every_refusal(built):
    L = cs.lib()

    def nb(n_streams=3, n=1024, reserved=(0, 0), null=False, **kw):
        q = cs.tcfar_params(**{"epochs_per_stream": 10, "cells": 64, "rank": 16, "alpha": 1.5, "guard_epochs": 1, **kw})
        for i, x in enumerate(reserved):
            q.reserved[i] = x
        return L.crn_tcfar_hist_bytes(n_streams, n, None if null else C.byref(q))
    assert nb() == 3 * 65 * 1024 * 4 == cs.tcfar_hist_bytes(3, 1024, cs.tcfar_params(10, 64, 16, 1.5))
    assert nb(1, 512, cells=2, guard_epochs=0, rank=2) == 2 * 512 * 4 and nb(2 ** 20, 4096, cells=128, guard_epochs=16, rank=128) == 2 ** 20 * 144 * 4096 * 4
    assert nb(first=True) == nb() and nb(epochs_per_stream=1) == nb() and nb(alpha=1e-30) == nb()
    inf, nan = math.inf, math.nan
    for bad in ({"null": True}, {"n_streams": 0}, {"n_streams": -1}, {"n": 0}, {"n": 256}, {"n": 1000}, {"n": 8192}, {"n": -512},
                {"epochs_per_stream": 0}, {"epochs_per_stream": -3},
                {"cells": 0}, {"cells": 1}, {"cells": 63}, {"cells": 130}, {"cells": -2}, {"cells": 129},
                {"guard_epochs": -1}, {"guard_epochs": 17},
                {"rank": 0}, {"rank": 65}, {"rank": -1}, {"cells": 2, "rank": 3},
                {"alpha": 0.0}, {"alpha": -1.0}, {"alpha": inf}, {"alpha": nan},
                {"reserved": (1, 0)}, {"reserved": (0, -1)}):
        assert nb(**bad) == -1, bad
    try:
        cs.tcfar_hist_bytes(0, 512, cs.tcfar_params(10, 64, 16, 1.5))
        assert False
    except cs.CrnError:
        pass


def test_no_handle_is_refused_before_anything_is_looked_at(built):
    L = cs.lib()
    q = cs.tcfar_params(8, 4, 1, 1.5)
    buf = (C.c_uint8 * 65536)()
    p = (C.addressof(buf) + 63) & ~63
    assert L.crn_tcfar_device(None, p, 8, C.byref(q), p, p, p, p, p, None) == cs.CRN_ERR_ARG
    assert b"crn_tcfar_device" in L.crn_last_error()
    assert L.crn_tcfar_device(None, None, -1, None, None, None, None, None, None, None) == cs.CRN_ERR_ARG
    assert not bytes(buf).strip(b"\0")


# ---- the simulation -------------------------------------------------------------------------------------------------------------
def test_receiver_with_a_shaped_floor_a_spur_and_a_dc_spike(built):
    """N = 512, K = 10, 1024 epochs; the floor 1 + 0.75 cos(2 pi k / N), x100 at bin 100, x30 at bin 0; channels of 30, 33 and 120 bins,
    one of idle / 1 / 2 / 3 driven per epoch.  D = 64, rank 16, guard 1, alpha for 1e-3; LAD with one block at 1e-2 / 1e-4 on the same
    rows.  The bars (tests/tcfar_cases.py): the false-alarm rate in noise within a factor 1.5 of 1e-3; the driven channel's bins set
    >= 0.9 at +6 dB and >= 0.99 at +10 dB; the spur bin set in under 1 % of the epochs; LAD over 0.2 false alarms on idle bins."""
    alpha = cs.tcfar_alpha(tc.PFA, tc.K, tc.CELLS, tc.RANK)
    H = tc.CELLS + tc.GUARD
    t = lf.factor(1e-2, tc.K)
    lad_q = (t, lf.factor(1e-2, tc.K, t), lf.factor(1e-4, tc.K, t))
    rng = np.random.default_rng(2025)
    P, pick = tc.simulate(rng, 1024, None)
    mask, _, _, _ = _whole(P, 1024, tc.CELLS, tc.GUARD, tc.RANK, alpha)
    decisions = mask[H:].size
    rate = mask[H:].mean()
    print(f"noise only: alpha {alpha:.4f}; false-alarm rate {rate:.3e} over {decisions} decisions; spur bin set in {mask[H:, tc.SPUR_BIN].mean():.2e} "
          f"of the epochs, DC bin in {mask[H:, tc.DC_BIN].mean():.2e}")
    assert decisions >= 4e5 and tc.FA_LO <= rate <= tc.FA_HI, rate
    got = {}
    for db in (3, 6, 10):
        P, pick = tc.simulate(rng, 1024, db)
        mask, _, _, _ = _whole(P, 1024, tc.CELLS, tc.GUARD, tc.RANK, alpha)
        rows = slice(H, 1024, 3)                                # LAD: every third epoch is enough for a share
        lad = np.zeros(mask.shape, bool)
        lad[rows] = lf.run(P[rows], 1, 10, *lad_q)[0]
        new = tc.shares(mask, pick, skip=H)
        old = tc.shares(lad[rows], pick[rows])
        got[db] = (new, old)
        print(f"+{db} dB: driven channel's bins set: LAD {old[0]:.3f} / along time {new[0]:.3f}; false alarms on idle bins {old[1]:.3f} / {new[1]:.2e}; "
              f"spur set {old[2]:.2f} / {new[2]:.2e}; DC set {old[3]:.2f} / {new[3]:.2e}")
        assert new[2] < tc.SPUR_BAR and tc.FA_LO <= new[1] <= tc.FA_HI, (db, new)
        assert old[1] > tc.LAD_FALSE_BAR, (db, old)
    assert got[6][0][0] >= tc.SHARE_6DB and got[10][0][0] >= tc.SHARE_10DB, got
