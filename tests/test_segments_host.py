"""Segments from the CFAR bin mask, without a GPU: the float64 twin (tests/segments_f64.py) on hand-made masks, whose answers are
written out here by hand from the definition in include/crn_sense.h; the C ABI (the symbol, the three structures, the refusals that
are decided before any device call) and the host helper that turns a segment into hertz."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crnsense as cs
import segments_f64 as sg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 64


def _mask(bits, n=N):
    d = np.zeros(n, bool)
    d[list(bits)] = True
    return d


def _spans(segs):
    return [(s["lo"], s["width"], s["n_detected"]) for s in segs]


def test_empty_mask():
    P = np.arange(N, dtype=np.float64) + 1
    for gap in (0, 5, N - 1):
        h, segs = sg.epoch(_mask([]), P, merge_gap=gap)
        assert segs == [] and (h["n_found"], h["n_stored"], h["noise_bins"]) == (0, 0, N)
        assert h["noise_mean"] == pytest.approx(P.mean(), rel=1e-15)


def test_all_ones():
    P = np.ones(N)
    P[17] = 3.0
    h, segs = sg.epoch(_mask(range(N)), P)
    assert (h["n_found"], h["n_stored"], h["noise_bins"], h["noise_mean"]) == (1, 1, 0, 0.0)
    assert _spans(segs) == [(0, N, N)] and segs[0]["peak_bin"] == 17 and segs[0]["peak_power"] == 3.0
    assert segs[0]["power"] == pytest.approx(N + 2.0) and segs[0]["centroid"] == pytest.approx((sum(range(N)) + 2 * 17) / (N + 2.0))


def test_run_across_the_wrap_comes_last():
    P = np.ones(N)
    P[0] = 5.0
    h, segs = sg.epoch(_mask([62, 63, 0, 1, 10, 11, 30]), P)
    assert _spans(segs) == [(10, 2, 2), (30, 1, 1), (62, 4, 4)]
    assert h["n_found"] == 3 and h["noise_bins"] == N - 7 and h["noise_mean"] == 1.0
    w = segs[-1]
    assert w["peak_bin"] == 0 and w["peak_power"] == 5.0 and w["power"] == 8.0
    assert w["centroid"] == pytest.approx((0 * 1 + 1 * 1 + 2 * 5 + 3 * 1) / 8.0)      # offsets count from lo = 62: bin 0 is offset 2


def test_two_runs_joined_across_the_wrap():
    P = np.ones(N)
    h, segs = sg.epoch(_mask([61, 1]), P, merge_gap=3)        # zeros 62, 63, 0: a run of 3
    assert _spans(segs) == [(61, 5, 2)] and h["noise_bins"] == N - 5
    h, segs = sg.epoch(_mask([61, 1]), P, merge_gap=2)
    assert _spans(segs) == [(1, 1, 1), (61, 1, 1)] and h["noise_bins"] == N - 2


def test_closing_that_fills_the_circle():
    h, segs = sg.epoch(_mask(range(0, N, 2)), np.ones(N), merge_gap=1)
    assert _spans(segs) == [(0, N, N // 2)] and (h["n_found"], h["noise_bins"], h["noise_mean"]) == (1, 0, 0.0)
    # one set bit: its zero run is N - 1 long, circularly
    assert _spans(sg.epoch(_mask([20]), np.ones(N), merge_gap=N - 1)[1]) == [(0, N, 1)]
    assert _spans(sg.epoch(_mask([20]), np.ones(N), merge_gap=N - 2)[1]) == [(20, 1, 1)]


def test_alternating_bits_capped():
    h, segs = sg.epoch(_mask(range(1, N, 2)), np.ones(N), max_segments=8)
    assert (h["n_found"], h["n_stored"], h["noise_bins"]) == (N // 2, 8, N // 2)
    assert _spans(segs) == [(k, 1, 1) for k in range(1, 17, 2)]
    eps, arr = sg.run(_mask(range(1, N, 2))[None], np.ones((1, N)), max_segments=40)
    assert eps["n_stored"][0] == 32 and (arr["width"][0, :32] == 1).all() and not arr["width"][0, 32:].any()


def test_min_width_after_merging_and_noise_before_it():
    P = np.ones(N)
    P[3] = 100.0
    h, segs = sg.epoch(_mask([3, 10, 12]), P, merge_gap=1, min_width=2)
    assert _spans(segs) == [(10, 3, 2)] and h["n_found"] == 1
    # bin 3 was dropped as a sliver, but it is not noise either: the estimate is taken before the filter
    assert h["noise_bins"] == N - 4 and h["noise_mean"] == 1.0
    h, segs = sg.epoch(_mask([3, 10, 12]), P, merge_gap=0, min_width=2)
    assert segs == [] and h["n_found"] == 0 and h["noise_bins"] == N - 3


def test_peak_ties_go_to_the_smallest_offset():
    P = np.ones(N)
    P[[5, 7]] = 4.0
    P[[63, 1]] = 9.0
    _, segs = sg.epoch(_mask([4, 5, 6, 7, 8, 62, 63, 0, 1]), P)
    assert [(s["lo"], s["peak_bin"], s["peak_power"]) for s in segs] == [(4, 5, 4.0), (62, 63, 9.0)]
    _, segs = sg.epoch(_mask([20, 21, 22]), np.zeros(N))
    assert segs[0]["peak_bin"] == 20 and segs[0]["power"] == 0.0 and segs[0]["centroid"] == 0.0


def test_mask_packing_round_trips():
    rng = np.random.default_rng(1)
    det = rng.random((5, 512)) < 0.3
    words = sg.pack_mask(det)
    assert words.shape == (5, 16) and words.dtype == np.uint32
    assert (sg.unpack_mask(words, 512) == det).all()
    assert words[0, 1] >> 3 & 1 == det[0, 35]


def test_symbol_structures_and_binding(built):
    L = cs.lib()
    assert "crn_segments_device" in cs.EXPORTS and hasattr(L, "crn_segments_device")
    assert (C.sizeof(cs.SegmentParams), C.sizeof(cs.Segment), C.sizeof(cs.SegmentEpoch)) == (16, 32, 16)
    assert (np.dtype(cs.SEGMENT_DTYPE).itemsize, np.dtype(cs.SEGMENT_EPOCH_DTYPE).itemsize) == (32, 16)
    assert [f[0] for f in cs.Segment._fields_] == [f[0] for f in cs.SEGMENT_DTYPE] == list(np.dtype(cs.SEGMENT_DTYPE).names)
    assert [f[0] for f in cs.SegmentEpoch._fields_] == [f[0] for f in cs.SEGMENT_EPOCH_DTYPE]
    assert callable(cs.Sensor.segments_device)
    hdr = open(os.path.join(ROOT, "include", "crn_sense.h")).read()
    for name, fields in (("crn_segment_params", "merge_gap, min_width, max_segments, reserved"), ("crn_segment_epoch", "n_found, n_stored, noise_bins")):
        assert re.search(r"typedef struct %s \{\s*int32_t %s;" % (name, fields), hdr), name
    assert L.crn_abi_version() == cs.CRN_ABI_VERSION        # additive: the ABI version stays


def test_refusals_decided_before_any_device_call(built):
    """Without a handle nothing can reach the device: a NULL handle is refused whatever else is passed."""
    L = cs.lib()
    q = cs.SegmentParams(merge_gap=0, min_width=1, max_segments=16, reserved=0)
    buf = (C.c_uint8 * 4096)()
    p = C.addressof(buf)
    assert L.crn_segments_device(None, p, p, 1, C.byref(q), p, p, None) == cs.CRN_ERR_ARG
    assert b"crn_segments_device" in L.crn_last_error()
    assert L.crn_segments_device(None, p, p, 0, C.byref(q), p, None, None) == cs.CRN_ERR_ARG
    assert L.crn_segments_device(None, None, None, -1, None, None, None, None) == cs.CRN_ERR_ARG


def test_segment_hz():
    n, fs, fc = 1024, 1.0e6, 2.4e9
    # lower half: bin k at fc + k fs / N
    f, bw = cs.segment_hz(100, 10, 4.5, n, fs, fc)
    assert f == pytest.approx(fc + 104.5 * fs / n, abs=1e-3) and bw == pytest.approx(10 * fs / n)
    # upper half: bin k at fc + (k - N) fs / N
    f, bw = cs.segment_hz(900, 8, 3.0, n, fs, fc)
    assert f == pytest.approx(fc + (903.0 - n) * fs / n, abs=1e-3) and bw == pytest.approx(8 * fs / n)
    # across the wrap: one emitter around fc, on whichever side its centroid falls
    f, bw = cs.segment_hz(1022, 4, 1.5, n, fs, fc)
    assert f == pytest.approx(fc - 0.5 * fs / n, abs=1e-3) and bw == pytest.approx(4 * fs / n)
    f, _ = cs.segment_hz(1022, 4, 2.5, n, fs, fc)
    assert f == pytest.approx(fc + 0.5 * fs / n, abs=1e-3)
    f, _ = cs.segment_hz(1023, 2, 1.0, n, fs, fc)
    assert f == pytest.approx(fc, abs=1e-3)
