"""Spectrum holes without a GPU: the twin (tests/holes_f64.py) on hand-made cases whose answers are written out here by hand from the
definition in include/crn_sense.h; the age rule (closed form against the loop, saturation, negative carries); the C ABI (symbols, the
three structure sizes, the workspace size and every refusal of crn_holes_workspace_bytes); hole_hz and pick_hole; and the coverage
simulation that justifies the end-to-end bar of tests/test_holes_gpu.py.

What is refused without a device: crn_holes_device needs a handle for everything but its NULL-handle refusal (a handle needs a device, and
the fake-HIP harness under tests/harness compiles no kernel unit), so here its parameter refusals are reached through
crn_holes_workspace_bytes, which runs the same checking code with min_width held to the largest fft_len.  min_width against the handle's
own fft_len, the alignments and the workspace that is too small need a live handle: tests/test_holes_gpu.py::test_refusals_with_a_live_handle."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crnsense as cs
import holes_f64 as hf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (512, 1024, 2048, 4096)


def _one_epoch(blocked, n, **kw):
    """One stream of one epoch, guard 0, min_age 1: the free bins are exactly the bins outside `blocked`."""
    det = np.zeros((1, n), bool)
    det[0, np.asarray(blocked, int) % n] = True
    kw.setdefault("max_holes", 16)
    age, free, st, holes = hf.run(det, None, 1, **kw)
    assert (free[0] == ~det[0]).all() and (age[0] == (~det[0]).astype(int)).all()
    return st[0], holes[0]


def _stored(st, holes):
    return [(int(h["lo"]), int(h["width"])) for h in holes[: st["n_stored"]]]


# ---- the twin, by hand ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_all_free_and_none_free(n):
    st, holes = _one_epoch([], n)
    assert (st["n_found"], st["n_stored"], st["free_bins"]) == (1, 1, n) and _stored(st, holes) == [(0, n)]
    assert (st["widest_lo"], st["widest_width"], st["widest_age"]) == (0, n, 1)
    st, holes = _one_epoch(np.arange(n), n)
    assert (st["n_found"], st["n_stored"], st["free_bins"]) == (0, 0, 0) and not holes["width"].any()
    assert (st["widest_lo"], st["widest_width"], st["widest_age"]) == (0, 0, 0)
    # min_width = N keeps the whole band and nothing less
    assert _one_epoch([], n, min_width=n)[0]["n_found"] == 1 and _one_epoch([7], n, min_width=n)[0]["n_found"] == 0
    assert _one_epoch([7], n, min_width=n - 1)[0]["n_found"] == 1


@pytest.mark.parametrize("n", SIZES)
def test_a_hole_across_the_wrap_is_stored_last(n):
    blocked = list(range(10, 20)) + list(range(100, n - 20))
    st, holes = _one_epoch(blocked, n)
    assert _stored(st, holes) == [(20, 80), (n - 20, 30)] and st["free_bins"] == 110
    assert (st["widest_lo"], st["widest_width"]) == (20, 80)
    # the wrap-crossing one the wider: it is still stored last, and widest_* names it
    st, holes = _one_epoch(list(range(10, 20)) + list(range(40, n - 20)), n)
    assert _stored(st, holes) == [(20, 20), (n - 20, 30)] and (st["widest_lo"], st["widest_width"]) == (n - 20, 30)
    # a hole that ends exactly at the wrap does not cross it
    st, holes = _one_epoch(list(range(0, 5)) + list(range(30, n - 8)), n)
    assert _stored(st, holes) == [(5, 25), (n - 8, 8)]


@pytest.mark.parametrize("n", SIZES)
def test_equal_widths_truncation_and_min_width(n):
    free = list(range(10, 20)) + list(range(50, 60))
    blocked = [k for k in range(n) if k not in free]
    st, holes = _one_epoch(blocked, n)
    assert _stored(st, holes) == [(10, 10), (50, 10)] and (st["widest_lo"], st["widest_width"]) == (10, 10)
    # max_holes = 1: the first by lo is stored, widest_* still names the one that was not
    free = list(range(5, 8)) + list(range(100, 150))
    blocked = [k for k in range(n) if k not in free]
    st, holes = _one_epoch(blocked, n, max_holes=1)
    assert (st["n_found"], st["n_stored"]) == (2, 1) and _stored(st, holes) == [(5, 3)]
    assert (st["widest_lo"], st["widest_width"], st["widest_age"]) == (100, 50, 1)
    # min_width drops the sliver before anything is counted; free_bins still counts its bins
    st, holes = _one_epoch(blocked, n, min_width=4)
    assert (st["n_found"], st["free_bins"]) == (1, 53) and _stored(st, holes) == [(100, 50)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("guard", [0, 1, 32])
@pytest.mark.parametrize("k", [0, 31, 32, -1])
def test_guard_across_word_edges_and_the_wrap(n, guard, k):
    k %= n
    det = np.zeros((1, n), bool)
    det[0, k] = True
    want = np.zeros(n, bool)
    want[(k + np.arange(-guard, guard + 1)) % n] = True
    assert (hf.dilate(det[0], guard) == want).all()
    age, free, st, holes = hf.run(det, None, 1, guard=guard)
    assert (free[0] == ~want).all() and st[0]["free_bins"] == n - 2 * guard - 1
    assert _stored(st[0], holes[0]) == [((k + guard + 1) % n, n - 2 * guard - 1)]


def test_alternating_bins_at_512():
    n = 512
    st, holes = _one_epoch(np.arange(1, n, 2), n, max_holes=256)
    assert (st["n_found"], st["n_stored"], st["free_bins"]) == (256, 256, 256)
    assert _stored(st, holes) == [(2 * i, 1) for i in range(256)] and (st["widest_lo"], st["widest_width"]) == (0, 1)
    st, holes = _one_epoch(np.arange(1, n, 2), n, max_holes=16)
    assert (st["n_found"], st["n_stored"]) == (256, 16)
    assert _one_epoch(np.arange(1, n, 2), n, min_width=2)[0]["n_found"] == 0


def test_fields_of_a_hole_by_hand():
    """N = 512, T = 3, avg_epochs 2: ages 3 (never blocked), 1 and 0; Pbar the mean of the last two rows."""
    n = 512
    det = np.zeros((3, n), bool)
    det[0, 100:] = True               # bins 100.. blocked in epoch 0: age 2 at the end ...
    det[1, 40:60] = True              # ... 40..59 in epoch 1: age 1
    det[2, 60:] = True                # ... 60.. in the latest: age 0
    P = np.ones((3, n), np.float32)
    P[0] = 1000.0                     # outside the average
    P[1, 7], P[2, 7] = 3.0, 5.0       # Pbar[7] = 4
    P[2, 45] = 7.0                    # Pbar[45] = 4 as well: the tie goes to the smaller offset
    age, free, st, holes = hf.run(det, P, 3, min_age=1, avg_epochs=2)
    assert (age[0, :40] == 3).all() and (age[0, 40:60] == 1).all() and (age[0, 60:] == 0).all()
    h = holes[0, 0]
    assert (h["lo"], h["width"], h["age"], h["age_max"], h["peak_bin"]) == (0, 60, 1, 3, 7) and h["peak_power"] == 4.0 and h["power"] == 66.0
    assert st[0]["floor_mean"] == pytest.approx(66.0 / 60) and st[0]["widest_age"] == 1
    age, free, st, holes = hf.run(det, P, 3, min_age=2, avg_epochs=64)       # A = min(64, 3): the first row enters
    h = holes[0, 0]
    assert (h["lo"], h["width"], h["age"], h["age_max"], h["peak_bin"]) == (0, 40, 3, 3, 7) and h["peak_power"] == np.float32(1008.0 / 3)
    age, free, st, holes = hf.run(det, None, 3, min_age=1)
    assert holes[0, 0]["peak_bin"] == 0 and holes[0, 0]["power"] == 0 and st[0]["floor_mean"] == 0


# ---- the age rule -----------------------------------------------------------------------------------------------------------------
def test_closed_form_equals_the_loop():
    rng = np.random.default_rng(11)
    n = 512
    for T, density, guard in ((1, 0.01, 0), (7, 0.05, 2), (70, 0.02, 1), (130, 0.002, 32), (20, 0.0, 3), (5, 1.0, 0)):
        det = rng.random((T, n)) < density
        start = rng.integers(-5, 50, n)
        assert (hf.ages(det, guard, start) == hf.ages_closed(det, guard, start)).all()
        assert (hf.ages(det, guard) == hf.ages_closed(det, guard)).all()
        # ... and a batch in two calls is the batch in one
        for cut in {1, T // 2, T - 1} - {0, T}:
            assert (hf.ages(det[cut:], guard, hf.ages(det[:cut], guard, start)) == hf.ages(det, guard, start)).all()


def test_saturation_and_negative_carries():
    n, T = 512, 10
    det = np.zeros((T, n), bool)
    det[3, 100] = True
    start = np.full(n, 2 ** 31 - 5)
    start[200] = 2 ** 31 - 1
    start[201] = 2 ** 31 - 11
    start[202] = 2 ** 31 - 12
    a = hf.ages(det, 0, start)
    assert a[0] == 2 ** 31 - 1 and a[200] == 2 ** 31 - 1 and a[201] == 2 ** 31 - 1 and a[202] == 2 ** 31 - 2 and a[100] == 6
    assert (a == hf.ages_closed(det, 0, start)).all()
    start = np.full(n, -7)
    start[5] = -2 ** 31
    a = hf.ages(det, 0, start)
    assert a[0] == T and a[5] == T and a[100] == 6 and (a == hf.ages_closed(det, 0, start)).all()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
def test_symbols_structures_and_binding(built):
    L = cs.lib()
    for name in ("crn_holes_workspace_bytes", "crn_holes_device"):
        assert name in cs.EXPORTS and hasattr(L, name)
    assert (C.sizeof(cs.HoleParams), C.sizeof(cs.Hole), C.sizeof(cs.HoleStream)) == (32, 32, 32)
    assert np.dtype(cs.HOLE_DTYPE).itemsize == 32 and np.dtype(cs.HOLE_STREAM_DTYPE).itemsize == 32
    for dt, st in ((cs.HOLE_DTYPE, cs.Hole), (cs.HOLE_STREAM_DTYPE, cs.HoleStream)):
        assert [(f[0], np.dtype(dt).fields[f[0]][1]) for f in dt] == [(f[0], getattr(st, f[0]).offset) for f in st._fields_]
    hdr = open(os.path.join(ROOT, "include", "crn_sense.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [f.strip() for decl in body.split(";") if decl.strip() for f in re.sub(r"^\s*(int32_t|float)\s", "", decl.strip()).split(",")]
    assert fields("crn_hole_params") == [f[0] for f in cs.HoleParams._fields_]
    assert fields("crn_hole") == [f[0] for f in cs.Hole._fields_]
    assert fields("crn_hole_stream") == [f[0] for f in cs.HoleStream._fields_]
    assert callable(cs.Sensor.holes_device)
    assert L.crn_abi_version() == cs.CRN_ABI_VERSION == 4     # additive: the ABI version stays


def test_no_handle_is_refused_before_anything_is_looked_at(built):
    L = cs.lib()
    q = cs.hole_params(4)
    buf = (C.c_uint8 * 65536)()
    p = (C.addressof(buf) + 63) & ~63
    nb = L.crn_holes_workspace_bytes(8, C.byref(q))
    assert 0 < nb <= 65536 - 64
    assert L.crn_holes_device(None, p, p, 8, C.byref(q), p, p, p, p, p, nb, None) == cs.CRN_ERR_ARG
    assert b"crn_holes_device" in L.crn_last_error()
    assert L.crn_holes_device(None, p, None, 0, C.byref(q), p, p, None, None, p, nb, None) == cs.CRN_ERR_ARG
    assert L.crn_holes_device(None, None, None, -1, None, None, None, None, None, None, 0, None) == cs.CRN_ERR_ARG
    assert not bytes(buf).strip(b"\0")


def test_workspace_bytes_and_its_refusals(built):
    L = cs.lib()

    def nb(E, eps=1, **kw):
        r = kw.pop("reserved", 0)
        q = cs.hole_params(eps, **kw)
        q.reserved = r
        return L.crn_holes_workspace_bytes(E, C.byref(q))
    assert nb(0) > 0 and nb(0, first=True) > 0 and nb(0, eps=1000) > 0
    # one byte per bin of the largest fft_len and (stream, chunk of 64 epochs)
    assert [nb(E, eps=E) for E in (1, 63, 64, 65, 129, 6656)] == [4096 * c for c in (1, 1, 1, 2, 3, 104)]
    assert nb(6656, eps=104) == 64 * 2 * 4096 == cs.holes_workspace_bytes(6656, 104)
    assert nb(6656, guard=32, min_age=2 ** 31 - 1, min_width=4096, max_holes=256, avg_epochs=64, first=True) > 0
    for bad in ({"E": -1}, {"eps": 0}, {"eps": -4}, {"E": 10, "eps": 3}, {"guard": -1}, {"guard": 33}, {"min_age": 0}, {"min_age": -1},
                {"min_width": 0}, {"min_width": 4097}, {"max_holes": 0}, {"max_holes": 257}, {"avg_epochs": 0}, {"avg_epochs": 65},
                {"reserved": 1}, {"reserved": -1}):
        assert nb(**{"E": 6656, **bad}) == -1, bad
    assert L.crn_holes_workspace_bytes(4, None) == -1
    # the longest stream the parameters can name, 2^31 - 1 epochs: the size is computed in 64 bits
    big = 2 ** 31 - 1
    assert nb(big, eps=big) == 2 ** 25 * 4096 and nb(2 * big, eps=big) == 2 ** 26 * 4096
    with pytest.raises(cs.CrnError):
        cs.holes_workspace_bytes(10, 3)


def test_hole_hz():
    n, fs, fc = 512, 512e3, 100e6                 # 1 kHz per bin
    assert cs.hole_hz(10, 1, n, fs, fc) == pytest.approx((fc + 10e3, 1e3))
    assert cs.hole_hz(10, 5, n, fs, fc) == pytest.approx((fc + 12e3, 5e3))
    assert cs.hole_hz(10, 4, n, fs, fc) == pytest.approx((fc + 11.5e3, 4e3))
    assert cs.hole_hz(300, 11, n, fs, fc) == pytest.approx((fc + (305 - 512) * 1e3, 11e3))      # the upper half lies below fc
    assert cs.hole_hz(n - 20, 41, n, fs, fc) == pytest.approx((fc, 41e3))                        # across the wrap: around fc
    assert cs.hole_hz(n - 10, 30, n, fs, fc) == pytest.approx((fc + 4.5e3, 30e3))
    assert cs.hole_hz(0, n, n, fs, fc)[1] == pytest.approx(fs)
    # the mapping is segment_hz's
    assert cs.hole_hz(37, 9, n, fs, fc) == cs.segment_hz(37, 9, 4.0, n, fs, fc)


def test_pick_hole():
    holes = np.zeros(6, np.dtype(cs.HOLE_DTYPE))
    for i, (lo, w, age, power) in enumerate([(10, 8, 5, 8.0), (40, 20, 9, 40.0), (100, 20, 9, 20.0), (200, 40, 9, 40.0), (300, 64, 3, 1.0)]):
        holes[i]["lo"], holes[i]["width"], holes[i]["age"], holes[i]["power"] = lo, w, age, power
    assert cs.pick_hole(holes, 8) == 2                    # the largest age, then the lower power per bin: 1.0 at both 2 and 3, the lower lo
    assert cs.pick_hole(holes, 21) == 3 and cs.pick_hole(holes, 41) == 4 and cs.pick_hole(holes, 65) is None
    holes[3]["power"] = 39.0
    assert cs.pick_hole(holes, 8) == 3                    # now the quieter per bin
    holes[0]["age"] = 10
    assert cs.pick_hole(holes, 8) == 0 and cs.pick_hole(holes, 9) == 3
    assert cs.pick_hole(holes[5:], 1) is None and cs.pick_hole(holes[:0], 1) is None      # an empty slot is no hole


# ---- the coverage simulation ------------------------------------------------------------------------------------------------------
SIM = {"n": 512, "channels": [(40, 96), (200, 96), (380, 96)], "p_flip": 0.1, "pfa": 1e-3, "guard": 2, "min_age": 8, "min_width": 8, "T": 40,
       "streams": 200, "seed": 14}
COVERAGE_BAR = 0.85


def test_coverage_simulation():
    """Three 96-bin channels that flip with p = 0.1 per epoch (every bin of a busy channel detected), Bernoulli false alarms at 1e-3 in
    every other bin, guard 2, min_age 8, min_width 8, 40 epochs, 200 streams.  A bin is truly idle when it lies in no channel that was
    busy in the last 8 epochs.  The stored holes must hold no bin that is not truly idle, and must cover at least 0.85 of the truly
    idle bins, pooled over the streams: what is lost are the bins a false alarm (with its guard) blocked in the last 8 epochs, and the
    slivers between them narrower than min_width.  Each bin is blocked by a false alarm in 8 epochs with probability about
    1 - (1 - 1e-3)^(8 x 5) = 0.04, and the slivers cost about as much again: the figure is printed (DESIGN.md §5 records it)."""
    rng = np.random.default_rng(SIM["seed"])
    n, T, S = SIM["n"], SIM["T"], SIM["streams"]
    idle_bins = covered = violations = 0
    for _ in range(S):
        busy = np.stack([(rng.integers(0, 2) + np.cumsum(rng.random(T) < SIM["p_flip"])) % 2 for _ in SIM["channels"]], axis=1).astype(bool)
        det = rng.random((T, n)) < SIM["pfa"]
        truly_idle = np.ones(n, bool)
        for c, (lo, w) in enumerate(SIM["channels"]):
            det[:, lo: lo + w] = busy[:, c: c + 1]
            if busy[-SIM["min_age"]:, c].any():
                truly_idle[lo: lo + w] = False
        age, free, st, holes = hf.run(det, None, T, guard=SIM["guard"], min_age=SIM["min_age"], min_width=SIM["min_width"], max_holes=16)
        assert st[0]["n_found"] == st[0]["n_stored"]
        inside = np.zeros(n, bool)
        for h in holes[0, : st[0]["n_stored"]]:
            inside[(h["lo"] + np.arange(h["width"])) % n] = True
        violations += int((inside & ~truly_idle).sum())
        covered += int((inside & truly_idle).sum())
        idle_bins += int(truly_idle.sum())
    print(f"coverage simulation: {covered} of {idle_bins} truly idle bins lie in a stored hole: {covered / idle_bins:.4f} pooled over {S} streams "
          f"(bar {COVERAGE_BAR}); {violations} stored bins in a channel busy in the last {SIM['min_age']} epochs")
    assert violations == 0
    assert covered / idle_bins >= COVERAGE_BAR
