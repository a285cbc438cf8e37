"""Tracks from the segment lists, without a GPU: the float64 twin (tests/tracks_f64.py) on hand-made segment lists whose answers are
written out here by hand from the definition in include/crn_sense.h; the whole chain on the twins that exist (the C oracle's
generator -> its spectrum -> cfar_f64 -> segments_f64 -> tracks_f64) on the intended Markov chain, which is where the parameters of
the end-to-end GPU test (tests/test_tracks_gpu.py) come from; and the C ABI: symbols, structures, the refusals that need no handle,
the workspace size."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crnsense as cs
import tracks_f64 as tk
from tracks_cases import E2E, check_end_to_end, e2e_cfg, e2e_synth, runs_of_truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 256


def _run(E, per_epoch, S=4, eps=None, **kw):
    ep, sg = tk.make_lists(E, S, per_epoch)
    return tk.run(ep, sg, N, E if eps is None else eps, **kw)


def _spans(streams, tracks, st=0):
    return [(int(t["first_t"]), int(t["last_t"])) for t in tracks[st, : streams["n_stored"][st]]]


def test_one_emitter_is_one_track():
    st, tr, of = _run(12, {e: [(10, 3)] for e in range(3, 10)}, slack_bins=0)
    assert (st["n_found"][0], st["n_stored"][0], st["n_nodes"][0]) == (1, 1, 7)
    t = tr[0, 0]
    assert (t["first_t"], t["last_t"], t["first_slot"], t["last_slot"], t["n_epochs_hit"], t["n_segments"]) == (3, 9, 0, 0, 7, 7)
    assert (t["lo_off"], t["hi_off"], t["width_sum"], t["flags"]) == (0, 2, 21, 0)
    assert t["power_sum"] == 7.0 and t["peak_power"] == 1.0 and t["centre"] == pytest.approx(11.0)
    assert (of[3:10, 0] == 0).all() and (of[:3] == -1).all() and (of[10:] == -1).all() and (of[:, 1:] == -1).all()
    assert not tr[0, 1:].tobytes().strip(b"\0")


def test_gap_bridged_by_max_miss():
    lists = {e: [(40, 2)] for e in (2, 3, 5, 6)}
    st, tr, of = _run(8, lists, slack_bins=0, max_miss=1)
    assert _spans(st, tr) == [(2, 6)] and tr[0, 0]["n_epochs_hit"] == 4 and tr[0, 0]["flags"] == 2      # 6 >= 8 - 1 - 1
    st, tr, of = _run(8, lists, slack_bins=0, max_miss=0)
    assert _spans(st, tr) == [(2, 3), (5, 6)] and of[[2, 3, 5, 6], 0].tolist() == [0, 0, 1, 1]


def test_pair_across_the_wrap():
    """lo = N - 1 then lo = 0, one bin each: no shared bin, touching.  Powers 1 and 3, so the centre is N - 1 + 3 / 4."""
    lists = {0: [(N - 1, 1, 1.0, 0.0)], 1: [(0, 1, 3.0, 0.0)]}
    st, tr, _ = _run(2, lists, slack_bins=0)
    assert st["n_found"][0] == 2 and _spans(st, tr) == [(0, 0), (1, 1)]
    st, tr, _ = _run(2, lists, slack_bins=1)
    assert st["n_found"][0] == 1 and _spans(st, tr) == [(0, 1)]
    t = tr[0, 0]
    assert (t["lo_off"], t["hi_off"], t["power_sum"]) == (0, 1, 4.0) and t["centre"] == pytest.approx(N - 1 + 0.75)
    # the other way round the circle: the root is the segment at lo = 0, the member sits at offset -1
    st, tr, _ = _run(2, {0: [(0, 1, 3.0, 0.0)], 1: [(N - 1, 1, 1.0, 0.0)]}, slack_bins=1)
    t = tr[0, 0]
    assert (t["lo_off"], t["hi_off"]) == (-1, 0) and t["centre"] == pytest.approx(N - 0.25)
    # a segment of width N links to everything, a wrap-crossing one to what it covers
    st, tr, _ = _run(2, {0: [(0, N)], 1: [(77, 1), (200, 3)]}, slack_bins=0)
    assert st["n_found"][0] == 1 and tr[0, 0]["n_segments"] == 3
    st, tr, _ = _run(2, {0: [(N - 2, 4)], 1: [(1, 1), (2, 1)]}, slack_bins=0)
    assert st["n_found"][0] == 2 and [int(x) for x in tr[0, :2]["n_segments"]] == [2, 1]


def test_sweep_needs_the_slack_of_its_step():
    """Width 4, stepping 8 bins per epoch: the gap between consecutive positions is 4 bins, smaller than slack_bins from 5 on."""
    lists = {e: [(8 * e, 4)] for e in range(6)}
    st, tr, _ = _run(6, lists, slack_bins=4)
    assert st["n_found"][0] == 6 and _spans(st, tr) == [(e, e) for e in range(6)]
    st, tr, _ = _run(6, lists, slack_bins=5)
    assert st["n_found"][0] == 1 and _spans(st, tr) == [(0, 5)]
    t = tr[0, 0]
    assert (t["lo_off"], t["hi_off"], t["width_sum"], t["n_segments"], t["flags"]) == (0, 43, 24, 6, 3)
    assert t["centre"] == pytest.approx(20 + 1.5)          # offsets 0, 8, .. 40, equal powers, centroid 1.5


def test_two_carriers_that_merge_once_are_one_track():
    lists = {e: [(10, 2), (20, 2)] for e in (0, 1, 2, 4, 5)}
    lists[3] = [(10, 12)]
    st, tr, of = _run(6, lists, slack_bins=0)
    assert st["n_found"][0] == 1 and tr[0, 0]["n_segments"] == 11 and tr[0, 0]["n_epochs_hit"] == 6
    assert (tr[0, 0]["first_slot"], tr[0, 0]["last_slot"], tr[0, 0]["lo_off"], tr[0, 0]["hi_off"]) == (0, 0, 0, 11)
    assert (of[:, :2][np.array([[True, True]] * 3 + [[True, False]] + [[True, True]] * 2)] == 0).all()
    del lists[3]                                           # without the merging epoch they stay apart (max_miss 1 bridges the hole)
    st, tr, of = _run(6, lists, slack_bins=0, max_miss=1)
    assert st["n_found"][0] == 2 and of[0].tolist()[:2] == [0, 1] and of[5].tolist()[:2] == [0, 1]


def test_min_epochs_drops_singles_and_labels_them():
    lists = {e: [(100, 2)] for e in range(1, 6)}
    lists[2] = [(30, 1), (100, 2)]
    lists[4] = [(100, 2), (180, 1)]
    st, tr, of = _run(7, lists, slack_bins=1, min_epochs=1)
    assert st["n_found"][0] == 3 and _spans(st, tr) == [(1, 5), (2, 2), (4, 4)]
    assert of[2].tolist()[:2] == [1, 0] and of[4].tolist()[:2] == [0, 2]
    assert (tr[0, 0]["first_slot"], tr[0, 0]["last_slot"]) == (0, 0) and tr[0, 1]["first_slot"] == 0 and tr[0, 2]["first_slot"] == 1
    st, tr, of = _run(7, lists, slack_bins=1, min_epochs=2)
    assert st["n_found"][0] == 1 and _spans(st, tr) == [(1, 5)] and st["n_nodes"][0] == 7
    assert of[2].tolist()[:2] == [-1, 0] and of[4].tolist()[:2] == [0, -1]
    # two members in ONE epoch are one hit: a component living in a single epoch cannot exist (no links inside an epoch), but a
    # component of two epochs with three members has n_epochs_hit 2
    st, tr, _ = _run(2, {0: [(10, 2), (13, 2)], 1: [(11, 3)]}, slack_bins=0, min_epochs=2)
    assert (tr[0, 0]["n_epochs_hit"], tr[0, 0]["n_segments"]) == (2, 3)
    st, tr, _ = _run(2, {0: [(10, 2), (13, 2)], 1: [(11, 3)]}, slack_bins=0, min_epochs=3)
    assert st["n_found"][0] == 0


def test_truncation_keeps_the_count():
    lists = {0: [(20 * k, 2) for k in range(4)], 1: [(20 * k, 2) for k in range(4)], 2: [(200, 1)]}
    st, tr, of = _run(3, lists, slack_bins=0, max_tracks=2)
    assert (st["n_found"][0], st["n_stored"][0]) == (5, 2) and tr.shape == (1, 2)
    assert of[0].tolist() == [0, 1, 2, 3] and of[2].tolist() == [4, -1, -1, -1]
    # segments beyond max_segments were never stored and are not seen
    st, tr, of = _run(3, lists, S=2, slack_bins=0, max_tracks=8)
    assert (st["n_found"][0], st["n_nodes"][0]) == (3, 5)


def test_no_link_across_a_stream_boundary_and_the_flags():
    lists = {e: [(50, 4)] for e in range(2, 6)}
    st, tr, of = _run(8, lists, eps=4, slack_bins=0)
    assert st["n_found"].tolist() == [1, 1] and _spans(st, tr, 0) == [(2, 3)] and _spans(st, tr, 1) == [(0, 1)]
    assert tr[0, 0]["flags"] == 2 and tr[1, 0]["flags"] == 1 and of[:, 0].tolist() == [-1, -1, 0, 0, 0, 0, -1, -1]
    st, tr, _ = _run(8, lists, eps=8, slack_bins=0)
    assert st["n_found"].tolist() == [1] and tr[0, 0]["flags"] == 0
    st, tr, _ = _run(8, lists, eps=8, slack_bins=0, max_miss=2)
    assert tr[0, 0]["flags"] == 3                             # first_t 2 <= 2, last_t 5 >= 8 - 1 - 2
    st, tr, _ = _run(8, {e: [(50, 4)] for e in range(8)}, eps=4, slack_bins=0, max_miss=3)
    assert [t["flags"] for t in tr[:, 0]] == [3, 3] and _spans(st, tr, 1) == [(0, 3)]


# ---- the chain on the twins -------------------------------------------------------------------------------------------------
def test_chain_on_the_twins_finds_every_dwell_run(built):
    """8 streams x 104 epochs of the intended Markov chain from the C oracle's generator, through the oracle's spectrum, the CFAR twin,
    the segments twin and the tracks twin with the E2E parameters: every dwell run is exactly one track, every other track lives one
    epoch, the transition counts come back."""
    import cfar_f64 as cf
    import oracle_py as orc
    import segments_f64 as sg
    cfg = e2e_cfg()
    n_streams, eps = 8, E2E["eps"]
    E = n_streams * eps
    iq, truth = orc.synth(cfg, e2e_synth(n_streams), E, cs.samples_per_epoch(cfg))
    P = orc.run(cfg, iq, E, want_spectrum=True)["spectrum"].astype(np.float64)
    alpha = cs.cfar_alpha(E2E["pfa"], E2E["k"], E2E["train"])
    det = cf.ratio(P, E2E["guard"], E2E["train"], alpha) > 1.0
    ep, segs = sg.run(det, P, E2E["merge_gap"], E2E["min_width"], E2E["max_segments"])
    assert (ep["n_found"] == ep["n_stored"]).all()
    streams, tracks, track_of = tk.run(ep, segs, cfg.fft_len, eps, E2E["slack_bins"], E2E["max_miss"], E2E["min_epochs"], E2E["max_tracks"])
    n_runs, n_other = check_end_to_end(cfg, truth.reshape(n_streams, eps), streams, tracks)
    print(f"twins, {n_streams} streams x {eps} epochs: {n_runs} dwell runs each one track, {n_other} other tracks of one epoch, "
          f"{int(det.sum()) - int((truth > 0).sum())} detections off the carrier")
    assert n_runs == sum(len(runs_of_truth(r)) for r in truth.reshape(n_streams, eps))
    assert ((track_of >= 0) == (np.arange(segs.shape[1])[None, :] < ep["n_stored"][:, None])).all()       # min_epochs 1: every node labelled


# ---- the C ABI --------------------------------------------------------------------------------------------------------------
def test_symbols_structures_and_binding(built):
    L = cs.lib()
    for name in ("crn_tracks_device", "crn_tracks_workspace_bytes"):
        assert name in cs.EXPORTS and hasattr(L, name)
    assert C.sizeof(cs.TrackParams) == 32
    assert (np.dtype(cs.TRACK_DTYPE).itemsize, np.dtype(cs.TRACK_STREAM_DTYPE).itemsize) == (64, 16)
    hdr = open(os.path.join(ROOT, "include", "crn_sense.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.sub(r"\[\d+\]", "", f).strip() for decl in body.split(";") if decl.strip()
                for f in re.sub(r"^\s*(int32_t|int64_t|float)\s", "", decl.strip()).split(",")]
    assert fields("crn_track_params") == [f[0] for f in cs.TrackParams._fields_]
    assert fields("crn_track") == list(np.dtype(cs.TRACK_DTYPE).names)
    assert fields("crn_track_stream") == list(np.dtype(cs.TRACK_STREAM_DTYPE).names)
    assert [n for n in np.dtype(cs.TRACK_DTYPE).names if n != "reserved"] == list(tk.TRACK_F64.names)
    assert callable(cs.Sensor.tracks_device)
    assert L.crn_abi_version() == cs.CRN_ABI_VERSION == 4     # additive: the ABI version stays


def test_refusals_that_need_no_handle(built):
    L = cs.lib()
    q = cs.track_params(16, 4, 1, 0, 1, 64)
    buf = (C.c_uint8 * 65536)()
    p = (C.addressof(buf) + 63) & ~63
    nb = L.crn_tracks_workspace_bytes(4, C.byref(q))
    assert 0 < nb <= 65536 - 64
    assert L.crn_tracks_device(None, p, p, 4, C.byref(q), p, p, p, p, nb, None) == cs.CRN_ERR_ARG
    assert b"crn_tracks_device" in L.crn_last_error()
    assert L.crn_tracks_device(None, p, p, 0, C.byref(q), p, p, None, p, nb, None) == cs.CRN_ERR_ARG
    assert L.crn_tracks_device(None, None, None, -1, None, None, None, None, None, 0, None) == cs.CRN_ERR_ARG


def test_workspace_bytes(built):
    L = cs.lib()

    def nb(E, S=16, eps=1, slack=1, miss=0, mine=1, mt=64, r0=0, r1=0):
        q = cs.track_params(S, eps, slack, miss, mine, mt)
        q.reserved[0], q.reserved[1] = r0, r1
        return L.crn_tracks_workspace_bytes(E, C.byref(q))
    assert nb(0) > 0
    sizes = [nb(E) for E in (0, 1, 2, 64, 6656, 100000)]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    sizes = [nb(6656, S=S) for S in (1, 2, 16, 17, 256)]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert nb(6656, eps=104) == nb(6656, eps=6656) == cs.tracks_workspace_bytes(6656, 16, 104)
    # at least the parent array and one accumulator word per node
    assert nb(6656) >= 6656 * 16 * 8
    for bad in ({"E": -1}, {"S": 0}, {"S": 257}, {"eps": 0}, {"E": 10, "eps": 3}, {"miss": -1}, {"miss": 16}, {"mine": 0}, {"mt": 0}, {"mt": 1025},
                {"r0": 1}, {"r1": 1}, {"slack": -1}, {"E": 2 ** 31, "S": 1}, {"E": 2 ** 23, "S": 256}):
        assert nb(**{"E": 6656, **bad}) <= 0, bad
    assert L.crn_tracks_workspace_bytes(4, None) <= 0
    with pytest.raises(cs.CrnError):
        cs.tracks_workspace_bytes(10, 16, 3)


def test_track_hz():
    n, fs, fc = 1024, 1.0e6, 2.4e9
    f, bw = cs.track_hz(104.5, 30, 3, n, fs, fc)
    assert f == pytest.approx(fc + 104.5 * fs / n, abs=1e-3) and bw == pytest.approx(10 * fs / n)
    f, bw = cs.track_hz(1023.5, 7, 2, n, fs, fc)              # just below fc
    assert f == pytest.approx(fc - 0.5 * fs / n, abs=1e-3) and bw == pytest.approx(3.5 * fs / n)
    assert cs.track_hz(0.0, 4, 4, n, fs, fc) == (pytest.approx(fc), pytest.approx(fs / n))
