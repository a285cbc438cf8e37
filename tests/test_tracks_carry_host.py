"""Tracks carried across batches, without a GPU: the float64 twin of the incremental rule (tests/tracks_carry_f64.py) against the
whole-batch twin (tests/tracks_f64.py) on the concatenated lists, cut into random calls; hand-made cases with the answers written out
from the definition in include/crn_sense.h; the intended-Markov chain on the twins fed in calls of 8 epochs; and the C ABI: the three
symbols, the 32-byte header, the refusals that need no handle, the two size functions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crnsense as cs
import segments_f64 as sg
import tracks_carry_f64 as tc
import tracks_f64 as tk
from tracks_cases import E2E, carry_hand_made, check_end_to_end, collect_calls, e2e_cfg, e2e_synth, runs_of_truth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 256


def _random_lists(rng, n, S, T):
    """Sparse random detections plus a few emitters that stay for a while (some with a neighbour they touch now and then), through the
    segments twin."""
    det = rng.random((T, n)) < rng.choice([0.004, 0.01, 0.02])
    for _ in range(int(rng.integers(1, 4))):
        lo, w, a, b = int(rng.integers(0, n)), int(rng.integers(1, 5)), int(rng.integers(0, T)), int(rng.integers(0, T + 1))
        on = (np.arange(T) >= min(a, b)) & (np.arange(T) <= max(a, b)) & (rng.random(T) < 0.85)
        det[np.ix_(on, (lo + np.arange(w)) % n)] = True
        if rng.random() < 0.5:                                # a neighbour two bins away, bridged now and then: carried tracks that merge
            det[np.ix_(on, (lo + w + 2 + np.arange(w)) % n)] = True
            det[np.ix_(on & (rng.random(T) < 0.08), (lo + w + np.arange(2)) % n)] = True
    P = rng.gamma(10.0, 1e-4, (T, n))
    return sg.run(det, P, 0, 1, S)


def test_twin_equals_the_whole_batch_twin_under_any_cut():
    rng = np.random.default_rng(2031)
    n_records = n_wide = n_bound = n_extra = 0
    for case in range(150):
        n, S = int(rng.choice([64, 256])), int(rng.choice([1, 4, 16]))
        slack, miss, mine = int(rng.choice([0, 1, 3])), int(rng.choice([0, 1, 3])), int(rng.choice([1, 2, 4]))
        T = int(rng.integers(1, 40))
        ep, segs = _random_lists(rng, n, S, T)
        chunks = []
        while sum(chunks) < T:
            chunks.append(min(int(rng.integers(1, 8)), T - sum(chunks)))
        big = T * S + 1
        st, whole, _ = tk.run(ep, segs, n, T, slack, miss, 1, big)                    # every component, then min_epochs by hand
        want = {(int(t["first_t"]), int(t["first_slot"])): t for t in whole[0, : st["n_stored"][0]]}
        calls = tc.run_cut(ep, segs, n, chunks, slack_bins=slack, max_miss=miss, min_epochs=mine, max_tracks=big)
        got = tc.closed_records(calls)
        assert sum(int(h["n_nodes"][0]) for h, *_ in calls) == st["n_nodes"][0]
        assert all(int(h["n_found"][0]) == int(h["n_stored"][0]) for h, *_ in calls)
        assert int(calls[-1][0]["n_open"][0]) == 0                                   # the flush leaves nothing open
        keys = [(int(g["first_t"]), int(g["first_slot"])) for g in got]
        assert len(set(keys)) == len(keys), "a component reported twice"
        for key, g in zip(keys, got):
            assert key in want, (case, key)
            w = want[key]
            n_records += 1
            span = int(w["last_t"]) - int(w["first_t"]) + 1
            bound = bool(g["flags"] & tc.HITS_UPPER_BOUND)
            n_bound += bound
            if w["n_epochs_hit"] < mine:
                assert bound, (case, key, "an extra record without bit 2")
                n_extra += 1
            if w["hi_off"] - w["lo_off"] >= n // 2:                                # exception (b): re-basing is exact below N/2 only
                n_wide += 1
                continue
            for f in tk.INT_FIELDS:
                if f == "n_epochs_hit" and bound:
                    assert w[f] <= g[f] <= span, (case, key, f, int(g[f]), int(w[f]), span)
                elif f == "flags":
                    assert g[f] & 3 == w[f] and g[f] & ~7 == 0, (case, key, int(g[f]), int(w[f]))
                else:
                    assert g[f] == w[f], (case, key, f, int(g[f]), int(w[f]))
            assert g["peak_power"] == w["peak_power"]
            assert abs(g["power_sum"] - w["power_sum"]) <= tk.POWER_TOL * abs(w["power_sum"])
            dc = abs(g["centre"] - w["centre"])
            assert min(dc, n - dc) <= n * tk.CENTRE_TOL, (case, key, float(g["centre"]), float(w["centre"]))
        missing = [k for k, w in want.items() if w["n_epochs_hit"] >= mine and k not in keys]
        assert not missing, (case, missing)
    print(f"{n_records} records, {n_bound} with bit 2 ({n_extra} of them kept by the bound alone), {n_wide} wider than N/2")
    assert n_records > 1000
    assert n_wide <= 0.02 * n_records and n_bound <= 0.10 * n_records                # the inputs stay inside the two stated exceptions


# ---- hand-made cases ----------------------------------------------------------------------------------------------------------
def _cut(E, per_epoch, chunks, S=4, flush_last=True, **kw):
    ep, segs = tk.make_lists(E, S, per_epoch)
    return tc.run_cut(ep, segs, N, chunks, flush_last=flush_last, **kw)


def _ints(t):
    return tuple(int(t[f]) for f in ("first_t", "last_t", "first_slot", "last_slot", "n_epochs_hit", "n_segments"))


def test_one_emitter_across_three_calls_is_one_record():
    calls = _cut(12, {e: [(10, 3)] for e in range(3, 10)}, [4, 4, 4], slack_bins=0)
    assert [(int(h["n_found"][0]), int(h["n_open"][0]), int(h["n_nodes"][0])) for h, *_ in calls] == [(0, 1, 1), (0, 1, 4), (1, 0, 2)]
    t = calls[2][1][0, 0]
    assert _ints(t) == (3, 9, 0, 0, 7, 7) and (t["lo_off"], t["hi_off"], t["width_sum"], t["flags"]) == (0, 2, 21, 0)
    assert t["power_sum"] == 7.0 and t["peak_power"] == 1.0 and t["centre"] == pytest.approx(11.0)
    # while it is open, d_open shows it as it stands, with bit 1
    o = calls[1][2][0, 0]
    assert _ints(o) == (3, 7, 0, 0, 5, 5) and o["flags"] == 2 and calls[1][0]["n_open_stored"][0] == 1


@pytest.mark.parametrize("chunks", [[4, 4], [5, 3], [3, 5], [1] * 8])
def test_gap_bridged_by_max_miss_on_a_cut(chunks):
    lists = {e: [(40, 2)] for e in (2, 3, 5, 6)}
    got = tc.closed_records(_cut(8, lists, chunks, slack_bins=0, max_miss=1))
    assert [_ints(t) for t in got] == [(2, 6, 0, 0, 4, 4)] and got[0]["flags"] == 2            # closed by the flush: 6 >= 8 - 1 - 1
    got = tc.closed_records(_cut(8, lists, chunks, slack_bins=0, max_miss=0))
    assert [_ints(t)[:2] for t in got] == [(2, 3), (5, 6)]


def test_calls_of_one_epoch_with_max_miss_3():
    """H = 4 epochs of tail, fed one epoch at a time: the tail is a shift register.  Members at 0, 4, 8: each gap is 3 misses."""
    calls = _cut(14, {0: [(7, 2)], 4: [(8, 2)], 8: [(7, 2)]}, [1] * 14, slack_bins=0, max_miss=3)
    emitted = [i for i, (h, *_) in enumerate(calls) if h["n_found"][0]]
    assert emitted == [12]                                     # T = 13: last_t 8 < 13 - 1 - 3
    t = calls[12][1][0, 0]
    assert _ints(t) == (0, 8, 0, 0, 3, 3) and t["flags"] == 1 and (t["lo_off"], t["hi_off"]) == (0, 2)
    assert [int(h["n_open"][0]) for h, *_ in calls] == [1] * 12 + [0, 0]
    got = tc.closed_records(_cut(14, {0: [(7, 2)], 5: [(8, 2)]}, [1] * 14, slack_bins=0, max_miss=3))
    assert [_ints(t)[:2] for t in got] == [(0, 0), (5, 5)]     # four misses are one too many


def test_two_carried_carriers_merged_by_one_wide_segment():
    lists = {e: [(10, 2), (20, 2)] for e in (0, 1, 2, 4, 5)}
    lists[3] = [(10, 12)]
    calls = _cut(6, lists, [3, 3], slack_bins=0)
    assert calls[0][0]["n_open"][0] == 2 and calls[0][0]["n_found"][0] == 0
    got = tc.closed_records(calls)
    assert len(got) == 1
    t = got[0]
    assert _ints(t) == (0, 5, 0, 0, 6, 11) and t["flags"] == 7                         # hits = min(3 + 3 + 3, span 6)
    assert (t["lo_off"], t["hi_off"], t["width_sum"]) == (0, 11, 32)
    # merged in the first call nothing is unknown: no bit 2
    got = tc.closed_records(_cut(6, lists, [4, 2], slack_bins=0))
    assert len(got) == 1 and _ints(got[0]) == (0, 5, 0, 0, 6, 11) and got[0]["flags"] == 3


def test_pairs_across_the_wrap_across_a_cut():
    got = tc.closed_records(_cut(2, {0: [(N - 1, 1, 1.0, 0.0)], 1: [(0, 1, 3.0, 0.0)]}, [1, 1], slack_bins=1))
    assert len(got) == 1 and (got[0]["lo_off"], got[0]["hi_off"], got[0]["power_sum"]) == (0, 1, 4.0)
    assert got[0]["centre"] == pytest.approx(N - 1 + 0.75)
    # two carried tracks either side of the wrap joined by a wrap-crossing segment: B (lo_root 1) is re-based by delta = +3 onto A
    # (lo_root N - 2)
    lists = {0: [(1, 1, 3.0, 0.0), (N - 2, 1, 1.0, 0.0)], 1: [(1, 1, 3.0, 0.0), (N - 2, 1, 1.0, 0.0)], 2: [(N - 2, 4, 1.0, 1.5)]}
    got = tc.closed_records(_cut(3, lists, [2, 1], slack_bins=0))
    assert len(got) == 1
    t = got[0]
    # the root is slot 0 of epoch 0, lo 1: A = the track at lo 1, B at N - 2 has delta = -3
    assert _ints(t) == (0, 2, 0, 0, 3, 5) and t["flags"] == 7 and (t["lo_off"], t["hi_off"]) == (-3, 0)
    assert t["power_sum"] == 9.0 and t["centre"] == pytest.approx((1 + (2 * 1.0 * -3 + 1.0 * (-3 + 1.5)) / 9.0) % N)
    whole = tk.run(*tk.make_lists(3, 4, lists), N, 3, 0, 0, 1, 8)[1][0, 0]
    assert t["centre"] == pytest.approx(whole["centre"]) and (t["lo_off"], t["hi_off"]) == (whole["lo_off"], whole["hi_off"])


def test_a_single_in_the_last_epoch_waits_for_the_next_call():
    calls = _cut(8, {3: [(100, 2)], 4: [(100, 2)]}, [4, 4], slack_bins=0, min_epochs=2)
    h = calls[0][0]
    assert (h["n_found"][0], h["n_open"][0], h["n_open_found"][0], h["n_open_stored"][0]) == (0, 1, 0, 0)
    assert [_ints(t) for t in tc.closed_records(calls)] == [(3, 4, 0, 0, 2, 2)]
    calls = _cut(8, {3: [(100, 2)]}, [4, 4], slack_bins=0, min_epochs=2)              # a false alarm after all
    assert calls[0][0]["n_open"][0] == 1 and not tc.closed_records(calls)


def test_flush_sets_bit_1():
    lists = {e: [(50, 4)] for e in range(4)}
    got = tc.closed_records(_cut(4, lists, [4], slack_bins=0))
    assert len(got) == 1 and got[0]["flags"] == 3
    calls = _cut(4, lists, [4], flush_last=False, slack_bins=0)
    h, tr, op = calls[0]
    assert (h["n_found"][0], h["n_open"][0], h["n_open_found"][0], h["n_open_stored"][0]) == (0, 1, 1, 1) and op[0, 0]["flags"] == 3
    assert not tr.tobytes().strip(b"\0")


def test_truncation_keeps_the_count():
    lists = {0: [(20 * k, 2) for k in range(4)], 1: [(20 * k, 2) for k in range(4)], 2: [(200, 1)]}
    h, tr, op = _cut(3, lists, [3], slack_bins=0, max_tracks=2)[0]
    assert (h["n_found"][0], h["n_stored"][0]) == (5, 2) and tr.shape == (1, 2) and [_ints(t)[:3] for t in tr[0]] == [(0, 1, 0), (0, 1, 1)]
    h, tr, op = _cut(3, lists, [3], flush_last=False, slack_bins=0, max_tracks=2)[0]
    assert (h["n_found"][0], h["n_open"][0], h["n_open_found"][0], h["n_open_stored"][0]) == (4, 1, 1, 1)


def test_a_carry_that_does_not_match_is_taken_as_empty():
    ep, segs = tk.make_lists(8, 4, {e: [(50, 4)] for e in range(8)})
    h, tr, op, states = tc.step(None, ep[:4], segs[:4], N, 4, 0, slack_bins=0)
    h2, tr2, *_ = tc.step(states, ep[4:], segs[4:], N, 4, 4, flush=1, slack_bins=0)
    assert h2["status"][0] == 0 and _ints(tr2[0, 0])[:2] == (0, 7)
    for kw, t0 in (({}, 5), ({"max_miss": 1}, 4)):
        h2, tr2, *_ = tc.step(states, ep[4:], segs[4:], N, 4, t0, flush=1, slack_bins=0, **kw)
        assert h2["status"][0] == 1 and _ints(tr2[0, 0])[:2] == (t0, t0 + 3)
    h2, tr2, *_ = tc.step(None, ep[4:], segs[4:], N, 4, 4, flush=1, slack_bins=0)
    assert h2["status"][0] == 1


def test_hand_made_lists_run_through_the_twin_and_match_the_whole_batch():
    for name, E, lists, chunks, kw in carry_hand_made(N):
        ep, segs = tk.make_lists(E, 4, lists)
        got = tc.closed_records(tc.run_cut(ep, segs, N, chunks, **{**kw, "max_tracks": 64}))
        st, whole, _ = tk.run(ep, segs, N, E, kw.get("slack_bins", 1), kw.get("max_miss", 0), kw.get("min_epochs", 1), 64)
        assert len(got) == st["n_found"][0], name
        for g, w in zip(sorted(got, key=lambda t: (t["first_t"], t["first_slot"])), whole[0]):
            for f in tk.INT_FIELDS:
                if f == "flags":
                    assert g[f] & 3 == w[f], (name, f)
                elif not (f == "n_epochs_hit" and g["flags"] & 4):
                    assert g[f] == w[f], (name, f, int(g[f]), int(w[f]))


# ---- the chain on the twins ---------------------------------------------------------------------------------------------------
def test_chain_on_the_twins_in_calls_of_8_epochs(built):
    """The traffic and the parameters of test_tracks_host.py's chain, the tracks stage fed 8 epochs at a time: every dwell run is
    exactly one record with the run's first and last global epoch, and no record carries bit 2."""
    import cfar_f64 as cf
    import oracle_py as orc
    cfg = e2e_cfg()
    n_streams, eps, step = 8, E2E["eps"], 8
    E = n_streams * eps
    iq, truth = orc.synth(cfg, e2e_synth(n_streams), E, cs.samples_per_epoch(cfg))
    P = orc.run(cfg, iq, E, want_spectrum=True)["spectrum"].astype(np.float64)
    det = cf.ratio(P, E2E["guard"], E2E["train"], cs.cfar_alpha(E2E["pfa"], E2E["k"], E2E["train"])) > 1.0
    ep, segs = sg.run(det, P, E2E["merge_gap"], E2E["min_width"], E2E["max_segments"])
    ep, segs = ep.reshape(n_streams, eps), segs.reshape(n_streams, eps, -1)
    streams, tracks = collect_calls(
        lambda states, t, flush: tc.step(states, ep[:, t:t + step].reshape(-1), segs[:, t:t + step].reshape(n_streams * step, -1), cfg.fft_len,
                                         step, t, flush, E2E["slack_bins"], E2E["max_miss"], E2E["min_epochs"], E2E["max_tracks"]),
        n_streams, eps, step)
    assert not (tracks["flags"] & tc.HITS_UPPER_BOUND).any()
    n_runs, n_other = check_end_to_end(cfg, truth.reshape(n_streams, eps), streams, tracks)
    assert n_runs == sum(len(runs_of_truth(r)) for r in truth.reshape(n_streams, eps))
    print(f"twins, {n_streams} streams x {eps} epochs in calls of {step}: {n_runs} dwell runs each one record, {n_other} other records")


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_symbols_structures_and_binding(built):
    L = cs.lib()
    for name in ("crn_tracks_carry_bytes", "crn_tracks_carry_workspace_bytes", "crn_tracks_carry_device"):
        assert name in cs.EXPORTS and hasattr(L, name)
    assert np.dtype(cs.TRACK_CARRY_STREAM_DTYPE).itemsize == 32
    assert (cs.TRACK_BEGAN_BEFORE, cs.TRACK_GOES_ON, cs.TRACK_HITS_UPPER_BOUND) == (1, 2, 4) == (tc.BEGAN_BEFORE, tc.GOES_ON, tc.HITS_UPPER_BOUND)
    hdr = open(os.path.join(ROOT, "include", "crn_sense.h")).read()
    body = re.search(r"typedef struct crn_track_carry_stream \{(.*?)\} crn_track_carry_stream;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [f.strip() for decl in body.split(";") if decl.strip() for f in re.sub(r"^\s*int32_t\s", "", decl.strip()).split(",")]
    assert names == list(np.dtype(cs.TRACK_CARRY_STREAM_DTYPE).names) == list(tc.CARRY_STREAM_F64.names)
    assert callable(cs.Sensor.tracks_carry_device)
    assert L.crn_abi_version() == cs.CRN_ABI_VERSION == 4      # additive: the ABI version stays
    engine = os.path.join(ROOT, "cognitive-radio-network_amd", "cognitive_engines", "CE_Predictive_Node_GPU", "crn_sense.h")
    assert open(engine).read() == hdr


def test_refusals_that_need_no_handle(built):
    L = cs.lib()
    q = cs.track_params(16, 4, 1, 0, 1, 64)
    buf = (C.c_uint8 * (1 << 20))()
    p = (C.addressof(buf) + 63) & ~63
    nb, cb = L.crn_tracks_carry_workspace_bytes(4, C.byref(q)), L.crn_tracks_carry_bytes(1, C.byref(q))
    assert 0 < nb <= (1 << 19) and 0 < cb <= (1 << 19)
    v = C.c_void_p
    assert L.crn_tracks_carry_device(None, v(p), v(p), 4, C.byref(q), 0, 0, v(p), cb, v(p), v(p), v(p), v(p), nb, None) == cs.CRN_ERR_ARG
    assert b"crn_tracks_carry_device" in L.crn_last_error()
    assert L.crn_tracks_carry_device(None, v(p), v(p), 0, C.byref(q), 0, 0, v(p), cb, v(p), v(p), None, v(p), nb, None) == cs.CRN_ERR_ARG
    assert L.crn_tracks_carry_device(None, None, None, -1, None, -1, 0, None, 0, None, None, None, None, 0, None) == cs.CRN_ERR_ARG


def test_size_functions(built):
    L = cs.lib()

    def q(S=16, eps=1, slack=1, miss=0, mine=1, mt=64, r0=0):
        p = cs.track_params(S, eps, slack, miss, mine, mt)
        p.reserved[0] = r0
        return p
    ws = lambda E, **kw: L.crn_tracks_carry_workspace_bytes(E, C.byref(q(**kw)))      # noqa: E731
    cb = lambda n, **kw: L.crn_tracks_carry_bytes(n, C.byref(q(**kw)))               # noqa: E731
    assert ws(0) > 0 and cb(0) > 0
    for f in (ws, cb):
        sizes = [f(E) for E in (1, 2, 64, 6656)]
        assert all(a > 0 for a in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
        sizes = [f(64, miss=m) for m in (0, 1, 3, 15)]
        assert all(a > 0 for a in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
        sizes = [f(64, S=S) for S in (1, 2, 16, 256)]
        assert all(a > 0 for a in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
        for bad in ({"S": 0}, {"S": 257}, {"eps": 0}, {"miss": -1}, {"miss": 16}, {"mine": 0}, {"mt": 0}, {"mt": 1025}, {"r0": 1}, {"slack": -1}):
            assert f(64, **bad) == -1, bad
        assert f(-1) == -1 and f(4, ) > 0
    assert ws(10, eps=3) == -1 and ws(2 ** 31, S=1) == -1 and ws(2 ** 23, S=256) == -1
    assert L.crn_tracks_carry_workspace_bytes(4, None) == -1 and L.crn_tracks_carry_bytes(4, None) == -1
    # room for every open track the definition allows: (max_miss + 1) x max_segments per stream
    assert cb(3, S=16, miss=3) >= 3 * 4 * 16 * 64
    assert cs.tracks_carry_bytes(3, 16, 3) == cb(3, S=16, miss=3)
    assert cs.tracks_carry_workspace_bytes(6656, 16, 104, 3) == ws(6656, eps=104, miss=3)
    with pytest.raises(cs.CrnError):
        cs.tracks_carry_workspace_bytes(10, 16, 3)
