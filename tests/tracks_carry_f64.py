"""The float64 twin of crn_tracks_carry_device, written from the incremental rule in include/crn_sense.h ("tracks carried across
batches", items 1-10), not from the kernels.  The state is plain Python: per stream a dict with the mark (max_segments, max_miss,
fft_len, T), the tail (the last max_miss + 1 epochs' lists of (lo, width, position of the open track)) and the open tracks in ascending
root order, each a dict of accumulators.  One call:

  nodes   the open tracks in carry order, then the tail segments, then the new stored segments by (t, slot);
  unions  every tail segment with its open track; step 2's link condition between a tail or new segment and a NEW segment 1 .. H
          epochs later; the root of a component is its smallest node;
  sums    a component rooted at carried track A starts from A; every further carried track B adds itself re-based by
          delta = ((lo_root_B - lo_root_A + N/2) mod N) - N/2; new segments add with their offset from the root's lo_root; tail
          segments add nothing; distinct new epochs add to the hits; two or more carried tracks in one component set the merged bit
          (flag bit 2), and a merged track's hits are min(sum, last_t - first_t + 1);
  split   open (last_t >= T - 1 - max_miss and no flush) go to the new carry, closed ones with hits >= min_epochs are emitted.

`step` gives the three arrays in the kernel's layout with the float fields kept in float64, and the new state."""
import numpy as np

import tracks_f64 as tk

CARRY_STREAM_F64 = np.dtype([("n_found", "<i4"), ("n_stored", "<i4"), ("n_nodes", "<i4"), ("n_open", "<i4"), ("n_open_found", "<i4"),
                             ("n_open_stored", "<i4"), ("status", "<i4"), ("reserved", "<i4")])
BEGAN_BEFORE, GOES_ON, HITS_UPPER_BOUND = 1, 2, 4


def _empty(S, max_miss, n, T):
    return {"S": S, "max_miss": max_miss, "n": n, "T": T, "tail": [[] for _ in range(max_miss + 1)], "open": []}


def _record(out, a, n, max_miss, T):
    out["first_t"], out["first_slot"], out["last_t"], out["last_slot"] = a["root_t"], a["root_slot"], a["last"][0], -a["last"][1]
    out["n_epochs_hit"], out["n_segments"], out["lo_off"], out["hi_off"] = a["hits"], a["nseg"], a["lo_off"], a["hi_off"]
    out["width_sum"], out["power_sum"], out["peak_power"] = a["width_sum"], a["power"], a["peak"]
    out["centre"] = (a["lo_root"] + (a["moment"] / a["power"] if a["power"] > 0 else 0.0)) % n
    out["flags"] = ((BEGAN_BEFORE if a["root_t"] <= max_miss else 0) | (GOES_ON if a["last"][0] >= T - 1 - max_miss else 0) |
                    (HITS_UPPER_BOUND if a["merged"] else 0))


def _one_stream(state, n_stored, segs, n, t_start, flush, slack_bins, max_miss, min_epochs):
    """state: the stream's carry (already checked against the mark); n_stored [eps], segs [eps][S].  Returns (closed accumulators in
    root order, open accumulators in root order, the new state)."""
    eps, S = segs.shape
    H, T, half = max_miss + 1, t_start + eps, n // 2
    G = len(state["open"])
    # rows of (lo, width) lists at the times t_start - H .. T - 1: the tail, then the new epochs
    lo, width = segs["lo"].astype(np.int64), segs["width"].astype(np.int64)
    power, peak, centroid = segs["power"].astype(np.float64), segs["peak_power"].astype(np.float64), segs["centroid"].astype(np.float64)
    rows = [[(g[0], g[1]) for g in state["tail"][j]] for j in range(H)]
    rows += [[(int(lo[e, s]), int(width[e, s])) for s in range(int(n_stored[e]))] for e in range(eps)]
    base = np.concatenate(([G], G + np.cumsum([len(r) for r in rows]))).astype(np.int64)      # first node of each row
    find, union = tk.union_find(int(base[-1]))
    for j in range(H):
        for s, g in enumerate(state["tail"][j]):
            union(int(base[j]) + s, g[2])
    arr = [(np.array([g[0] for g in r], np.int64), np.array([g[1] for g in r], np.int64)) for r in rows]
    for jb in range(H, H + eps):
        if not rows[jb]:
            continue
        for d in range(1, H + 1):
            ja = jb - d
            if ja < 0 or not rows[ja]:
                continue
            hit = tk.linked(arr[ja][0][:, None], arr[ja][1][:, None], arr[jb][0][None, :], arr[jb][1][None, :], n, slack_bins)
            for a, b in np.argwhere(hit):
                union(int(base[ja]) + int(a), int(base[jb]) + int(b))
    # the components' accumulators, keyed by root
    acc, new_epochs = {}, {}
    for g in range(G):
        r = find(g)
        b = state["open"][g]
        if r == g:
            acc[r] = dict(b, n_carried=1)
            continue
        a = acc[r]
        delta = (b["lo_root"] - a["lo_root"] + half) % n - half
        a["lo_off"], a["hi_off"] = min(a["lo_off"], b["lo_off"] + delta), max(a["hi_off"], b["hi_off"] + delta)
        a["moment"] += b["moment"] + delta * b["power"]
        for f in ("hits", "nseg", "width_sum", "power"):
            a[f] += b[f]
        a["peak"], a["last"] = max(a["peak"], b["peak"]), max(a["last"], b["last"])
        a["merged"] = a["merged"] or b["merged"]
        a["n_carried"] += 1
    for e in range(eps):
        t = t_start + e
        for s in range(len(rows[H + e])):
            i = int(base[H + e]) + s
            r = find(i)
            if r not in acc:                                  # a component without a carried track: r is its first new node
                assert r == i
                acc[r] = {"root_t": t, "root_slot": s, "lo_root": int(lo[e, s]), "last": (-1, 0), "hits": 0, "nseg": 0, "lo_off": 2 ** 62,
                          "hi_off": -2 ** 62, "width_sum": 0, "power": 0.0, "moment": 0.0, "peak": 0.0, "merged": False, "n_carried": 0}
            a = acc[r]
            off = (int(lo[e, s]) - a["lo_root"] + half) % n - half
            a["nseg"] += 1
            a["last"] = max(a["last"], (t, -s))                # the latest epoch, there the lowest slot
            a["lo_off"], a["hi_off"] = min(a["lo_off"], off), max(a["hi_off"], off + int(width[e, s]) - 1)
            a["width_sum"] += int(width[e, s])
            a["power"] += power[e, s]
            a["moment"] += power[e, s] * (off + centroid[e, s])
            a["peak"] = max(a["peak"], peak[e, s])
            new_epochs.setdefault(r, set()).add(t)
    closed, opened, position = [], [], {}
    for r in sorted(acc):
        a = acc[r]
        a["hits"] += len(new_epochs.get(r, ()))
        if a["n_carried"] >= 2:
            a["merged"] = True
        if a["merged"]:
            a["hits"] = min(a["hits"], a["last"][0] - a["root_t"] + 1)
        del a["n_carried"]
        if not flush and a["last"][0] >= T - 1 - max_miss:
            position[r] = len(opened)
            opened.append(a)
        else:
            closed.append(a)
    new = _empty(S, max_miss, n, T)
    if not flush:
        new["open"] = opened
        for j in range(H):                                    # the times T - H .. T - 1 are rows eps .. eps + H - 1
            new["tail"][j] = [(g[0], g[1], position[find(int(base[j + eps]) + s)]) for s, g in enumerate(rows[j + eps])]
        assert all(any(g[2] == k for row in new["tail"] for g in row) for k in range(len(opened))), "an open track without a tail segment"
    return closed, opened, new


def step(states, epochs, segments, n, epochs_per_stream, t_start, flush=0, slack_bins=1, max_miss=0, min_epochs=1, max_tracks=64,
         want_open=True):
    """One call.  states: None or a list of per-stream states as an earlier call returned them; epochs [E] / segments [E][S] as
    crn_segments_device wrote them (any dtype with the fields of tracks_f64.run).
    Returns (headers [n_streams] CARRY_STREAM_F64, tracks [n_streams][max_tracks] TRACK_F64, open [n_streams][max_tracks] TRACK_F64,
    new states)."""
    E, S = segments.shape
    eps = epochs_per_stream
    assert eps >= 1 and E % eps == 0 and t_start >= 0
    n_streams = E // eps
    n_stored = np.clip(np.asarray(epochs["n_stored"], np.int64), 0, S)
    headers = np.zeros(n_streams, CARRY_STREAM_F64)
    tracks, opens = np.zeros((n_streams, max_tracks), tk.TRACK_F64), np.zeros((n_streams, max_tracks), tk.TRACK_F64)
    new_states = []
    for k in range(n_streams):
        st = states[k] if states is not None and k < len(states) else None
        if t_start == 0:
            st = _empty(S, max_miss, n, 0)
        elif st is None or (st["S"], st["max_miss"], st["n"], st["T"]) != (S, max_miss, n, t_start):
            st = _empty(S, max_miss, n, t_start)
            headers["status"][k] = 1
        sl = slice(k * eps, (k + 1) * eps)
        closed, opened, new = _one_stream(st, n_stored[sl], segments[sl], n, t_start, flush, slack_bins, max_miss, min_epochs)
        new_states.append(new)
        T = t_start + eps
        found = [a for a in closed if a["hits"] >= min_epochs]
        open_found = [a for a in opened if a["hits"] >= min_epochs]
        headers[k]["n_found"], headers[k]["n_stored"], headers[k]["n_nodes"] = len(found), min(len(found), max_tracks), n_stored[sl].sum()
        headers[k]["n_open"], headers[k]["n_open_found"] = len(opened), len(open_found)
        headers[k]["n_open_stored"] = min(len(open_found), max_tracks) if want_open else 0
        for i, a in enumerate(found[:max_tracks]):
            _record(tracks[k, i], a, n, max_miss, T)
        if want_open:
            for i, a in enumerate(open_found[:max_tracks]):
                _record(opens[k, i], a, n, max_miss, T)
    return headers, tracks, opens, new_states


def run_cut(epochs, segments, n, chunks, flush_last=True, **kw):
    """One stream's lists (epochs [T], segments [T][S]) fed in calls of the lengths `chunks` from t_start = 0.  Returns the list of
    (headers, tracks, open) per call; the last call flushes when flush_last."""
    out, states, t = [], None, 0
    for i, c in enumerate(chunks):
        h, tr, op, states = step(states, epochs[t:t + c], segments[t:t + c], n, c, t, flush=int(flush_last and i == len(chunks) - 1), **kw)
        out.append((h, tr, op))
        t += c
    assert t == len(epochs)
    return out


def closed_records(calls, stream=0):
    """The stored closed records of a list of (headers, tracks, ...) in the order they were emitted."""
    return [tr[stream, i].copy() for h, tr, *_ in calls for i in range(int(h["n_stored"][stream]))]


HEADER_FIELDS = CARRY_STREAM_F64.names


def compare(got_headers, got_tracks, got_open, want_headers, want_tracks, want_open, n):
    """The kernel's three arrays against step()'s: headers equal; the closed and the open records by tracks_f64.compare (every integer
    field, flags, peak bits, zero fill equal; power_sum and centre within its tolerances).  got_open None: not asked for."""
    for f in HEADER_FIELDS:
        assert (got_headers[f] == want_headers[f]).all(), (f, got_headers[f][:8], want_headers[f][:8])
    p, c = tk.compare(got_headers, got_tracks, None, want_headers, want_tracks, None, n)
    if got_open is not None:
        as_streams = np.zeros(len(want_headers), tk.STREAM_F64)
        as_streams["n_found"], as_streams["n_stored"], as_streams["n_nodes"] = (want_headers["n_open_found"], want_headers["n_open_stored"],
                                                                                want_headers["n_nodes"])
        p2, c2 = tk.compare(as_streams, got_open, None, as_streams, want_open, None, n)
        p, c = max(p, p2), max(c, c2)
    return p, c
