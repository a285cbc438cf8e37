"""What the tracks tests share, on the host and on the GPU (test_tracks_host.py, test_tracks_carry_host.py, test_tracks_gpu.py,
test_tracks_carry_gpu.py): the parameters and the condition of the end-to-end case, the hand-made lists of the carried stage, and the
gathering of a sequence of calls.  A plain module, not collected."""
import numpy as np

import crnsense as cs
import tracks_f64 as tk

# The parameters of the end-to-end test, chosen on the twins (the chain of tests/test_tracks_host.py): the headline plan (N = 4096,
# K = 10, rectangular window), CRN_SIG_CW (one
# on-grid bin on the rectangular window, so min_width = 1 and no closing), CA-CFAR guard 2 / train 16 at Pfa 1e-6: with 4096 bins
# and 6656 epochs that leaves some tens of single-bin false alarms in the batch, and two of them in touching bins of consecutive
# epochs (which would make a second track of two epochs) are expected 6656 x 4096 x 3 x 1e-12 = 1e-4 times.
E2E = {"n": 4096, "k": 10, "guard": 2, "train": 16, "pfa": 1e-6, "merge_gap": 0, "min_width": 1, "max_segments": 16, "slack_bins": 1,
       "max_miss": 0, "min_epochs": 1, "max_tracks": 256, "signal_kind": cs.SIG_CW, "noise_power": 1e-6, "signal_rms": 0.02, "seed": 2027,
       "eps": 104}


def e2e_cfg():
    c = cs.cfg_energy_scaled(E2E["n"])
    c.window, c.hop, c.frames_per_epoch = cs.WINDOW_RECT, E2E["n"], E2E["k"]
    return c


def e2e_synth(n_streams):
    sc = cs.SynthCfg()
    sc.seed, sc.noise_power, sc.signal_rms = E2E["seed"], E2E["noise_power"], E2E["signal_rms"]
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = 8, cs.PU_MARKOV_INTENDED, E2E["signal_kind"], n_streams
    return sc


def band_of_bin(cfg, k):
    k = int(np.floor(k)) % cfg.fft_len
    for s in range(cfg.n_segs):
        if cfg.segs[s].lo <= k < cfg.segs[s].hi:
            return cfg.segs[s].band
    return -1


def runs_of_truth(truth_row):
    """[(band, first_t, last_t)] of the maximal runs of one stream's truth."""
    cuts = np.flatnonzero(np.diff(truth_row)) + 1
    starts, ends = np.r_[0, cuts], np.r_[cuts, truth_row.size]
    return [(int(truth_row[a]), int(a), int(b - 1)) for a, b in zip(starts, ends)]


def check_end_to_end(cfg, truth, streams, tracks):
    """The condition of the end-to-end test on one batch: truth [n_streams][eps]; streams / tracks as the kernel or the twin gives them.
    Returns (dwell runs, single-epoch other tracks)."""
    n_streams, eps = truth.shape
    n_runs = n_other = 0
    for st in range(n_streams):
        assert streams["n_found"][st] == streams["n_stored"][st], "max_tracks too small for this batch"
        trs = tracks[st, : streams["n_stored"][st]]
        bands = np.array([band_of_bin(cfg, t["centre"]) for t in trs])
        matched = np.zeros(trs.size, bool)
        seq = []
        for band, a, b in runs_of_truth(truth[st]):
            if band == 0:
                continue
            hit = np.flatnonzero((bands == band) & (trs["first_t"] == a) & (trs["last_t"] == b))
            assert hit.size == 1, (st, band, a, b, hit, [(int(t["first_t"]), int(t["last_t"]), float(t["centre"])) for t in trs])
            matched[hit[0]] = True
            seq.append((int(trs["first_t"][hit[0]]), band, b - a + 1))
            n_runs += 1
        assert (trs["n_epochs_hit"][~matched] == 1).all(), (st, trs[~matched])
        n_other += int((~matched).sum())
        # the 3 x 3 transition counts rebuilt from the matched tracks in time order against those counted in the truth
        seq.sort()
        got = np.zeros((4, 4), np.int64)
        for i, (_, band, length) in enumerate(seq):
            got[band, band] += length - 1
            if i + 1 < len(seq):
                got[band, seq[i + 1][1]] += 1
        want = np.zeros((4, 4), np.int64)
        np.add.at(want, (truth[st][:-1], truth[st][1:]), 1)
        assert (got == want).all(), (st, got, want)
    return n_runs, n_other


def carry_hand_made(n):
    """(name, E, {epoch: [(lo, width[, power, centroid, peak])]}, the calls' lengths, parameters): the lists of the hand-made cases of
    tests/test_tracks_carry_host.py at size n, for tests/test_tracks_carry_gpu.py to upload (4 slots per epoch); the answers are asserted
    there, on the GPU the kernel must equal the twin."""
    merge = {e: [(10, 2), (20, 2)] for e in (0, 1, 2, 4, 5)}
    merge[3] = [(10, 12)]
    wrap = {0: [(1, 1, 3.0, 0.0), (n - 2, 1, 1.0, 0.0)], 1: [(1, 1, 3.0, 0.0), (n - 2, 1, 1.0, 0.0)], 2: [(n - 2, 4, 1.0, 1.5)]}
    four = {0: [(20 * k, 2) for k in range(4)], 1: [(20 * k, 2) for k in range(4)], 2: [(200, 1)]}
    return [("one emitter across three calls", 12, {e: [(10, 3, 2.0 + e, 0.5 * e % 3, 1.0 + e)] for e in range(3, 10)}, [4, 4, 4], dict(slack_bins=0)),
            ("gap on the cut", 8, {e: [(40, 2)] for e in (2, 3, 5, 6)}, [4, 4], dict(slack_bins=0, max_miss=1)),
            ("gap before the cut", 8, {e: [(40, 2)] for e in (2, 3, 5, 6)}, [5, 3], dict(slack_bins=0, max_miss=1)),
            ("gap, no miss allowed", 8, {e: [(40, 2)] for e in (2, 3, 5, 6)}, [4, 4], dict(slack_bins=0, max_miss=0)),
            ("calls of one epoch, max_miss 3", 14, {0: [(7, 2)], 4: [(8, 2)], 8: [(7, 2)]}, [1] * 14, dict(slack_bins=0, max_miss=3)),
            ("four misses", 14, {0: [(7, 2)], 5: [(8, 2)]}, [1] * 14, dict(slack_bins=0, max_miss=3)),
            ("two carried carriers merged", 6, merge, [3, 3], dict(slack_bins=0)), ("merged within a call", 6, merge, [4, 2], dict(slack_bins=0)),
            ("pair across the wrap", 2, {0: [(n - 1, 1, 1.0, 0.0)], 1: [(0, 1, 3.0, 0.0)]}, [1, 1], dict(slack_bins=1)),
            ("carried tracks joined across the wrap", 3, wrap, [2, 1], dict(slack_bins=0)),
            ("a single waits", 8, {3: [(100, 2)], 4: [(100, 2)]}, [4, 4], dict(slack_bins=0, min_epochs=2)),
            ("a false alarm", 8, {3: [(100, 2)]}, [4, 4], dict(slack_bins=0, min_epochs=2)),
            ("flush", 4, {e: [(50, 4)] for e in range(4)}, [4], dict(slack_bins=0)), ("truncation", 3, four, [3], dict(slack_bins=0, max_tracks=2)),
            ("truncation of the open list", 6, {e: [(20 * k, 2) for k in range(4)] for e in range(6)}, [2, 2, 2], dict(slack_bins=0, max_tracks=2)),
            ("width N", 4, {0: [(0, n)], 1: [(77, 1), (200, 3)], 2: [(77, 1)], 3: [(0, n)]}, [1, 2, 1], dict(slack_bins=0)),
            ("zero power", 3, {e: [(9, 2, 0.0, 0.0, 0.0)] for e in range(3)}, [1, 1, 1], dict(slack_bins=0)),
            ("nothing at all", 6, {}, [3, 3], dict(slack_bins=1, max_miss=1))]


def collect_calls(call, n_streams, eps, step, dtype=tk.TRACK_F64):
    """Runs call(states, t_start, flush) -> (headers, tracks, open, states) over eps epochs in calls of `step` and gathers every
    stream's closed records into (streams, tracks) as check_end_to_end takes them."""
    per_stream, states = [[] for _ in range(n_streams)], None
    for t in range(0, eps, step):
        h, tr, _, states = call(states, t, int(t + step >= eps))
        for k in range(n_streams):
            assert h["n_found"][k] == h["n_stored"][k]
            per_stream[k] += [tr[k, i] for i in range(int(h["n_stored"][k]))]
    most = max(1, max(len(r) for r in per_stream))
    streams, tracks = np.zeros(n_streams, tk.STREAM_F64), np.zeros((n_streams, most), dtype)
    for k, recs in enumerate(per_stream):
        streams["n_found"][k] = streams["n_stored"][k] = len(recs)
        for i, r in enumerate(recs):
            tracks[k, i] = r
    return streams, tracks
