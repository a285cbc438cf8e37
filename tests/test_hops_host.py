"""Hop counts without a GPU: the twin (tests/hops_twin.py) and its identities, its cut independence, crn_hop_forecast in C against the
Python, every refusal of the functions that need no device, and what the records are for: the hop table of a user that dwells and jumps,
and channel picks under the interferer's sweep against the per-channel rule of crnsense.best_channel."""
import ctypes as C

import numpy as np
import pytest

import channels_f64 as ch
import crnsense as cs
import hops_cases as hc
import hops_twin as ht


def _rec(r, n_lags):
    return cs.hop_record(r.tobytes(), n_lags)


# ---- the twin ---------------------------------------------------------------------------------------------------------------------
def test_by_hand():
    """CH0, CH0, CH1, nothing, CH1 with lags 1 and 2, every count by hand."""
    r = ht.sequence([1, 1, 2, 0, 2], 2, (1, 2))
    assert int(r["n_epochs"]) == 5 and r["lag"].tolist() == [1, 2, 0, 0, 0, 0, 0, 0] and (int(r["n_channels"]), int(r["n_lags"])) == (2, 2)
    hop = np.zeros((64, 64), int)
    hop[0, 1] = hop[1, 63] = hop[63, 1] = 1
    assert (r["hop"] == hop).all()
    pair = np.zeros((2, 64, 64), int)
    pair[0, 0, 0] = pair[0, 0, 1] = pair[0, 1, 63] = pair[0, 63, 1] = 1           # 0>0, 0>1, 1>idle, idle>1
    pair[1, 0, 1] = pair[1, 0, 63] = pair[1, 1, 1] = 1                            # two epochs on: 0>1, 0>idle, 1>1
    assert (r["lags"]["pair"] == pair).all()
    assert (r["lags"]["from"] == pair.sum(axis=2)).all() and (r["lags"]["to"] == pair.sum(axis=1)).all()
    # hist: bit k = k epochs before the last; channel 1 was busy in the last epoch and two before it, channel 0 three and four before
    assert int(r["hist"][1]) == 0b00101 and int(r["hist"][0]) == 0b11000 and int(r["hist"][63]) == 0b00010 and not r["hist"][2:63].any()


@pytest.mark.parametrize("C_", [1, 3, 63])
def test_identities_with_one_bit_per_word(C_):
    rng = np.random.default_rng(C_)
    lags = (1, 2, 5, 64)
    for T in (1, 2, 5, 64, 65, 150):
        w = hc.words("chain", T, C_, rng)
        r = ht.sequence(w, C_, lags)
        for m, d in enumerate(lags):
            pair = r["lags"]["pair"][m]
            assert pair.sum() == max(0, T - d), (T, d)
            assert (r["lags"]["from"][m] == pair.sum(axis=1)).all() and (r["lags"]["to"][m] == pair.sum(axis=0)).all()
        assert np.trace(r["hop"]) == 0 and r["hop"].sum() <= T - 1
        states = [ht.augment(x, C_).bit_length() - 1 for x in w.tolist()]
        assert r["hop"].sum() == sum(a != b for a, b in zip(states[:-1], states[1:]))


def test_the_twin_is_cut_independent():
    rng = np.random.default_rng(9)
    lags, C_, T = (1, 3, 64), 5, 193
    for kind in ("chain", "d0.5", "high"):
        w = np.concatenate([hc.words(kind, T, C_, rng), hc.words(kind, T, C_, rng)])
        whole = ht.update(None, w, C_, lags, T, True)
        rec, at = None, 0
        for n in (1, 2, 61, 1, 64, 64):
            part = np.concatenate([w[at: at + n], w[T + at: T + at + n]])
            rec = ht.update(None if rec is None else rec.tobytes(), part, C_, lags, n, at == 0)
            at += n
        assert rec.tobytes() == whole.tobytes(), kind


def test_the_carry_as_the_rule_reads_it():
    lags, C_ = (1, 2), 3
    dt = ht.dtype(2)
    w = np.array([1, 2, 4, 2, 1], np.uint64)
    fresh = ht.update(None, w, C_, lags, 5, True)
    # 0xFF bytes, another n_channels, another lag: all taken as empty
    for spoil in ("ff", "nch", "lag", "n0"):
        old = ht.update(None, w, C_, lags, 5, True)
        if spoil == "ff":
            old = np.frombuffer(b"\xff" * dt.itemsize, dt).copy()
        elif spoil == "nch":
            old["n_channels"] = 4
        elif spoil == "lag":
            old["lag"][0, 2] = 7
        else:
            old["n_epochs"] = 0
        assert ht.update(old.tobytes(), w, C_, lags, 5, False).tobytes() == fresh.tobytes(), spoil
    # a valid head over counts at 2^31 - 2, negative counts and hist bits outside the mask
    old = ht.update(None, w, C_, lags, 5, True)
    old["hop"][0, 0, 1], old["hop"][0, 1, 0] = ht.SAT - 1, -5
    old["hist"][0, 10], old["hist"][0, 0] = 0xFFFF, int(old["hist"][0, 0]) | 0xFF00
    new = ht.update(old.tobytes(), np.array([2, 1, 2, 1, 2], np.uint64), C_, lags, 5, False)[0]
    assert new["hop"][0, 1] == ht.SAT and new["hop"][1, 0] == 2 and int(new["n_epochs"]) == 10 and new["hist"][10] == 0


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
def test_symbols_structures_and_binding(built):
    L = cs.lib()
    for name in ("crn_hops_bytes", "crn_hops_workspace_bytes", "crn_hops_device", "crn_hop_forecast"):
        assert name in cs.EXPORTS and hasattr(L, name)
    assert C.sizeof(cs.HopParams) == 64
    for n_lags in range(1, 9):
        assert cs.hop_dtype(n_lags) == ht.dtype(n_lags) and ht.dtype(n_lags).itemsize == ht.record_bytes(n_lags) == 64 + 512 + 16384 + n_lags * 16896
        assert cs.hops_bytes(3, 5, tuple(range(1, n_lags + 1))) == 3 * ht.record_bytes(n_lags)
    assert callable(cs.Sensor.hops_device) and L.crn_abi_version() == cs.CRN_ABI_VERSION == 4     # additive: the ABI version stays
    q = cs.hop_params(5, 100, (1, 2, 64), True)
    assert (q.n_channels, q.epochs_per_stream, q.n_lags, q.first, list(q.lag), list(q.reserved)) == (5, 100, 3, 1, [1, 2, 64, 0, 0, 0, 0, 0], [0] * 4)
    with pytest.raises(ValueError):
        cs.hop_params(5, 100, range(1, 10))
    with pytest.raises(ValueError):
        cs.hop_record(b"\0" * 100, 1)


def _q(nch=5, eps=4, lags=(1, 2), first=0, r=None, n_lags=None):
    q = cs.hop_params(nch, eps, lags, first)
    if r is not None:
        q.reserved[r] = 1
    if n_lags is not None:
        q.n_lags = n_lags
    return q


BAD_PARAMS = ({"nch": 0}, {"nch": 64}, {"nch": -1}, {"n_lags": 0}, {"n_lags": 9}, {"n_lags": -1}, {"lags": (0,)}, {"lags": (65,)}, {"lags": (-1, 2)},
              {"lags": (2, 2)}, {"lags": (3, 2)}, {"lags": (1, 2, 3, 3)}, {"lags": (1, 64, 65)}, {"eps": 0}, {"eps": -4}, {"r": 0}, {"r": 3})


def test_refusals_of_the_size_functions(built):
    L = cs.lib()
    assert L.crn_hops_bytes(0, C.byref(_q())) == 0 and L.crn_hops_bytes(2, C.byref(_q())) == 2 * ht.record_bytes(2)
    assert L.crn_hops_workspace_bytes(0, C.byref(_q())) > 0 and L.crn_hops_workspace_bytes(0, C.byref(_q(first=1))) > 0
    sizes = [L.crn_hops_workspace_bytes(E, C.byref(_q(eps=E))) for E in (1, 64, 65, 6656, 100000)]
    assert all(a > 0 for a in sizes) and sizes == sorted(sizes) and sizes[-1] > sizes[0]
    assert L.crn_hops_workspace_bytes(6656, C.byref(_q(eps=104))) == cs.hops_workspace_bytes(6656, 5, 104, (1, 2))
    # the longest stream the parameters can name: a bounded number of parts, so the size stays small
    big = 2 ** 31 - 1
    assert 0 < L.crn_hops_workspace_bytes(big, C.byref(_q(eps=big))) < 2 ** 24
    # unused lag entries are not looked at
    q = _q()
    q.lag[5] = 99
    assert L.crn_hops_bytes(1, C.byref(q)) == ht.record_bytes(2) and L.crn_hops_workspace_bytes(8, C.byref(q)) > 0
    for bad in BAD_PARAMS:
        assert L.crn_hops_bytes(2, C.byref(_q(**bad))) == -1, bad
        assert L.crn_hops_workspace_bytes(8 if "eps" not in bad else 0, C.byref(_q(**bad))) == -1, bad
    assert L.crn_hops_bytes(-1, C.byref(_q())) == -1 and L.crn_hops_workspace_bytes(-1, C.byref(_q())) == -1
    assert L.crn_hops_workspace_bytes(10, C.byref(_q(eps=3))) == -1
    assert L.crn_hops_bytes(2, None) == -1 and L.crn_hops_workspace_bytes(8, None) == -1
    with pytest.raises(cs.CrnError):
        cs.hops_workspace_bytes(10, 5, 3)
    with pytest.raises(cs.CrnError):
        cs.hops_bytes(1, 64)


def test_no_handle_is_refused_before_anything_is_looked_at(built):
    L = cs.lib()
    buf = (C.c_uint8 * 65536)()
    p = (C.addressof(buf) + 63) & ~63
    q = _q()
    assert L.crn_hops_device(None, p, 8, C.byref(q), p, 2 ** 20, p, 2 ** 20, None) == cs.CRN_ERR_ARG
    assert b"crn_hops_device" in L.crn_last_error()
    assert L.crn_hops_device(None, None, -1, None, None, 0, None, 0, None) == cs.CRN_ERR_ARG
    assert not bytes(buf).strip(b"\0")


def test_forecast_in_c_against_the_python(built):
    rng = np.random.default_rng(17)
    for C_, lags in ((1, (1,)), (4, (1, 2, 3)), (63, (1, 2, 3, 5, 8, 13, 63, 64))):
        r = np.zeros(1, ht.dtype(len(lags)))[0]
        r["n_epochs"], r["n_channels"], r["n_lags"] = 1000, C_, len(lags)
        r["lag"][:len(lags)] = lags
        r["lags"]["pair"] = rng.integers(0, 50, r["lags"]["pair"].shape)
        r["lags"]["from"] = r["lags"]["pair"].sum(axis=2) + rng.integers(0, 3, r["lags"]["from"].shape)
        r["lags"]["from"][:, 0], r["lags"]["pair"][:, 0] = 0, 0                 # a state never seen: 0 / 0
        r["lags"]["pair"][0, C_ - 1, 0] = -7                                      # a negative count is read as 0
        rec = _rec(r, len(lags))
        several = (1 << C_) - 1 if C_ < 63 else 0x5A5A5A5A5A5A5A5A | 1 | 1 << 62          # (channels 0 and C - 1 among them)
        for m in range(len(lags)):
            for word in (1, 1 << (C_ - 1), 0, several, (1 << 63) | (1 << C_), 3):
                for prior in (0.0, 1.0, 0.25):
                    got, want = cs.hop_forecast(rec, m, word, prior), ht.forecast(r, m, word, prior)
                    assert got == pytest.approx(want, rel=1e-12, abs=0), (C_, m, word, prior)
                    assert not got[C_:63].any()
        assert cs.hop_forecast(rec, 0, 1, 0.0)[0] == 0.5 and cs.hop_forecast(rec, 0, 1, 0.0)[63] == 0.5       # 0 / 0
        # the most threatening of several emitters
        two = cs.hop_forecast(rec, 0, several, 1.0)
        assert (two >= cs.hop_forecast(rec, 0, 1, 1.0)).all() and (two >= cs.hop_forecast(rec, 0, 1 << (C_ - 1), 1.0)).all()


def test_forecast_refusals(built):
    L = cs.lib()
    r = np.zeros(1, ht.dtype(2))
    r["n_channels"], r["n_lags"] = 3, 2
    raw = np.frombuffer(r.tobytes(), np.uint8).copy()
    ptr = raw.ctypes.data_as(C.c_void_p)
    p = (C.c_double * 64)(*([-1.0] * 64))
    assert L.crn_hop_forecast(ptr, 1, 1, 1.0, p) == 0 and p[0] == 0.5
    p[0] = -1.0
    assert L.crn_hop_forecast(None, 0, 1, 1.0, p) == cs.CRN_ERR_ARG and b"crn_hop_forecast" in L.crn_last_error()
    assert L.crn_hop_forecast(ptr, 0, 1, 1.0, None) == cs.CRN_ERR_ARG
    for m, prior in ((-1, 1.0), (2, 1.0), (8, 1.0), (0, -0.5), (0, float("nan")), (0, float("inf")), (0, float("-inf"))):
        assert L.crn_hop_forecast(ptr, m, 1, prior, p) == cs.CRN_ERR_ARG, (m, prior)
    for field, v in (("n_channels", 0), ("n_channels", 64), ("n_channels", -1), ("n_lags", 0), ("n_lags", 9)):
        bad = r.copy()
        bad[field] = v
        raw = np.frombuffer(bad.tobytes(), np.uint8).copy()
        assert L.crn_hop_forecast(raw.ctypes.data_as(C.c_void_p), 0, 1, 1.0, p) == cs.CRN_ERR_ARG, (field, v)
    assert p[0] == -1.0
    with pytest.raises(cs.CrnError):
        cs.hop_forecast(_rec(r[0], 2), 2, 1)


# ---- what the records are for -----------------------------------------------------------------------------------------------------
def test_hop_table_of_a_user_that_dwells_and_jumps():
    """A user on three channels that stays 20 epochs and then jumps by the intended Markov table with its diagonal removed and rows
    renormalised, 3000 jumps; 2 % of the epochs show nothing busy.  A flickered epoch is a move to the idle state and back, and one on a
    jump's seam takes that jump through the idle state, so the rows are compared over the channels: hop_table's row without its idle
    column, renormalised, against the jump table, each cell within 4.5 binomial standard deviations sqrt(p (1 - p) / n), n the row's
    channel-to-channel jumps (six cells at once: a correct implementation fails with probability about 1e-4).  The diagonal is exactly
    0: stays are left out."""
    rng = np.random.default_rng(2026)
    w, left = hc.dwelling_user(rng, hc.TABLE, 3000, 20, 0.02)
    r = ht.sequence(w, 3, (1,))
    rec = _rec(r, 1)
    tbl = cs.hop_table(rec)
    assert tbl.shape == (4, 4) and np.allclose(tbl.sum(axis=1), 1.0) and not np.diag(tbl).any()
    want = hc.jump_table(hc.TABLE)
    worst = 0.0
    for i in range(3):
        n = int(rec["hop"][i, :3].sum())
        est = tbl[i, :3] / tbl[i, :3].sum()
        sd = np.sqrt(want[i] * (1 - want[i]) / n)
        assert n >= 0.9 * left[i], (i, n, left[i])                                # 2 % flicker loses about 4 % of the jumps
        for j in range(3):
            if i != j:
                worst = max(worst, abs(est[j] - want[i, j]) / sd[j])
                assert abs(est[j] - want[i, j]) <= 4.5 * sd[j], (i, j, est[j], want[i, j], sd[j], n)
        print(f"CH{i + 1}: {n} jumps ({left[i]} made), to {np.round(est, 4).tolist()} against {np.round(want[i], 4).tolist()}, 4.5 sd = {np.round(4.5 * sd, 3).tolist()}")
    print(f"worst cell {worst:.2f} standard deviations; idle column {np.round(tbl[:3, 3], 3).tolist()}, idle row {np.round(tbl[3, :3], 3).tolist()}")
    # prior > 0 fills the cells off the diagonal only
    assert not np.diag(cs.hop_table(rec, 1.0)).any() and (cs.hop_table(rec, 1.0)[:3, :3] + np.eye(3) > 0).all()


def test_picks_under_the_sweep(built):
    """The interferer's sweep over 8 channels, 1, 2, .., 8, 7, .., 2, .., 560 epochs.  The hop record (lags 1, 2, 3) is learnt on the first
    half; on the second half next_channel picks at horizons 2 and 3 from the busy word of the epoch at hand, and a pick collides when
    the sweep reaches it within the horizon.  The per-channel rule, best_channel's, on crn_channel_stats records (tests/channels_f64.py)
    that keep learning every epoch: the largest p_idle of crnsense.channel_forecast, ties to the lowest channel."""
    T, C_ = 560, 8
    pos = hc.sweep(C_, T + 3)
    w = (np.uint64(1) << pos.astype(np.uint64)).astype(np.uint64)
    rec = _rec(ht.sequence(w[: T // 2], C_, (1, 2, 3)), 3)
    stats = ch.update(None, w[: T // 2], None, T // 2, True, C_)
    for h in (2, 3):
        st = stats.copy()
        hops_hit = chan_hit = 0
        for t in range(T // 2, T):
            st = ch.update(st, w[t: t + 1], None, 1, False)
            ahead = set(pos[t + 1: t + 1 + h].tolist())
            hops_hit += cs.next_channel(rec, int(w[t]), h) in ahead
            p_idle = [cs.channel_forecast(st[0, c], h)[2] for c in range(C_)]
            chan_hit += int(np.argmax(p_idle)) in ahead
        n = T - T // 2
        print(f"horizon {h}: next_channel collides in {hops_hit} of {n} epochs, the per-channel rule in {chan_hit} ({100 * chan_hit / n:.1f} %)")
        assert hops_hit == 0
        assert chan_hit >= 0.10 * n
    with pytest.raises(ValueError):
        cs.next_channel(rec, 1, 4)
    with pytest.raises(ValueError):
        cs.next_channel(_rec(ht.sequence(w[:50], C_, (1, 3)), 2), 1, 2)
