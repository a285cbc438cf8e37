"""crn_resample_device without a GPU: the twin (tests/resample_f64.py) against signals whose resampling is known — multitones that must
come out as the same tones at the output's times, a tone that would alias, the extraction's off-grid tone brought to rest — the cut
rule, the count at the ends of the ratio's range, dropped outputs, the helpers of crnsense.py and the binding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import crnsense as cs
import extract_f64 as xf
import resample_f64 as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMP_SUM = 3.25     # 1 + .5 + .25 + .5 + 1


def _resample(x, T, P, beta, fc, rho, dphi=0):
    """One row through the twin from an empty state, out_cap = n: (the outputs, the table, the step)."""
    h = rf.table(T, P, fc, beta)
    step = int(np.rint(rho * 2 ** 32))
    cap = rf.count(0, step, x.size)
    y, st = rf.run(x[None, :], rf.rows([step], [dphi]), h, rf.states(1), cap, first=True)
    assert int(st["last_n_out"][0]) == cap == int(st["n_out"][0]) and int(st["n_dropped"][0]) == 0 and int(st["n_in"][0]) == x.size
    return y[0], h, step


# (T, P, beta, fc, rho, b, bar): the bars are the issue's, each its prototype's figure (1.04e-4, 1.26e-4, 1.10e-4, 8.5e-6, 5.4e-6, 2.9e-3)
# with about 40 % of room; the twin gives 1.036e-4, 1.262e-4, 1.103e-4, 8.45e-6, 5.37e-6 and 2.893e-3
MULTITONES = [(16, 128, 8, 0.40, 0.72, 0.22, 1.5e-4),
              (16, 32, 8, 0.40, 0.72, 0.22, 1.8e-4),          # what the linear interpolation between phase rows is for
              (16, 128, 8, 0.40 / 1.44, 1.44, 0.10, 1.6e-4),
              (32, 256, 10, 0.42 / 1.44, 1.44, 0.18, 1.2e-5),
              (32, 256, 10, 0.40, 0.72, 0.29, 8e-6),
              (8, 32, 5, 0.40, 1.0, 0.15, 4e-3)]


@pytest.mark.parametrize("T,P,beta,fc,rho,b,bar", MULTITONES)
def test_multitone_comes_out_as_the_same_tones_at_the_outputs_times(T, P, beta, fc, rho, b, bar):
    """Five tones inside the passband, 4096 samples rounded to complex64: output u is the same tones at time u rho - T / 2."""
    x = rf.tones(b, np.arange(4096)).astype(np.complex64)
    y, _, step = _resample(x, T, P, beta, fc, rho)
    want = rf.tones(b, np.arange(y.size) * (step / 2.0 ** 32) - T / 2)
    err = float(np.abs(y[64:] - want[64:]).max()) / AMP_SUM
    print(f"T={T} P={P} beta={beta} fc={fc:.4f} rho={rho} b={b}: largest error / amplitude sum {err:.3e}; bar {bar:g}")
    assert y.size > 2000 and err <= bar, (err, bar)


# (T, P, beta, fc, rho, tone, bar in dB): the twin gives -82.27 and -96.65 dB
ALIASES = [(16, 128, 8, 0.40 / 1.44, 1.44, 0.46, -80.0), (32, 256, 10, 0.42 / 1.44, 1.44, 0.40, -94.0)]


@pytest.mark.parametrize("T,P,beta,fc,rho,f0,bar", ALIASES)
def test_a_tone_that_would_alias_is_gone(T, P, beta, fc, rho, f0, bar):
    x = np.exp(2j * np.pi * f0 * np.arange(4096)).astype(np.complex64)
    y, _, _ = _resample(x, T, P, beta, fc, rho)
    db = 20 * np.log10(float(np.abs(y[64:]).max()))
    print(f"T={T} P={P} rho={rho}: a unit tone at {f0} comes out at {db:.2f} dB; bar {bar:g} dB")
    assert db <= bar, (db, bar)


def test_the_limit_the_documents_state():
    """Tones at b = 0.30 under the first table are 2 % off: 0.10 inside the cutoff is not enough for 16 taps."""
    x = rf.tones(0.30, np.arange(4096)).astype(np.complex64)
    y, _, step = _resample(x, 16, 128, 8, 0.40, 0.72)
    err = float(np.abs(y[64:] - rf.tones(0.30, np.arange(y.size) * (step / 2.0 ** 32) - 8)[64:]).max()) / AMP_SUM
    print(f"b = 0.30: {err:.3e}")
    assert 1.5e-2 <= err <= 2.5e-2
    for name in ("include/crn_sense.h", "DESIGN.md"):
        txt = re.sub(r"\s+", " ", open(os.path.join(ROOT, name)).read().replace(" * ", " "))
        assert "16 taps have a transition band of about +-0.16 cycles per sample" in txt and "8 taps +-0.18, 32 taps +-0.10" in txt, name
        assert "tones at 0.30 are 2 % off" in txt, name


def test_chain_the_extractions_off_grid_tone_comes_to_rest():
    """extract_f64 on a tone of amplitude 0.5 at bin 300.37 (N 1024, M 64, flat 16, centre 300, 40 frames) leaves 0.37 bins of offset,
    0.37 / 64 cycles per extracted sample; the mixer takes them away per OUTPUT sample, dphi = rint(-(0.37 / 64) step).  Outputs 64
    onwards are one constant.  The twin gives 2.34e-4 (mean modulus 0.500001); the issue's figure is 2.3e-4 and its bar 3.3e-4."""
    n, m, F = 1024, 64, 40
    x = 0.5 * np.exp(2j * np.pi * 300.37 * np.arange((F + 1) * n // 2) / n)
    e = xf.run(xf.spectra(x, n), xf.channel_records([(0, 300)]), xf.taper(m, 16), m, F)[0].astype(np.complex64)
    step = int(np.rint(0.72 * 2 ** 32))
    y, _, _ = _resample(e, 16, 128, 8, 0.40, 0.72, dphi=int(np.rint(-(0.37 / 64) * step)))
    z = y[64:]
    dev = float(np.abs(z - z.mean()).max()) / 0.5
    print(f"chain: largest deviation from the mean {dev:.3e} of 0.5; mean modulus {abs(z.mean()):.6f}; bar 3.3e-4")
    assert z.size > 1500 and dev <= 3.3e-4 and abs(abs(z.mean()) - 0.5) <= 1e-5
    # the helper's way to the same record: the offset in cycles per output sample
    rec = cs.resample_rows(0.72, -(0.37 / 64) * 0.72)
    assert int(rec["step"][0]) == step and abs(int(rec["dphi"][0]) - int(np.rint(-(0.37 / 64) * step))) <= 1


def _noise(rng, n_rows, n):
    return (rng.standard_normal((n_rows, n)) + 1j * rng.standard_normal((n_rows, n))).astype(np.complex64)


def _fed_in_cuts(x, rws, h, cuts, out_cap):
    """The rows fed in calls of the given lengths from an empty state: (outputs concatenated over last_n_out, per row; the final states)."""
    st = rf.states(len(rws), 0xFF)
    got = [[] for _ in rws]
    at = 0
    for i, c in enumerate(cuts):
        y, st = rf.run(x[:, at: at + c], rws, h, st, out_cap, first=(i == 0))
        for r in range(len(rws)):
            got[r].append(y[r, : int(st["last_n_out"][r])])
        at += c
    assert at == x.shape[1]
    return [np.concatenate(g) for g in got], st


@pytest.mark.parametrize("T,P", [(16, 128), (8, 32), (32, 256)])
def test_cut_1_2_997_3096_equals_the_uncut_row(T, P):
    rng = np.random.default_rng(T)
    x = _noise(rng, 3, 4096)
    h = rf.table(T, P, 0.3, 8)
    rws = rf.rows([int(np.rint(0.72 * 2 ** 32)), int(np.rint(1.44 * 2 ** 32)), 2 ** 32 + 1], [12345, -2 ** 31, 2 ** 31 - 1])
    cap = rf.count(0, int(rws["step"].min()), 4096)
    whole, st1 = _fed_in_cuts(x, rws, h, [4096], cap)
    parts, st2 = _fed_in_cuts(x, rws, h, [1, 2, 997, 3096], cap)
    for a, b in zip(whole, parts):
        assert a.size > 2800 and a.tobytes() == b.tobytes()
    assert st1["last_n_out"].tolist() != st2["last_n_out"].tolist()
    st2["last_n_out"] = st1["last_n_out"]                   # the one field that speaks of the last call alone
    assert st1.tobytes() == st2.tobytes()
    assert st1["n_in"].tolist() == [4096] * 3 and st1["n_out"].tolist() == [a.size for a in whole] and not st1["n_dropped"].any()
    assert (st1["hist"][:, : T - 1] == x[:, 4096 - (T - 1):]).all() and not st1["hist"][:, T - 1:].any() and (st1["taps"] == T).all()


@pytest.mark.parametrize("T", rf.TAPS)
def test_the_ends_of_the_ratios_range_at_the_shortest_rows(T):
    """Ratios 2^30 and 2^34 at in_len 1, 2, T - 2, T - 1, T: the n of step 1 against a loop, fed call after call, and the history."""
    rng = np.random.default_rng(7)
    h = rf.table(T, 32, 0.1, 5)
    for step in (2 ** 30, 2 ** 34):
        for in_len in (1, 2, T - 2, T - 1, T):
            x = _noise(rng, 1, 5 * in_len)
            st = rf.states(1)
            pos = 0
            for call in range(5):
                L = in_len << 32
                n = 0
                while pos + n * step < L:
                    n += 1
                y, st = rf.run(x[:, call * in_len: (call + 1) * in_len], rf.rows([step]), h, st, 160, first=(call == 0))
                assert int(st["last_n_out"][0]) == n == rf.count(pos, step, in_len), (step, in_len, call)
                assert not y[0, n:].any()
                pos = pos + n * step - L if n else pos - L
                assert int(st["pos"][0]) == pos
                seen = np.concatenate([np.zeros(T - 1, np.complex64), x[0, : (call + 1) * in_len]])
                assert (st["hist"][0, : T - 1] == seen[seen.size - (T - 1):]).all() and not st["hist"][0, T - 1:].any()
            assert int(st["n_in"][0]) == 5 * in_len
            assert int(st["n_out"][0]) == rf.count(0, step, 5 * in_len)      # cut or not: the same count


def test_out_cap_below_n_drops_outputs_and_keeps_the_timing():
    rng = np.random.default_rng(8)
    x = _noise(rng, 1, 600)
    h = rf.table(16, 64, 0.3, 8)
    step, dphi = int(np.rint(0.72 * 2 ** 32)), 1234567
    n = rf.count(0, step, 300)
    full, s_full = rf.run(x[:, :300], rf.rows([step], [dphi]), h, rf.states(1), n, first=True)
    short, s_short = rf.run(x[:, :300], rf.rows([step], [dphi]), h, rf.states(1), n - 7, first=True)
    assert short[0].tobytes() == full[0, : n - 7].tobytes()
    assert (int(s_short["last_n_out"][0]), int(s_short["n_out"][0]), int(s_short["n_dropped"][0])) == (n - 7, n - 7, 7)
    assert int(s_short["pos"][0]) == int(s_full["pos"][0]) == n * step - (300 << 32)
    assert int(s_short["phase"][0]) == int(s_full["phase"][0]) == n * dphi % 2 ** 32
    # ... so the next call goes on as if nothing were lost
    a, sa = rf.run(x[:, 300:], rf.rows([step], [dphi]), h, s_full, n + 1)
    b, sb = rf.run(x[:, 300:], rf.rows([step], [dphi]), h, s_short, n + 1)
    assert a.tobytes() == b.tobytes() and int(sb["n_dropped"][0]) == 7 and int(sa["n_out"][0]) == int(sb["n_out"][0]) + 7


def test_twin_edges():
    rng = np.random.default_rng(9)
    x = _noise(rng, 6, 50)
    h = rf.table(8, 32, 0.3, 5)
    st = rf.states(6, 0xFF)
    st["taps"][4:] = 8                                       # valid states: pos = 2^64 - 1 >= L, negative counters
    y, new = rf.run(x, rf.rows([0, 2 ** 30 - 1, 2 ** 34 + 1, 2 ** 64 - 1, 2 ** 32, 2 ** 32], 5), h, st, 60)
    assert not y[:4].any() and not new["last_n_out"][:4].any()
    keep = new.copy()
    keep["last_n_out"][:4] = -1
    assert keep[:4].tobytes() == st[:4].tobytes()            # dead rows: the rest of the state untouched
    assert not y[4:].any() and new["pos"][4] == 2 ** 64 - 1 - (50 << 32) and new["phase"][4] == 2 ** 32 - 1
    assert (new["n_in"][4], new["n_out"][4], new["n_dropped"][4], new["last_n_out"][4]) == (50, 0, 0, 0)
    # another T: the state is taken as empty
    y8, s8 = rf.run(x[:1], rf.rows([2 ** 32]), h, rf.states(1), 50, first=True)
    h16 = rf.table(16, 32, 0.3, 5)
    a, sa = rf.run(x[:1], rf.rows([2 ** 32]), h16, s8, 50)
    b, sb = rf.run(x[:1], rf.rows([2 ** 32]), h16, rf.states(1), 50, first=True)
    assert a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes() and int(sa["taps"][0]) == 16 and y8.any()
    # an impulse at sample 3, rho = 1: output u is h[0][u - 3]
    imp = np.zeros((1, 20), np.complex64)
    imp[0, 3] = 2.0
    y, _ = rf.run(imp, rf.rows([2 ** 32]), h, rf.states(1), 20, first=True)
    assert (y[0, 3:11] == 2.0 * h[0].astype(np.float64)).all() and not y[0, :3].any() and not y[0, 11:].any()
    assert rf.gamma(8) == 20 and rf.gamma(32) == 44


def test_helpers():
    for T in cs.RESAMPLE_TAPS:
        for P in cs.RESAMPLE_PHASES:
            h = cs.resample_taps(T, P, 0.3, 8)
            assert h.dtype == np.float32 and h.shape == (P + 1, T) and h.tobytes() == rf.table(T, P, 0.3, 8).tobytes()
            assert abs(float(h[:P].astype(np.float64).sum()) - P) <= 1e-4 * P and h[0, 0] == 0            # g(-T / 2) = 0
            assert (h[P, :-1] == h[0, 1:]).all()                                                          # row P is row 0 one tap on
            assert int(np.argmax(h[0])) == T // 2 == cs.resample_delay(T)
    for bad in ((12, 128, .3, 8), (16, 100, .3, 8), (16, 128, 0, 8), (16, 128, .6, 8), (16, 128, .3, -1)):
        with pytest.raises(ValueError):
            cs.resample_taps(*bad)
    r = cs.resample_rows([0.72, 1.44, 1.0, 0.1], [0.25, -0.5, 0.5, 0.75])
    assert r.dtype == np.dtype(cs.RESAMPLE_ROW_DTYPE) == np.dtype(rf.ROW_DTYPE) and r.dtype.itemsize == 16
    assert r["step"].tolist() == [int(np.rint(0.72 * 2 ** 32)), int(np.rint(1.44 * 2 ** 32)), 2 ** 32, int(np.rint(0.1 * 2 ** 32))]
    assert r["dphi"].tolist() == [2 ** 30, -2 ** 31, -2 ** 31, -2 ** 30] and not r["reserved"].any()
    assert cs.resample_rows(0.5)["step"].tolist() == [2 ** 31] and cs.resample_rows(0.5)["dphi"].tolist() == [0]
    assert cs.resample_rows([1, 2], 0.125)["dphi"].tolist() == [2 ** 29] * 2
    for bad in ((float("nan"), 0.0), (float("inf"), 0.0), (1.0, float("nan")), ([1.0, 2.0], [0.0, float("-inf")])):
        with pytest.raises(ValueError, match="resample_rows"):
            cs.resample_rows(*bad)
    for in_len, rho in ((1, 0.25), (1000, 0.72), (4096, 1.44), (5, 4.0)):
        assert cs.resample_out_cap(in_len, rho) == rf.count(0, int(np.rint(rho * 2 ** 32)), in_len)
    assert cs.resample_out_cap(1, 0.25) == 4 and cs.resample_out_cap(5, 4.0) == 2
    for bad in ((0, 1.0), (10, 0.2), (10, 4.5)):
        with pytest.raises(ValueError):
            cs.resample_out_cap(*bad)
    assert cs.resample_ratio(128, 44.4444, 4) == 128 / 44.4444 / 4 and abs(cs.resample_ratio(128, 44.4444, 4) - 0.72) < 1e-4
    for bad in (0, 0.0, -1.0):
        with pytest.raises(ValueError):
            cs.resample_ratio(128, bad, 4)
    q = cs.resample_params(1000, 1400, 32, 256, first=True)
    assert (q.in_len, q.out_cap, q.taps, q.phases, q.first, list(q.reserved)) == (1000, 1400, 32, 256, 1, [0] * 3)
    assert cs.resample_params(5, 6).first == 0 and (cs.resample_params(5, 6).taps, cs.resample_params(5, 6).phases) == (16, 128)


def test_symbols_structures_and_binding(built):
    L = cs.lib()
    for name in ("crn_resample_device", "crn_resample_state_bytes"):
        assert name in cs.EXPORTS and hasattr(L, name)
    assert callable(cs.Sensor.resample_device)
    assert C.sizeof(cs.ResampleParams) == 32 and C.sizeof(cs.ResampleRow) == 16
    assert np.dtype(cs.RESAMPLE_ROW_DTYPE).itemsize == 16 and np.dtype(cs.RESAMPLE_STATE_DTYPE).itemsize == 320
    assert np.dtype(cs.RESAMPLE_STATE_DTYPE) == np.dtype(rf.STATE_DTYPE)
    sd = np.dtype(cs.RESAMPLE_STATE_DTYPE)
    assert [sd.fields[f][1] for f in sd.names] == [0, 8, 12, 16, 24, 32, 40, 44, 64]
    assert (cs.ResampleRow.step.offset, cs.ResampleRow.dphi.offset, cs.ResampleRow.reserved.offset) == (0, 8, 12)
    assert cs.resample_state_bytes(0) == 0 and cs.resample_state_bytes(3) == 960 and cs.resample_state_bytes(65536) == 320 * 65536
    assert L.crn_resample_state_bytes(-1) == -1 and L.crn_resample_state_bytes(65537) == -1
    with pytest.raises(ValueError):
        cs.resample_state_bytes(65537)
    hdr = open(os.path.join(ROOT, "include", "crn_sense.h")).read()

    def fields(struct):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        return [re.sub(r"\[\d+\]", "", f.strip()) for decl in body.split(";") if decl.strip()
                for f in re.sub(r"^\s*(u?int32_t|u?int64_t|float)\s", "", decl.strip()).split(",")]
    assert fields("crn_resample_params") == [f[0] for f in cs.ResampleParams._fields_]
    assert fields("crn_resample_row") == [f[0] for f in cs.ResampleRow._fields_] == [f[0] for f in cs.RESAMPLE_ROW_DTYPE]
    assert fields("crn_resample_state") == [f[0] for f in cs.RESAMPLE_STATE_DTYPE]
    for struct, size in (("crn_resample_params", 32), ("crn_resample_row", 16), ("crn_resample_state", 320)):
        assert f"/* {size} bytes */" in hdr[hdr.index("} %s;" % struct):][:48], struct
    assert hdr.index("crn_extract_device(") < hdr.index("crn_resample_state_bytes(") < hdr.index("crn_resample_device(") < hdr.index("crn_sense_reserve_host(")
    assert "gamma = T + 12" in hdr
    engine = os.path.join(ROOT, "cognitive-radio-network_amd", "cognitive_engines", "CE_Predictive_Node_GPU", "crn_sense.h")
    assert open(engine).read() == hdr
    assert L.crn_abi_version() == cs.CRN_ABI_VERSION == 4     # additive: the ABI version stays


def test_no_handle_is_refused_before_anything_is_looked_at(built):
    """Every refusal that needs no device: with no handle the call is refused whatever else it holds, and nothing is touched."""
    L = cs.lib()
    q = cs.resample_params(64, 100)
    buf = (C.c_uint8 * 65536)()
    p = (C.addressof(buf) + 63) & ~63
    assert L.crn_resample_device(None, p, 2, C.byref(q), p, p, p, p, None) == cs.CRN_ERR_ARG
    assert b"crn_resample_device" in L.crn_last_error()
    assert L.crn_resample_device(None, None, -1, None, None, None, None, None, None) == cs.CRN_ERR_ARG
    assert not bytes(buf).strip(b"\0")
