"""crn_resample_device on the MI355X: the kernel against the twin (tests/resample_f64.py) fed the kernel's own fp32 input, table, rows
and states, every output within gamma 2^-24 sum max(|h[phi][k]|, |h[phi + 1][k]|) |x[j - k]| of it (gamma = T + 12, include/crn_sense.h);
the zero tails, the dead rows and every byte of the states exact.  Then the carries, the cut rule, the 0xFF behind every array, every
refusal, the generator's RRC-QPSK carrier brought to four samples per symbol, and the cost next to the transform and the extraction
that feed the stage."""
import ctypes as C

import numpy as np
import pytest

import crnsense as cs
import extract_f64 as xf
import resample_f64 as rf

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import stage_gpu as sgpu        # noqa: E402  (needs torch)
from stage_gpu import DEV       # noqa: E402

R072, R144 = int(np.rint(0.72 * 2 ** 32)), int(np.rint(1.44 * 2 ** 32))
LIVE = (2 ** 30, 2 ** 34, 2 ** 32, 2 ** 32 + 1, R072, R144)
DEAD = (0, 2 ** 30 - 1, 2 ** 34 + 1, 2 ** 64 - 1)
DPHI = (0, 1, -1, 2 ** 31 - 1, -2 ** 31)


def _upload(a):
    """An array's bytes on the device."""
    return torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(DEV)


def _call(s, x, rws, h, state, out_cap, first=False):
    """One call on host arrays: (out [n_rows][out_cap] complex64 as the device wrote it, the states it left); the guard bytes behind
    the output and the states are checked."""
    n_rows, in_len = x.shape
    x_t, r_t, h_t = _upload(np.ascontiguousarray(x, np.complex64)), _upload(rws), _upload(h)
    pd = sgpu.Padded(out=n_rows * out_cap * 8, state=n_rows * 320)
    pd.state[: n_rows * 320] = _upload(state)
    q = cs.resample_params(in_len, out_cap, h.shape[1], h.shape[0] - 1, first)
    s.resample_device(x_t.data_ptr(), n_rows, q, r_t.data_ptr(), h_t.data_ptr(), pd.state.data_ptr(), pd.out.data_ptr())
    pd.host()
    assert pd.pads_untouched(), "memory behind the output or the states was written"
    return pd.view("out", np.complex64, (n_rows, out_cap)), pd.view("state", np.dtype(rf.STATE_DTYPE))


def _against_twin(y, new, x, rws, h, state, out_cap, first, what):
    """Every output within the bound; the zero tail of every row, the dead rows and the states byte for byte.  Returns the twin's
    states and the largest share of the bound used."""
    want, st, scale = rf.run(x, rws, h, state, out_cap, first, want_scale=True)
    b = rf.bound(scale, h.shape[1])
    assert np.isfinite(y.view(np.float32)).all(), what
    err = np.abs(y.astype(np.complex128) - want)
    assert (err <= b).all(), (what, float((err / np.where(b > 0, b, 1)).max()))
    for r in range(len(rws)):
        assert not y[r, int(st["last_n_out"][r]):].tobytes().strip(b"\0"), (what, r)
    assert new.tobytes() == st.tobytes(), (what, [name for name in new.dtype.names if new[name].tobytes() != st[name].tobytes()])
    return st, float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0


def _noise(rng, n_rows, n):
    return (rng.standard_normal((n_rows, n)) + 1j * rng.standard_normal((n_rows, n))).astype(np.complex64)


def _mixed_rows(n_rows, shift=0):
    """The ratios mixed across the rows of one call: the six live steps and the four dead ones in turn, every dphi with each."""
    steps = [(LIVE + DEAD)[(i + shift) % 10] for i in range(n_rows)]
    return rf.rows(steps, [DPHI[(i + i // 10) % 5] for i in range(n_rows)])


@pytest.mark.parametrize("T,P", [(8, 32), (16, 128), (32, 256), (16, 32)])
def test_kernel_against_twin(built, T, P):
    """Per (T, P): in_len 1, 2, T - 2, T - 1, T, 255, 256, 257 (n = in_len at rho = 1: the tile borders) and 1000 with 37 rows of mixed
    ratios, two calls each, the second from the state the first left (the history is in use); 1 and 3 rows; the input scaled by 1e12
    and by 1e-14; in_len 513 with out_cap = n - 1 and n + 1 of the rows at rho = 1; a table of zeros; the impulse's closed form."""
    s = cs.Sensor(sgpu.cfg(512))
    rng = np.random.default_rng(100 * T + P)
    h = cs.resample_taps(T, P, 0.3, 8.0)
    share = 0.0

    def two_calls(x, rws, out_cap, what):
        nonlocal share
        in_len = x.shape[1] // 2
        st = rf.states(len(rws), 0xFF)                        # taps = -1: taken as empty without `first`
        for call in range(2):
            part = x[:, call * in_len: (call + 1) * in_len]
            y, new = _call(s, part, rws, h, st, out_cap)
            st, sh = _against_twin(y, new, part, rws, h, st, out_cap, False, (T, P) + what + (call,))
            share = max(share, sh)
        return st
    for in_len in (1, 2, T - 2, T - 1, T, 255, 256, 257, 1000):
        rws = _mixed_rows(37, in_len)
        st = two_calls(_noise(rng, 37, 2 * in_len), rws, cs.resample_out_cap(in_len, 0.25), (in_len, 37))
        one = rws["step"] == 2 ** 32
        assert one.any() and (st["n_out"][one] == 2 * in_len).all() and (st["last_n_out"][one] == in_len).all()
    for n_rows, in_len, steps in ((1, 1000, [R072]), (1, 257, [2 ** 34 + 1]), (3, 1000, [R144, 0, 2 ** 30]), (3, 255, [2 ** 32 + 1, R072, 2 ** 34])):
        two_calls(_noise(rng, n_rows, 2 * in_len), rf.rows(steps, DPHI[1: 1 + n_rows]), cs.resample_out_cap(in_len, 0.25), (in_len, n_rows))
    x0 = _noise(rng, 37, 2 * 257)
    for scale in (1e12, 1e-14):
        two_calls((x0 * np.float32(scale)).astype(np.complex64), _mixed_rows(37), 4 * 257, (257, 37, scale))
    # n = 513 at rho = 1, out_cap one below and one above; the other ratios drop more or fill less
    for out_cap in (512, 514):
        st = two_calls(_noise(rng, 37, 2 * 513), _mixed_rows(37), out_cap, (513, 37, out_cap))
        assert (st["n_dropped"][_mixed_rows(37)["step"] == 2 ** 32] == 2 * max(513 - out_cap, 0)).all()
    # a table of zeros: every output 0
    x = _noise(rng, 3, 300)
    y, _ = _call(s, x, rf.rows([R072, R144, 2 ** 32], DPHI[:3]), np.zeros_like(h), rf.states(3), 420, first=True)
    assert (y == 0).all()
    # a one-sample impulse at rho = 1: the table's row 0; at half a sample's offset: the mean of rows P / 2 (mu = 0: the row itself)
    imp = np.zeros((2, 3 * T), np.complex64)
    imp[:, 5] = 2 - 1j
    st = rf.states(2)
    st["pos"][1], st["taps"] = 2 ** 31, T
    y, _ = _call(s, imp, rf.rows([2 ** 32, 2 ** 32]), h, st, 3 * T)
    for r, row in ((0, h[0]), (1, h[P // 2])):
        want = np.zeros(3 * T, np.complex64)
        want[5: 5 + T] = row * np.complex64(2 - 1j)
        assert (y[r, : 3 * T - r] == want[: 3 * T - r]).all(), (T, P, r)
    s.close()
    print(f"T={T} P={P}: largest |z - z_twin| is {100 * share:.1f} % of the bound (gamma = {rf.gamma(T)})")


def test_carries(built):
    """`first` over states of 0xFF; 0xFF without `first`; a state of another T; a valid state with pos >= L (n = 0, pos falls by L);
    negative counters; a dead row over a foreign state: all byte for byte as the twin has them."""
    T, P, in_len, out_cap = 16, 128, 300, 450
    s = cs.Sensor(sgpu.cfg(512))
    rng = np.random.default_rng(5)
    h = cs.resample_taps(T, P, 0.3, 8.0)
    x = _noise(rng, 8, in_len)
    rws = rf.rows([R072, R144, 2 ** 32 + 1, R072, 2 ** 34, R144, 2 ** 64 - 1, 2 ** 30], [7, -7, 2 ** 31 - 1, -2 ** 31, 1, 99, 5, 0])
    st = rf.states(8, 0xFF)
    prev = rf.run(_noise(rng, 1, 100), rws[:1], h, rf.states(1), 200, first=True)[1]
    st[0] = prev[0]                                                   # a state a call left
    st["taps"][2] = 8                                                   # another T, everything else 0xFF
    st[3] = prev[0]
    st["pos"][3] = (in_len << 32) + 12345                               # valid, pos >= L
    st["taps"][4] = T                                                   # valid, pos = 2^64 - 1, counters -1, a history of NaN bytes
    st[5] = prev[0]
    st["n_in"][5], st["n_out"][5], st["n_dropped"][5] = -5, -2 ** 63, -1
    st["taps"][6] = T                                                   # a dead row: only last_n_out is written
    for first in (False, True):
        y, new = _call(s, x, rws, h, st, out_cap, first)
        _against_twin(y, new, x, rws, h, st, out_cap, first, ("carry", first))
        assert not y[6].tobytes().strip(b"\0") and new["last_n_out"][6] == 0 and np.abs(y[[0, 1, 2, 5, 7], 20: 200]).min() > 0
        if not first:
            assert new["pos"][3] == 12345 and new["last_n_out"][3] == 0 and not y[3].tobytes().strip(b"\0")
            assert new["pos"][4] == 2 ** 64 - 1 - (in_len << 32) and (new["n_in"][4], new["n_out"][4], new["n_dropped"][4]) == (in_len, 0, 0)
            assert (new["n_in"][5], new["n_out"][5], new["n_dropped"][5]) == (in_len, new["last_n_out"][5], 0)
            assert new["n_in"][0] == 100 + in_len and new["n_in"][1] == in_len and new["n_in"][2] == in_len and new["taps"][2] == T
            keep = new[6: 7].copy()
            keep["last_n_out"] = st["last_n_out"][6]
            assert keep.tobytes() == st[6: 7].tobytes()
    s.close()


@pytest.mark.parametrize("T,P", [(16, 128), (32, 256)])
def test_cutting(built, T, P):
    """1000 samples as 1, 2, 61, 1, 64, 64, 807 against one call: outputs bit for bit and the final state byte for byte (last_n_out
    apart, which speaks of the last call alone), at rho 0.72 and 1.44 and just above 1; the same call twice from the same state."""
    s = cs.Sensor(sgpu.cfg(512))
    rng = np.random.default_rng(T)
    h = cs.resample_taps(T, P, 0.3, 8.0)
    x = _noise(rng, 3, 1000)
    rws = rf.rows([R072, R144, 2 ** 32 + 1], [123456789, -2 ** 31, 2 ** 31 - 1])
    cap = cs.resample_out_cap(1000, 0.72)
    st0 = rf.states(3, 0xFF)
    whole, st_whole = _call(s, x, rws, h, st0, cap, first=True)
    again, st_again = _call(s, x, rws, h, st0, cap, first=True)
    assert whole.tobytes() == again.tobytes() and st_whole.tobytes() == st_again.tobytes()
    _against_twin(whole, st_whole, x, rws, h, st0, cap, True, ("cut", T, P))
    st, at, got = st0, 0, [[], [], []]
    for i, c in enumerate((1, 2, 61, 1, 64, 64, 807)):
        if i == 4:                                             # the same call twice from the same state, a carried one
            y2, st2 = _call(s, x[:, at: at + c], rws, h, st, cap)
        y, st = _call(s, x[:, at: at + c], rws, h, st, cap, first=(i == 0))
        if i == 4:
            assert y2.tobytes() == y.tobytes() and st2.tobytes() == st.tobytes()
        for r in range(3):
            got[r].append(y[r, : int(st["last_n_out"][r])])
        at += c
    for r in range(3):
        w = int(st_whole["last_n_out"][r])
        assert w > 600 and np.concatenate(got[r]).tobytes() == whole[r, :w].tobytes(), (T, P, r)
    assert st["last_n_out"].tolist() != st_whole["last_n_out"].tolist()
    st = st.copy()
    st["last_n_out"] = st_whole["last_n_out"]
    assert st.tobytes() == st_whole.tobytes()
    s.close()


def test_refusals_with_a_live_handle(built):
    """Every refusal of the header's list; a refused call and n_rows = 0 leave the output and the states as they were."""
    T, P, n_rows, in_len, out_cap = 16, 128, 4, 64, 100
    L = cs.lib()
    s = cs.Sensor(sgpu.cfg(512))
    rng = np.random.default_rng(1)
    x_t = _upload(_noise(rng, n_rows, in_len + 2))
    r_t = _upload(np.concatenate([rf.rows([R072, R144, 2 ** 32, 2 ** 30]), rf.rows([2 ** 32])]))
    h = cs.resample_taps(T, P, 0.3, 8.0)
    h_t = _upload(np.concatenate([h, h]))
    pd = sgpu.Padded(out=n_rows * out_cap * 8, state=n_rows * 320)

    def rc(xp=x_t.data_ptr(), nr=n_rows, q=None, rp=r_t.data_ptr(), tp=h_t.data_ptr(), sp=pd.state.data_ptr(), op=pd.out.data_ptr(), hd=s._h,
           in_len=in_len, out_cap=out_cap, taps=T, phases=P, first=1, reserved=(0, 0, 0)):
        if q is None:
            q = cs.resample_params(in_len, out_cap, taps, phases, first)
            for i, v_ in enumerate(reserved):
                q.reserved[i] = v_
        v = lambda p: C.c_void_p(p or None)      # noqa: E731
        return L.crn_resample_device(hd, v(xp), nr, C.byref(q) if q != 0 else None, v(rp), v(tp), v(sp), v(op), None)
    assert rc() == 0
    before = {k: v.copy() for k, v in pd.host().items()}
    assert pd.pads_untouched() and np.abs(pd.view("out", np.complex64, (n_rows, out_cap))[:, 1: 16]).min() > 0      # (h[0][0] = 0: output 0 is 0)
    pd.out[: n_rows * out_cap * 8] = 255
    pd.state[: n_rows * 320] = 255
    for bad in ({"hd": None}, {"xp": 0}, {"q": 0}, {"rp": 0}, {"tp": 0}, {"sp": 0}, {"op": 0},
                {"taps": 0}, {"taps": 4}, {"taps": 12}, {"taps": 64}, {"taps": -16}, {"phases": 0}, {"phases": 16}, {"phases": 96}, {"phases": 512},
                {"phases": -128}, {"in_len": 0}, {"in_len": -1}, {"in_len": 2 ** 24 + 1}, {"out_cap": 0}, {"out_cap": -5}, {"out_cap": 2 ** 26 + 1},
                {"nr": -1}, {"nr": 65537}, {"reserved": (1, 0, 0)}, {"reserved": (0, -1, 0)}, {"reserved": (0, 0, 7)},
                {"xp": x_t.data_ptr() + 8}, {"rp": r_t.data_ptr() + 8}, {"tp": h_t.data_ptr() + 4}, {"tp": h_t.data_ptr() + 8},
                {"sp": pd.state.data_ptr() + 8}, {"op": pd.out.data_ptr() + 8}):
        assert rc(**bad) == cs.CRN_ERR_ARG, bad
        assert b"crn_resample_device" in L.crn_last_error(), bad
    assert rc(nr=0) == 0 and rc(nr=0, first=0) == 0
    raw = pd.host()
    assert (raw["out"] == 255).all() and (raw["state"] == 255).all() and pd.pads_untouched()
    # the ends of the ranges and aligned offsets are accepted
    assert rc(in_len=1) == 0 and rc(out_cap=1) == 0 and rc(taps=8, phases=32) == 0 and rc(taps=32, phases=256) == 0 and rc(phases=64) == 0
    assert rc(xp=x_t.data_ptr() + 16, rp=r_t.data_ptr() + 16, tp=h_t.data_ptr() + 16 * T) == 0 and rc(nr=1) == 0
    assert rc() == 0
    raw = pd.host()
    assert raw["out"].tobytes() == before["out"].tobytes() and raw["state"].tobytes() == before["state"].tobytes() and pd.pads_untouched()
    s.close()


# The generator's carrier end to end, as in tests/test_extract_gpu.py: RRC-QPSK at the default levels on the 60-bin channel.
E2E = {"n": 1024, "frames": 8, "epochs": 32, "seed": 2051, "noise_power": 1e-6, "signal_rms": 0.02, "channel": 2, "out_len": 128, "flat": 40,
       "symbol_bins": 44.4444, "sps": 4}


def _line(z):
    """The strength of the line of |z|^2 at exactly 1 / 4 cycle per sample, relative to the sum of |z|^2; z [rows][samples]."""
    p = np.abs(z.astype(np.complex128)) ** 2
    return float(np.abs((p * np.exp(-0.5j * np.pi * np.arange(z.shape[1]))[None, :]).sum())) / float(p.sum())


def test_end_to_end_the_generators_carrier_at_four_samples_per_symbol(built):
    """The extraction's own end-to-end setup (crn_synth_fill_device_ex RRC-QPSK, crn_fft_forward_device at stride N / 2, crn_extract_device
    at M = 128 on the centre of the 60-bin channel), then this stage on the extracted rows as they lie on the device, with
    resample_ratio(128, 44.4444, 4) and the (16, 128, beta 8, cutoff 0.40) table.  The device is within the bound of the twin fed the same
    extracted samples; at four samples per symbol |z|^2 carries a line at exactly 1 / 4 cycle per sample, and its strength relative to
    sum |z|^2 over the epochs that drive the channel equals the twin's to 1e-3 relative."""
    n, K, E, m, flat = E2E["n"], E2E["frames"], E2E["epochs"], E2E["out_len"], E2E["flat"]
    cfg = sgpu.cfg(n, k=K)
    bins = [b for g in cfg.segs[: cfg.n_segs] if g.band == E2E["channel"] for b in range(g.lo, g.hi)]
    centre = (bins[0] + bins[-1] + 1) // 2
    F = 2 * K
    iq_t = sgpu.zeros(((E * K * n + n // 2) * 2,), torch.float32)
    truth_t = torch.full((E,), -1, dtype=torch.int32, device=DEV)
    sc = cs.SynthCfg()
    sc.seed, sc.noise_power, sc.signal_rms = E2E["seed"], E2E["noise_power"], E2E["signal_rms"]
    sc.tones_per_band, sc.pu_model, sc.signal_kind, sc.n_streams = 0, cs.PU_UNIFORM, cs.SIG_RRC_QPSK, 1
    s = cs.Sensor(cfg)
    s.synth_fill_device_ex(iq_t.data_ptr(), E, K * n, sc, truth_ptr=truth_t.data_ptr())
    x_t = sgpu.zeros((E * F * n * 2,), torch.float32)
    s.fft_forward_device(iq_t.data_ptr(), E * F, n, x_t.data_ptr(), frame_stride=n // 2)
    ch = xf.channel_records([(e, centre) for e in range(E)])
    ch_t, h_t = _upload(ch), torch.from_numpy(cs.extract_taper(m, flat)).to(DEV)
    in_len = F * (m // 2)
    e_t = sgpu.zeros((E * in_len * 2,), torch.float32)
    s.extract_device(x_t.data_ptr(), E * F, cs.extract_params(m, F), ch_t.data_ptr(), E, h_t.data_ptr(), e_t.data_ptr())
    rho = cs.resample_ratio(m, E2E["symbol_bins"], E2E["sps"])
    rws = cs.resample_rows([rho] * E)
    taps = cs.resample_taps(16, 128, 0.40, 8.0)
    cap = cs.resample_out_cap(in_len, rho)
    r_t, t_t = _upload(rws), _upload(taps)
    pd = sgpu.Padded(out=E * cap * 8, state=cs.resample_state_bytes(E))
    s.resample_device(e_t.data_ptr(), E, cs.resample_params(in_len, cap, 16, 128, first=True), r_t.data_ptr(), t_t.data_ptr(), pd.state.data_ptr(),
                      pd.out.data_ptr())
    pd.host()
    assert pd.pads_untouched()
    z = pd.view("out", np.complex64, (E, cap))
    new = pd.view("state", np.dtype(rf.STATE_DTYPE))
    ext = e_t.cpu().numpy().view(np.complex64).reshape(E, in_len)
    truth = truth_t.cpu().numpy()
    s.close()
    twin_states, share = _against_twin(z, new, ext, rws, taps, rf.states(E, 0xFF), cap, True, "end to end")
    want = rf.run(ext, rws, taps, rf.states(E), cap, True)[0]
    driven = np.flatnonzero(truth == E2E["channel"])
    w = int(new["last_n_out"][0])
    assert len(driven) >= 4 and (new["last_n_out"] == w).all() and w == cap
    keep = slice(64, w - w // F)                  # the filter's start and the frame that reaches into the next epoch left out
    got_line, twin_line = _line(z[driven][:, keep]), _line(want[driven][:, keep])
    idle = np.flatnonzero(truth == 0)
    print(f"channel {E2E['channel']} centre {centre}; rho {rho:.6f}, {w} outputs a row; {len(driven)} driven epochs of {E}; line of |z|^2 at 1/4 cycle per "
          f"sample relative to sum |z|^2: {got_line:.6f} on the device, {twin_line:.6f} in the twin"
          + (f" ({_line(z[idle][:, keep]):.6f} over the idle epochs)" if len(idle) else "") + f"; largest share of the bound {100 * share:.1f} %")
    assert twin_line > 0 and abs(got_line - twin_line) <= 1e-3 * twin_line, (got_line, twin_line)


# crn_fft_forward_device + crn_extract_device + this stage against the first two alone, with the margin of the other stages:
# 1 + 1.5 x (the largest measured B / A - 1).  Measured on an MI355X in two separate runs (profiles/r23_resample.txt): arm A
# 376.9 and 377.1 us; at rho 0.72 with (16, 128) B / A = 2.1897 and 2.2198, the stage alone 449.3 and 451.9 us; at rho 1.44 with (32, 256)
# 2.6774 and 2.6832, alone 640.6 and 641.8 us.
SPEED_RATIO = {(0.72, 16, 128): 2.830, (1.44, 32, 256): 3.525}


def test_cost_next_to_the_transform_and_the_extraction_that_feed_it(built):
    """N = 1024, 64 streams of 1024 half-overlapped frames, M = 64, 16 channels per stream: the batch of the extraction's cost test and the
    method of tests/stage_gpu.py (best_of_windows).  Arm A is the transform and the extraction; arm B the same followed by this stage on
    all 1024 extracted rows of 32 768 samples, at rho 0.72 with the (16, 128) table and at rho 1.44 with the (32, 256) one.  The stage
    alone is measured the same way; all figures are printed."""
    n, S, F, m = 1024, 64, 1024, 64
    iq_t = sgpu.noise_batch(S * F + 1, 1, n // 2)
    s = cs.Sensor(sgpu.cfg(n))
    x_t = sgpu.zeros((S * F * n * 2,), torch.float32)
    ht_t = torch.from_numpy(cs.extract_taper(m, 16)).to(DEV)
    ch = xf.channel_records([(st, 32 + 64 * i) for st in range(S) for i in range(16)])
    ch_t = _upload(ch)
    n_rows, in_len = len(ch), F * (m // 2)
    e_t = sgpu.zeros((n_rows * in_len * 2,), torch.float32)
    qe = cs.extract_params(m, F)
    loads = {}
    for rho, T, P in SPEED_RATIO:
        cap = cs.resample_out_cap(in_len, rho)
        taps = cs.resample_taps(T, P, 0.40 / max(rho, 1.0), 8.0)
        rws = cs.resample_rows([rho] * n_rows, 0.01)
        loads[(rho, T, P)] = (cap, taps, rws, _upload(taps), _upload(rws), sgpu.Padded(out=n_rows * cap * 8, state=n_rows * 320),
                              cs.resample_params(in_len, cap, T, P, first=True))

    def arm_a():
        s.fft_forward_device(iq_t.data_ptr(), S * F, n, x_t.data_ptr(), frame_stride=n // 2)
        s.extract_device(x_t.data_ptr(), S * F, qe, ch_t.data_ptr(), n_rows, ht_t.data_ptr(), e_t.data_ptr())

    def stage(key):
        cap, _, _, t_t, r_t, pd, q = loads[key]
        s.resample_device(e_t.data_ptr(), n_rows, q, r_t.data_ptr(), t_t.data_ptr(), pd.state.data_ptr(), pd.out.data_ptr())
    arms = {"A": arm_a}
    for key in SPEED_RATIO:
        arms[f"B, {key}"] = lambda key=key: (arm_a(), stage(key))
        arms[f"alone, {key}"] = lambda key=key: stage(key)
    times = sgpu.best_of_windows(arms)
    best = {name: min(v) for name, v in times.items()}
    # the stage computed what the definition says: the first 2048 samples of row 5 once more on their own give the same bytes (the cut
    # rule), and are within the bound of the twin
    part = e_t.view(n_rows, in_len, 2)[5, :2048].cpu().numpy().view(np.complex64).reshape(1, 2048)
    for key, (cap, taps, rws, _, _, pd, _) in loads.items():
        big = pd.out[5 * cap * 8: (5 * cap + 4096) * 8].cpu().numpy().view(np.complex64)
        y, new = _call(s, part, rws[5: 6], taps, rf.states(1), 4096, first=True)
        w = int(new["last_n_out"][0])
        assert 1000 < w < 4096 and y[0, :w].tobytes() == big[:w].tobytes(), key
        _against_twin(y, new, part, rws[5: 6], taps, rf.states(1), 4096, True, ("cost", key))
        assert bool((pd.out[n_rows * cap * 8:] == 255).all()) and bool((pd.state[n_rows * 320:] == 255).all()), "memory behind an array was written"
        st = pd.state[: n_rows * 320].cpu().numpy().view(np.dtype(rf.STATE_DTYPE))
        assert (st["last_n_out"] == cap).all() and (st["n_in"] == in_len).all() and not st["n_dropped"].any()
    s.close()
    for key in SPEED_RATIO:
        cap = loads[key][0]
        moved = n_rows * (in_len + cap) * 8
        alone = best[f"alone, {key}"]
        print(f"N=1024, {S} streams of {F} half-overlapped frames, M={m}, 16 channels per stream, {n_rows} rows of {in_len} samples, (rho, T, P) = {key}: arm A "
              f"(transform + extraction) {best['A']:.4f} ms; B / A = {best[f'B, {key}'] / best['A']:.4f}; crn_resample_device alone {alone * 1e3:.1f} us; "
              f"{moved / 1e6:.0f} MB to move: {moved / alone / 1e9:.2f} TB/s")
    for key in SPEED_RATIO:
        ratio = best[f"B, {key}"] / best["A"]
        assert ratio <= SPEED_RATIO[key], (key, ratio, SPEED_RATIO[key])
