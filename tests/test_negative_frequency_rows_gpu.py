"""The plain 4096-point kernels run pass-1 rows 9..15 as the negative frequencies a - 16 (their twiddle is the conjugate of a stored one),
so a thread's register row d holds bins [256 d - 7, 256 d + 249) instead of [256 d, 256 d + 256) (csrc/crn_kernels.h: lane_coord / bin_of).
On the MI355X: every bin where the two labellings differ or a row wraps lands where it belongs — through the LDS-walk close (spectrum
requests, the CFAR form) and through the register close on plans whose edges sit on both kinds of row boundary — and the pruned and
the unpruned kernel still agree bit for bit on the reference plan.  N = 4096, two frames per epoch, a handful of epochs."""
import numpy as np
import pytest

import cfar_f64 as cf
import crnsense as cs
import oracle_py as orc
import parity_policy as pol
import signals

pytestmark = pytest.mark.gpu

N = 4096
K = 2
LEAK = 1e-6 * float(N) ** 2          # what a unit tone may leave in any other bin or band (tests/test_gpu_parity.py)
OTHER = (2400, 2480)                 # a second band far from every edge under test (row 9 in both labellings)
# bins where the old and the new labelling differ, and where rows wrap
SPECTRUM_BINS = [0, 8, 9, 15, 16, 248, 249, 255, 256, 2047, 2048, 4087, 4088, 4089, 4095]
# (segments of band 0, the launch without a spectrum runs the kernel pruned to the reference plan's rows)
PLANS = [
    ([(240, 260)], True),
    ([(4089, 4096), (0, 9)], True),       # one band across the wrap
    ([(505, 512)], True),
    ([(760, 768)], False),                # inside the reference plan's unshifted rows, outside the shifted ones: the unpruned kernel
    ([(1273, 1280)], True),               # the other way round
]


def _cfg():
    cfg = cs.cfg_energy_scaled(N, 4.0)
    cfg.frames_per_epoch = K
    return cfg


def _tones(bins):
    """One epoch per bin: a unit tone on the grid, K frames of it."""
    t = np.arange(N)
    x = np.stack([np.tile(np.exp(2j * np.pi * (k % N) * t / N), K) for k in bins]).astype(np.complex64)
    return x.view(np.float32).ravel()


def test_spectrum_request_puts_every_bin_in_its_place(built):
    cfg = _cfg()
    iq = _tones(SPECTRUM_BINS)
    truth = signals.spectrum_f64(cfg, iq, len(SPECTRUM_BINS))
    s = cs.Sensor(cfg)
    got = s.run_host(iq, len(SPECTRUM_BINS), want_spectrum=True)["spectrum"]
    s.close()
    for i, k in enumerate(SPECTRUM_BINS):
        err = abs(got[i, k] / truth[i, k] - 1)
        rest = np.delete(got[i], k).max()
        print(f"tone at bin {k}: {got[i, k]:.6e} (float64 DFT {truth[i, k]:.6e}, rel. error {err:.2e}), largest other bin {rest:.3e}")
        assert err < pol.PER_BIN_TOL, k
        assert rest < LEAK, (k, int(np.argmax(np.where(np.arange(N) == k, 0, got[i]))))


@pytest.mark.parametrize("segs,pruned", PLANS, ids=[" + ".join(f"[{lo}, {hi})" for lo, hi in p[0]) for p in PLANS])
def test_register_close_on_plans_at_both_kinds_of_row_boundary(built, segs, pruned):
    cfg = _cfg()
    cfg.decide = cs.DECIDE_NONE
    cfg.n_bands = 2
    cfg.n_segs = len(segs) + 1
    for i, (lo, hi) in enumerate(segs):
        cfg.segs[i] = cs.BandSeg(lo, hi, 0)
    cfg.segs[len(segs)] = cs.BandSeg(OTHER[0], OTHER[1], 1)
    inside = {k for lo, hi in segs for k in range(lo, hi)}
    bins = [k % N for lo, hi in segs for k in (lo - 1, lo, hi - 1, hi)]
    iq = _tones(bins)
    s = cs.Sensor(cfg)
    name = s.kernel_info()["name"]
    assert "CLOSE=registers" in name, name
    assert ("PASS3_ROWS" in name) == pruned, name
    res = {want_spectrum: s.run_host(iq, len(bins), want_spectrum=want_spectrum) for want_spectrum in (True, False)}
    s.close()
    for want_spectrum, got in res.items():
        for i, k in enumerate(bins):
            f = got["features"][i]
            print(f"spectrum={want_spectrum} tone at bin {k}: band 0 {f[0]:.6e}, band 1 {f[1]:.3e}")
            if k in inside:
                assert abs(f[0] / float(N) ** 2 - 1) < pol.FEATURE_TOL, (k, want_spectrum)
            else:
                assert f[0] < LEAK, (k, want_spectrum)
            assert f[1] < LEAK, (k, want_spectrum)


def test_reference_plan_pruned_equals_unpruned_on_synth_traffic(built):
    torch = pytest.importorskip("torch")
    dev = "cuda"
    E = 64
    cfg = _cfg()
    spe = cs.samples_per_epoch(cfg)
    iq = torch.zeros(E * spe * 2, dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    res = []
    for v in (0, 2):
        s = cs.Sensor(cfg)
        s.set_variant(v)
        assert ("PASS3_ROWS=7-of-16" in s.kernel_info()["name"]) == (v == 0)
        if not res:
            s.synth_fill_device(iq.data_ptr(), E, spe, seed=4242, stream=stream)
        feats = torch.zeros(E, 4, dtype=torch.float32, device=dev)
        occ = torch.zeros(E, 4, dtype=torch.uint8, device=dev)
        s.run_device(iq.data_ptr(), E, N, {"features": feats.data_ptr(), "ann_out": 0, "decision": 0, "occupancy": occ.data_ptr(),
                                           "spectrum": 0}, stream=stream)
        torch.cuda.synchronize()
        s.close()
        res.append((feats.cpu().numpy(), occ.cpu().numpy()))
    assert res[0][0].tobytes() == res[1][0].tobytes()
    assert np.array_equal(res[0][1], res[1][1])
    want = orc.run(cfg, iq.cpu().numpy(), E)
    assert np.array_equal(res[0][1], want["occupancy"])
    assert res[0][1][:, 1:].any()      # the traffic drives channels


def test_cfar_mask_sets_exactly_the_tone_bin(built):
    torch = pytest.importorskip("torch")
    dev = "cuda"
    bins = [249, 255, 4089]
    cfg = _cfg()
    E = len(bins)
    # white noise of power 1e-6 per sample and, in epoch i, a tone 60 dB over the per-bin floor at bins[i].  alpha = 100: a noise bin is a
    # Gamma(K = 2) variable of mean 1 against a 32-cell average — exceeding 100 x has probability ~ 2e-42 per bin — and the tone is 1e6 x
    rng = np.random.default_rng(7)
    total = E * K * N
    x = rng.normal(0, np.sqrt(0.5e-6), total) + 1j * rng.normal(0, np.sqrt(0.5e-6), total)
    amp = np.sqrt(1e6 * 1e-6 / N)
    t = np.arange(K * N)
    for i, k in enumerate(bins):
        x[i * K * N:(i + 1) * K * N] += amp * np.exp(2j * np.pi * (k * t % N) / N)
    iq = torch.from_numpy(x.astype(np.complex64).view(np.float32).copy()).to(dev)
    s = cs.Sensor(cfg)
    s.set_cfar(2, 16, 100.0, 1)
    assert "lds+cfar" in s.kernel_info()["name"]
    mask = torch.zeros((E, N // 32), dtype=torch.int32, device=dev)
    feats = torch.zeros((E, 4), dtype=torch.float32, device=dev)
    s.run_device_cfar(iq.data_ptr(), E, N, {"features": feats.data_ptr(), "ann_out": 0, "decision": 0, "occupancy": 0, "spectrum": 0},
                      mask_ptr=mask.data_ptr())
    torch.cuda.synchronize()
    s.close()
    det = cf.unpack_mask(mask.cpu().numpy().view(np.uint32), N)
    for i, k in enumerate(bins):
        print(f"tone at bin {k}: detected bins {np.flatnonzero(det[i]).tolist()}")
        assert np.flatnonzero(det[i]).tolist() == [k]
