"""What test_cfar_gpu.py and test_cfar_methods_gpu.py share: the plan, the launch through either entry point, the cases of the twin
comparison with its tolerance band, and two kinds of traffic made on the host.  A plain module, not collected."""
import numpy as np
import torch

import crnsense as cs
import parity_policy as pol
import signals
import stage_gpu as sgpu

# The band the comparison leaves out: |P / (alpha Z) - 1| <= DELTA_FACTOR x parity_policy.snr_bound at the traffic's in-band SNR.
# Started at 4 x (1.57e-4 here): on the MI355X the kernel and the twin then disagreed at no bin of any case, and at most one bin of a
# case fell inside the band.  Tightened to 2 x: the fp32 ratio carries the per-bin error of P and, at most as large, that of Z.
DELTA_FACTOR = 2.0


def cfg(n, window, k, decide=cs.DECIDE_THRESHOLD):
    c = sgpu.cfg(n, window, k)
    c.decide = decide
    return c


def run(s, cfg, iq_t, E, L, cfar=True, spectrum=True, first=0, count=None, outs=None):
    """One launch over epochs [first, first + count) into the (optionally given) full-size output tensors."""
    N, nb = cfg.fft_len, cfg.n_bands
    count = E - first if count is None else count
    if outs is None:
        outs = {"features": sgpu.zeros((E, nb), torch.float32), "decision": sgpu.zeros((E,), torch.int32),
                "occupancy": sgpu.zeros((E, nb), torch.uint8), "spectrum": sgpu.zeros((E, N), torch.float32) if spectrum else None,
                "mask": sgpu.zeros((E, N // 32), torch.int32), "band_bins": sgpu.zeros((E, nb), torch.int32)}
    spe = cs.samples_per_epoch(cfg, L)
    ptr = {k: (v[first].data_ptr() if v is not None else 0) for k, v in outs.items()}
    o = {"features": ptr["features"], "ann_out": 0, "decision": ptr["decision"], "occupancy": ptr["occupancy"], "spectrum": ptr["spectrum"]}
    iq_ptr = iq_t.data_ptr() + first * spe * 8
    if cfar:
        s.run_device_cfar(iq_ptr, count, L, o, mask_ptr=ptr["mask"], band_bins_ptr=ptr["band_bins"])
    else:
        s.run_device(iq_ptr, count, L, o)
    return outs


def host(outs):
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if v is not None else None) for k, v in outs.items()}


def snr(cfg):
    return max(pol.in_band_snr_db(0.02, 1e-6, signals.band_bins(cfg, b).size, cfg.fft_len) for b in range(1, cfg.n_bands))


CASES = [(n, w, k, n) for n in (512, 1024, 2048, 4096) for w in (cs.WINDOW_RECT, cs.WINDOW_HANN, cs.WINDOW_BLACKMAN_HARRIS) for k in (1, 10)]
CASES.append((1024, cs.WINDOW_RECT, 10, 700))   # short packets: L < N, zero-padded


def strong_tones(cfg, E, db, seed):
    """Complex white noise (power 1e-6 per sample) plus on-grid tones `db` over the per-bin noise floor, one every N / 8 bins at
    sixteen different offsets within a thread's 16-bin block (bins 64 + j N / 8 + 3 j)."""
    n, k = cfg.fft_len, cfg.frames_per_epoch
    total = E * k * (cfg.hop if cfg.hop != n else n) + (n - cfg.hop if cfg.hop != n else 0)
    rng = np.random.default_rng(seed)
    x = (rng.normal(0, np.sqrt(0.5e-6), total) + 1j * rng.normal(0, np.sqrt(0.5e-6), total))
    amp = np.sqrt(10 ** (db / 10) * 1e-6 / n)          # |X|^2 = amp^2 N^2 against a floor of N 1e-6 (rect)
    m = np.arange(total)
    tones = [64 + j * (n // 8) + 3 * j for j in range(8)]
    for kb in tones:
        x += amp * np.exp(2j * np.pi * (kb * m % n) / n)
    return x.astype(np.complex64).view(np.float32).copy(), tones


def coloured(n, k, E, tone_bin, seed):
    """Frames built in the frequency domain: bins [0, N/2) at power 1, [N/2, N) 10 dB above, a tone 20 dB over the low floor."""
    rng = np.random.default_rng(seed)
    pw = np.where(np.arange(n) < n // 2, 1.0, 10.0)
    X = (rng.normal(size=(E * k, n)) + 1j * rng.normal(size=(E * k, n))) * np.sqrt(pw / 2)
    X[:, tone_bin] += 10.0 * np.exp(2j * np.pi * rng.uniform(size=E * k))
    x = np.fft.ifft(X, axis=1) * 1e-3
    return x.astype(np.complex64).view(np.float32).reshape(-1).copy()
