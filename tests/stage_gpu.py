"""What the GPU tests of the stages behind the CFAR launch share (test_cfar_gpu.py .. test_tcfar_gpu.py): the plan and the launch they
all start from, output arrays with a guard band behind them, the cost measurement behind every speed bar of DESIGN.md §5, and that
measurement's 2.18 GB batch.  A plain module, not collected; every helper here is the one copy of what each stage file used to carry."""
import numpy as np
import torch

import crnsense as cs
from mask_bits import pack_mask

DEV = "cuda"
PAD = 256                      # bytes of 0xFF kept behind every array of a Padded


def cfg(n, window=cs.WINDOW_RECT, k=10, bands=None):
    """The energy plan at n points (the Welch plan of `bands` equal bands if given), k frames per epoch, half-overlapped under Hann."""
    c = cs.cfg_energy_scaled(n) if bands is None else cs.cfg_welch(n, k, bands)
    c.window = window
    c.hop = n // 2 if window == cs.WINDOW_HANN else n
    c.frames_per_epoch = k
    return c


def zeros(shape, dtype, device=DEV):
    return torch.zeros(shape, dtype=dtype, device=device)


def upload_rows(P):
    """`spectrum` rows made on the host, as float32 on the device."""
    return torch.from_numpy(np.ascontiguousarray(P, np.float32)).to(DEV)


def upload_mask(det):
    """[E][N] bool -> the packed mask on the device, int32 words as the CFAR launch's own."""
    return torch.from_numpy(pack_mask(det).view(np.int32)).to(DEV)


def cfar_outs(cfg, E, spectrum=True, band_bins=True):
    """Zeroed device tensors for the outputs of a CFAR launch over E epochs: features, decision, occupancy, spectrum [E][N] (None if not
    asked), mask [E][N / 32] int32 and, if asked, band_bins."""
    N, nb = cfg.fft_len, cfg.n_bands
    outs = {"features": zeros((E, nb), torch.float32), "decision": zeros((E,), torch.int32), "occupancy": zeros((E, nb), torch.uint8),
            "spectrum": zeros((E, N), torch.float32) if spectrum else None, "mask": zeros((E, N // 32), torch.int32)}
    if band_bins:
        outs["band_bins"] = zeros((E, nb), torch.int32)
    return outs


def cfar_launch(s, cfg, iq_t, E, outs=None, spectrum=True, band_bins=True):
    """One CFAR launch over E epochs into `outs`, which it returns: cfar_outs with the two switches unless given; an output that `outs`
    does not hold is not asked of the launch."""
    if outs is None:
        outs = cfar_outs(cfg, E, spectrum, band_bins)
    ptr = {name: 0 if outs.get(name) is None else outs[name].data_ptr() for name in ("features", "decision", "occupancy", "spectrum", "mask", "band_bins")}
    o = {"features": ptr["features"], "ann_out": 0, "decision": ptr["decision"], "occupancy": ptr["occupancy"], "spectrum": ptr["spectrum"]}
    s.run_device_cfar(iq_t.data_ptr(), E, cfg.fft_len, o, mask_ptr=ptr["mask"], band_bins_ptr=ptr["band_bins"])
    return outs


class Padded:
    """Named byte arrays (name=bytes), each an attribute holding a uint8 tensor with PAD more bytes behind the payload, all 0xFF at first,
    so that whatever a kernel skipped, or wrote past the end, shows.  host() fetches them; raw, view() and pads_untouched() speak of
    the last host()."""

    def __init__(self, device=DEV, **sizes):
        self.device, self.sizes = device, sizes
        for name, nb in sizes.items():
            setattr(self, name, torch.full((nb + PAD,), 255, dtype=torch.uint8, device=device))

    def host(self):
        """{name: the payload bytes} after a synchronise; also kept as .raw."""
        if self.device == "cuda":
            torch.cuda.synchronize()
        whole = {name: getattr(self, name).cpu().numpy() for name in self.sizes}
        self.pads = {name: whole[name][nb:] for name, nb in self.sizes.items()}
        self.raw = {name: whole[name][:nb] for name, nb in self.sizes.items()}
        return self.raw

    def pads_untouched(self):
        return all((p == 255).all() for p in self.pads.values())

    def view(self, name, dtype, shape=-1):
        return np.frombuffer(self.raw[name].tobytes(), np.dtype(dtype)).reshape(shape)


def best_of_windows(arms, windows=5, launches=8, warm_up=True, report=True):
    """The cost measurement: {name: [ms per launch of each window]} for the closures of `arms`.  Every arm is called once and the device
    drained (warm_up); then, `windows` times, the arms take turns in dict order, so that a drift of the clocks meets all of them alike.
    A window is `launches` calls issued back to back behind one already queued, so the device never waits for the host inside it,
    timed by device events.  The caller takes min() of each list: the best window counts."""
    if warm_up:
        for fn in arms.values():
            fn()
        torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(windows):
        for name, fn in arms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            fn()
            a.record()
            for _ in range(launches):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / launches)
    if report:
        for name, v in times.items():
            print(f"ms per launch, {name}:", " ".join(f"{x:.4f}" for x in v))
    return times


def noise_batch(E, k, n, seed=5):
    """Unit white noise for E epochs of k frames of n points, interleaved I/Q: 6656 x 10 x 4096 x 8 B = 2.18 GB in the cost tests."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return torch.randn(E * k * n * 2, generator=gen, device=DEV, dtype=torch.float32)


def add_tones(iq_t, E, k, n):
    """Real traffic over noise_batch: one of the three channels of the energy plan driven in two epochs of three (8 tones; 0.02 rms over
    the unit noise would vanish, so 0.3: scaled to the generator's noise power 1), so that epochs carry segments as well as false alarms."""
    t = torch.arange(n, device=DEV, dtype=torch.float32)
    frames = iq_t.view(E, k, n, 2)
    for j, b in enumerate((300, 301, 302, 303, 1600, 1601, 1602, 3000)):
        ph = 2 * np.pi * ((b * t) % n) / n
        sel = slice(j % 3, E, 3)
        frames[sel, :, :, 0] += 0.3 * torch.cos(ph)
        frames[sel, :, :, 1] += 0.3 * torch.sin(ph)
    return iq_t
