"""Which form of the sensing kernel a test means.  A plain module, no fixtures.

At 512 / 1024 points the library has two forms of the same arithmetic (csrc/crn_sense_kernel.h): the STREAMING kernel (an epoch is one
lane group running its K frames one after the other; what large batches and bench.py run) and the DEALT-frame kernel (one epoch per
workgroup, its frames spread over the lane groups; what a launch of at most one epoch per compute unit runs by default).  Which one a
launch gets is decided from its size (crn_api.cpp, run_device_impl), so a test that only names a configuration changes subject when
that rule changes — tests/test_gpu_parity.py's streaming tests ran the dealt kernel for every 512 / 1024-point case of at most 256
epochs.  A test that is about one form says so here and checks afterwards that that form ran:

    s = forms.sensor(cfg, "streaming")
    got = s.run_host(iq, n_epochs)
    forms.assert_ran(s, "streaming", 1)
"""
import crnsense as cs

CODES = {"auto": 400, "streaming": 401, "dealt": 402}      # crn_sense_set_variant: the dealt form by size / never / at any batch size
LDS_BUDGET = 160 * 1024                                    # per workgroup on gfx950 (hipDeviceAttributeMaxSharedMemoryPerBlock)


def has_dealt_form(cfg, L=None, lds_budget=LDS_BUDGET):
    """The rule of crn::sense_deal_rounds (csrc/crn_forms.cpp) restated: 512 / 1024 points, at least two frames to deal, no window
    (any packet length, both modes) or the periodic Hann in energy mode on whole frames, and the frame slots fit the workgroup's LDS.
    (A handle with CFAR on has no dealt form either; a cfg does not say.)"""
    n, K = cfg.fft_len, cfg.frames_per_epoch
    L = n if L is None else L
    if n not in (512, 1024) or K < 2:
        return False
    mag = cfg.mode == cs.MODE_REF_MAG
    if cfg.window != cs.WINDOW_RECT and (mag or cfg.window != cs.WINDOW_HANN or L != n):
        return False
    r3 = n // 256
    t = 16 * r3
    groups = 256 // t
    rounds = (K + groups - 1) // groups
    # exchange buffers + pass-2 twiddles, kCloseLdsBytes (crn_forms.h: kBandTabWords = 656 words of crn_kernels.h + 8 x 16 floats), frame slots
    lds = (groups * 16 * (t + r3) + 16 * r3) * 8 + (656 * 4 + 8 * 16 * 4) + rounds * groups * n * (4 if mag else 8)
    return lds <= lds_budget


def sensor(cfg, form):
    """A Sensor on `cfg` pinned to `form`: "streaming", "dealt" (wherever a dealt form exists) or "auto" (the library's own choice)."""
    s = cs.Sensor(cfg)
    s.set_variant(CODES[form])
    return s


def assert_ran(s, form, launches, L=None):
    """After `launches` sensing launches of packet length L on a fresh sensor(cfg, form): none of them dealt for "streaming", all of
    them for "dealt" where the configuration has a dealt form (and none where it has not: the streaming kernel takes the launch).
    "auto" has no count of its own: compare s.dealt_launches() with what the epoch count should have picked."""
    n_dealt = s.dealt_launches()
    if form == "streaming":
        want = 0
    elif form == "dealt":
        want = launches if has_dealt_form(s.cfg, L) else 0
    else:
        raise ValueError(f"assert_ran: no fixed expectation for form {form!r}")
    assert n_dealt == want, f"{form}: {n_dealt} of {launches} launches ran the dealt-frame kernel, expected {want}"
