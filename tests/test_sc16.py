"""Samples kept in the radio's wire format (crn_sense_run_device_sc16: int16 pairs, 4 bytes per complex sample — what the reference's
USRPs put on the network, src/extensible_cognitive_radio.cpp:1263-1265): the kernel converts in its first pass exactly as UHD's
converter does (int16 / 32768), so every output must be BIT-IDENTICAL to the float path on the converted samples — and through it
equal to the oracle within the float path's own tolerance."""
import ctypes as C
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import crnsense as cs
import forms
import oracle_py as orc

# The wire-format kernels and their five entry points are OPTIONAL (make -C csrc SC16=1 -> libcrnsense_sc16.so): the default library does
# not carry them.  The tests of this file run when the loaded library has them ($CRN_SENSE_LIB=.../libcrnsense_sc16.so) and skip
# otherwise; test_wire_format_suite_on_the_optional_library runs them that way in a child process whenever that library was built.
HAVE = cs.has_sc16()
needs_sc16 = pytest.mark.skipif(not HAVE, reason="the loaded library was built without the optional wire-format kernels (make SC16=1)")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _child_suite(marker, at_least):
    """Runs this file (and the wire-format dealt-frame test) in a child process against libcrnsense_sc16.so.  ADVICE r05: the parent's
    "1 passed" must stand for the whole child suite — so the child's own count is asserted (>= at_least, none skipped) and, on an
    evidence pass ($CRN_EVIDENCE_DIR), its last line is kept under profiles/."""
    if HAVE:
        pytest.skip("already running against a library with the wire-format kernels")
    if not os.path.exists(cs.SC16_LIB_PATH):
        pytest.skip("libcrnsense_sc16.so was not built (make -C csrc SC16=1)")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", marker, "-k", "not optional_library and not default_library", "-p", "no:cacheprovider", os.path.abspath(__file__),
                        os.path.join(ROOT, "tests", "test_dealt_frames.py") + "::test_dealt_frames_in_the_wire_format"],
                       cwd=ROOT, env=dict(os.environ, CRN_SENSE_LIB=cs.SC16_LIB_PATH), capture_output=True, text=True, timeout=1500)
    tail = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else ""
    assert r.returncode == 0 and " passed" in tail and "skipped" not in tail, r.stdout[-3000:] + r.stderr[-2000:]
    n_passed = int(tail.split(" passed")[0].split()[-1])
    assert n_passed >= at_least, f"the child suite ran {n_passed} tests, expected at least {at_least}: {tail}"
    d = os.environ.get("CRN_EVIDENCE_DIR")
    if d and os.path.isdir(d):
        with open(os.path.join(d, f"wire_format_child_suite_{marker.replace(' ', '_')}.txt"), "w") as f:
            f.write(f"pytest -m '{marker}' tests/test_sc16.py + test_dealt_frames_in_the_wire_format with CRN_SENSE_LIB=libcrnsense_sc16.so (child process):\n{tail}\n")
    return tail


def test_default_library_has_no_wire_format_entry_points(built):
    """... and says so: the binding raises instead of calling into nothing, and the library itself answers a wire-format launch
    (which only an internal caller could request) with an error, not a crash."""
    if HAVE:
        pytest.skip("running against a library with the wire-format kernels")
    L = cs.lib()
    assert not any(hasattr(L, name) for name in cs.SC16_EXPORTS)
    with pytest.raises(cs.CrnError, match="SC16=1"):
        cs._need_sc16("x")


def test_wire_format_host_checks_on_the_optional_library(built):
    print(_child_suite("not gpu", 1))


@pytest.mark.gpu
def test_wire_format_suite_on_the_optional_library(built):
    print(_child_suite("gpu", 44))


@needs_sc16
def test_sc16_argument_errors(built):
    L = cs.lib()
    o = cs.Out()
    assert L.crn_sense_run_device_sc16(None, None, 1, 512, 0, C.byref(o), None) == cs.CRN_ERR_ARG
    assert L.crn_pack_sc16_device(None, None, 1, None, None) == cs.CRN_ERR_ARG


def _cfgs():
    yield "ref512", cs.cfg_reference(), 512
    yield "ref512_L364", cs.cfg_reference(), 364
    yield "ref512_L1", cs.cfg_reference(), 1
    for n in (512, 1024, 2048, 4096):
        yield f"energy{n}", cs.cfg_energy_scaled(n, 4.0), n
    yield "energy4096_L3000", cs.cfg_energy_scaled(4096, 4.0), 3000
    c = cs.cfg_energy_scaled(4096, 4.0)          # a band outside the reference plan's rows: the unpruned 4096-point kernel
    c.segs[2].lo, c.segs[2].hi = 900, 1100
    yield "energy4096_other_plan", c, 4096
    c = cs.cfg_energy_scaled(1024, 4.0)
    c.mode = cs.MODE_REF_MAG
    yield "mag1024", c, 1024
    for n in (1024, 4096):
        yield f"welch{n}", cs.cfg_welch(n, 8, 64), n
    c = cs.cfg_welch(4096, 5, 16)               # 256-bin aligned bands
    yield "welch4096_16bands", c, 4096
    for n in (512, 1024, 2048, 4096):           # the generic windowed kernels: Blackman-Harris (the monitor's window), magnitudes, short frames
        c = cs.cfg_energy_scaled(n, 4.0)
        c.window = cs.WINDOW_BLACKMAN_HARRIS
        yield f"bh{n}", c, n
    c = cs.cfg_welch(1024, 8, 64)
    c.mode = cs.MODE_REF_MAG
    yield "welch1024_mag", c, 1024
    c = cs.cfg_energy_scaled(2048, 4.0)
    c.window = cs.WINDOW_HANN
    yield "hann2048_L1500", c, 1500


@needs_sc16
@pytest.mark.gpu
@pytest.mark.parametrize("name,cfg,L", list(_cfgs()), ids=[n for n, _, _ in _cfgs()])
@pytest.mark.parametrize("want_spectrum", [False, True], ids=["", "spectrum"])
def test_wire_format_is_bit_identical_to_the_float_path(built, name, cfg, L, want_spectrum):
    import torch
    dev = torch.device("cuda", 0)
    n = 37
    spe = cs.samples_per_epoch(cfg, L)
    need = cs.samples_needed(cfg, n, L)
    rng = np.random.default_rng(zlib.crc32(name.encode()))   # reproducible per configuration
    raw = rng.integers(-2000, 2000, (need, 2), dtype=np.int16)
    raw[rng.random(need) < 0.01] = rng.integers(-32768, 32767, 2, dtype=np.int16)        # full-scale excursions, both extremes
    raw[0], raw[1] = (-32768, 32767), (32767, -32768)
    host_f = (raw.astype(np.float32) / np.float32(32768.0)).ravel()                       # UHD's sc16 -> fc32 conversion
    d_raw = torch.from_numpy(raw.copy()).to(dev)
    d_f = torch.from_numpy(host_f).to(dev)
    for k in range(cfg.n_bands):
        if np.isfinite(cfg.thresh[k]) and cfg.ref_band < 0:
            cfg.thresh[k] = 1e-3
    want = orc.run(cfg, host_f, n, L=L)
    # 37 epochs: by its own choice the library deals them at 512 / 1024 points.  Both forms, each named (tests/forms.py) and checked to have
    # run — the streaming one is what large batches run, the dealt one (where the configuration has it) what this launch gets by default
    for form in ("streaming", "dealt"):
        s = forms.sensor(cfg, form)
        outs = []
        for _ in range(2):
            feats = torch.zeros(n, cfg.n_bands, device=dev)
            ann = torch.zeros(n, 3, dtype=torch.float64, device=dev)
            dec = torch.full((n,), -7, dtype=torch.int32, device=dev)
            occ = torch.full((n, cfg.n_bands), 9, dtype=torch.uint8, device=dev)
            spec = torch.zeros(n, cfg.fft_len, device=dev) if want_spectrum else None
            outs.append((feats, ann, dec, occ, spec))
        ptrs = [{"features": o[0].data_ptr(), "ann_out": o[1].data_ptr(), "decision": o[2].data_ptr(), "occupancy": o[3].data_ptr(),
                 "spectrum": o[4].data_ptr() if want_spectrum else 0} for o in outs]
        s.run_device(d_f.data_ptr(), n, L, ptrs[0])
        s.run_device(d_raw.data_ptr(), n, L, ptrs[1], sc16=True)
        torch.cuda.synchronize()
        forms.assert_ran(s, form, 2, L=L)
        for a, b in zip(outs[0], outs[1]):
            if a is not None:
                assert torch.equal(a, b), form                                                # bit for bit
        assert np.allclose(outs[1][0].cpu().numpy(), want["features"], rtol=3e-5, atol=0), form
        s.close()
    # the device packer inverts the conversion exactly
    s = cs.Sensor(cfg)
    packed = torch.zeros(need, 2, dtype=torch.int16, device=dev)
    s.pack_sc16_device(d_f.data_ptr(), need, packed.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(packed, d_raw)
    s.close()


@needs_sc16
@pytest.mark.gpu
def test_wire_format_argument_checks(built):
    import torch
    cfg = cs.cfg_welch(1024, 8, 64)
    s = cs.Sensor(cfg)
    x = torch.zeros(cs.samples_needed(cfg, 4), 2, dtype=torch.int16, device="cuda")
    f = torch.zeros(4, 64, device="cuda")
    with pytest.raises(cs.CrnError) as ei:   # int16 pairs are 4-byte units
        s.run_device(x.data_ptr() + 2, 4, 1024, {"features": f.data_ptr(), "ann_out": 0, "decision": 0, "occupancy": 0, "spectrum": 0}, sc16=True)
    assert "4-byte aligned" in str(ei.value)
    s.close()


@needs_sc16
@pytest.mark.gpu
def test_wire_format_ring_matches_the_float_ring(built):
    """The ingest ring fed int16 packets (crn_ingest_create_sc16 / crn_ingest_push_sc16) against the ring fed the same samples as
    complex floats: the same (stream, epoch) results, bit for bit, reference-sized packets (364 of 512)."""
    cfg = cs.cfg_reference()
    rng = np.random.default_rng(77)
    S, E, L = 3, 6, 364
    raw = rng.integers(-3000, 3000, (S, E, 10, L, 2), dtype=np.int16)
    got = {}
    for sc16 in (False, True):
        sn = cs.Sensor(cfg)
        ring = cs.Ingest(sn, S, L, 4, sc16=sc16)
        res = []
        for e in range(E):
            for p in range(10):
                for st in range(S):
                    pk = raw[st, e, p] if sc16 else (raw[st, e, p].astype(np.float32) / np.float32(32768.0))
                    ring.push(st, np.ascontiguousarray(pk))
            res += ring.poll()
        ring.drain()
        res += ring.poll()
        got[sc16] = {(r.stream, r.epoch_seq): (r.decision, tuple(r.features[:4]), tuple(r.ann_out)) for r in res}
        assert len(got[sc16]) == S * E
        if sc16:
            with pytest.raises(cs.CrnError):
                cs.check(cs.lib().crn_ingest_push(ring._g, 0, np.zeros(2 * L, np.float32).ctypes.data), "crn_ingest_push")
        ring.close()
        sn.close()
    assert got[True] == got[False]


@needs_sc16
@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["ref512_L364", "energy4096", "welch1024"])
def test_wire_format_with_another_converter_constant(built, mode):
    """UHD's sc16 -> fc32 converter scales by 1/32767, not 1/32768.  crn_sense_set_wire_full_scale(32767): the wire path against the
    float path fed k * float(1/32767) — no longer bit for bit (the float path rounds the scaled samples one by one), equal to ~1e-6."""
    import torch
    cfg, L = {"ref512_L364": (cs.cfg_reference(), 364), "energy4096": (cs.cfg_energy_scaled(4096, 4.0), 4096),
              "welch1024": (cs.cfg_welch(1024, 8, 64), 1024)}[mode]
    n = 25
    need = cs.samples_needed(cfg, n, L)
    rng = np.random.default_rng(5)
    raw = rng.integers(-4000, 4000, (need, 2), dtype=np.int16)
    raw[:8] = [(32767, -32768), (-32768, 32767), (20000, -20000), (16384, 16383), (-16384, -16385), (1, -1), (0, 0), (30000, 29999)]
    host_f = (raw.astype(np.float32) * np.float32(1.0 / 32767.0)).ravel()
    s = cs.Sensor(cfg)
    with pytest.raises(cs.CrnError):
        s.set_wire_full_scale(0.5)
    s.set_wire_full_scale(32767.0)
    feats = [torch.zeros(n, cfg.n_bands, device="cuda") for _ in range(2)]
    spec = [torch.zeros(n, cfg.fft_len, device="cuda") for _ in range(2)]
    dec = [torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2)]
    ann = [torch.zeros(n, 3, dtype=torch.float64, device="cuda") for _ in range(2)]
    for i, (buf, sc) in enumerate(((torch.from_numpy(host_f).cuda(), False), (torch.from_numpy(raw).cuda(), True))):
        s.run_device(buf.data_ptr(), n, L, {"features": feats[i].data_ptr(), "ann_out": ann[i].data_ptr(), "decision": dec[i].data_ptr(),
                                            "occupancy": 0, "spectrum": spec[i].data_ptr()}, sc16=sc)
    torch.cuda.synchronize()
    packed = torch.zeros(need, 2, dtype=torch.int16, device="cuda")      # the packer uses the same constant: exact inverse again
    s.pack_sc16_device(torch.from_numpy(host_f).cuda().data_ptr(), need, packed.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(packed.cpu().numpy(), raw)
    f0, f1 = feats[0].cpu().numpy(), feats[1].cpu().numpy()
    assert not np.array_equal(f0, f1) and np.allclose(f0, f1, rtol=2e-6, atol=0)
    assert np.allclose(spec[0].cpu().numpy(), spec[1].cpu().numpy(), rtol=1e-5, atol=1e-5 * float(spec[0].mean()))
    if cfg.decide == cs.DECIDE_ANN:
        assert torch.equal(dec[0], dec[1])
    s.close()


if not HAVE:
    # Nothing of the above can run in this process; it runs in the child (test_wire_format_suite_on_the_optional_library).  Take the
    # tests out of this process's collection instead of reporting 40-odd "skipped": a skip should mean something did not run anywhere.
    for _name in [n for n in list(globals()) if n.startswith("test_") and n not in (
            "test_default_library_has_no_wire_format_entry_points", "test_wire_format_host_checks_on_the_optional_library",
            "test_wire_format_suite_on_the_optional_library")]:
        del globals()[_name]
