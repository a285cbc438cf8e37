"""The kernels that carry tracks across batches (csrc/crn_tracks_carry.hip) keep everything in registers and a little LDS: no scratch.
Like tests/test_tracks_resources.py this test compiles the file itself, for gfx950, with the library's flags and
-Rpass-analysis=kernel-resource-usage, and pins the scratch, the occupancy and the LDS of every kernel in it, and the file's place in
the Makefile.  Resource remarks only."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cognitive-radio-network_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

# LDS bytes per workgroup: link holds two lists of 256 (lo, width) pairs, gather the 256 roots of its row, scan four words per wave
LDS = {"carry_init_kernel": 0, "carry_link_kernel": 4096, "carry_gather_kernel": 1024, "carry_count_kernel": 0,
       "carry_scan_kernel": 256, "carry_emit_kernel": 0, "carry_tail_kernel": 0}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = tmp_path_factory.mktemp("tracks_carry") / "crn_tracks_carry.s"
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*:=\s*(.*?)\n(?=#)", mk, re.S | re.M).group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    r = subprocess.run([HIPCC, *flags, "--cuda-device-only", "-Wno-unused-command-line-argument", "-Rpass-analysis=kernel-resource-usage",
                        "-S", "-o", str(out), os.path.join(CSRC, "crn_tracks_carry.hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr


def _kernels(txt):
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
        name = b.split('\n')[0].strip().split(' ')[0]

        def g(k):
            m = re.search(k + r": (\d+)", b)
            return int(m.group(1)) if m else None
        dem = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
        short = re.search(r"(carry_\w+_kernel)", dem)
        out[short.group(1) if short else dem] = {"scratch": g(r"ScratchSize \[bytes/lane\]"), "occ": g(r"Occupancy \[waves/SIMD\]"),
                                                 "vgprs": g(r" VGPRs"), "lds": g(r"LDS Size \[bytes/block\]")}
    return out


def test_carry_kernels_do_not_spill(remarks):
    ks = _kernels(remarks)
    assert sorted(ks) == sorted(LDS), sorted(ks)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < 1}
    assert not bad, bad
    assert {n: k["lds"] for n, k in ks.items()} == LDS


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_tracks\.hip crn_tracks_carry\.hip\b", mk, re.M)          # after crn_tracks.hip
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    for objs in ("OBJS", "OBJS_AB", "OBJS_SC", "OBJS_PL"):
        assert re.search(r"^%s\s*:=.*(\$\(REST\)|\$\(H_SRCS:%%=\$\(O\)/%%\.o\))" % objs, mk, re.M), objs
    assert re.search(r"crn_tracks_carry\.hip\.o.*: \$\(HERE\)crn_segments\.h", mk)
