"""The fusion kernel (csrc/crn_fuse.hip) keeps everything in registers and LDS: no scratch.  Like tests/test_channels_resources.py this
test compiles the file itself, for gfx950, with the library's flags and -Rpass-analysis=kernel-resource-usage, and pins the scratch and the
LDS of every kernel in it: one instantiation per fft_len."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels

THREADS = {512: 128, 1024: 256, 2048: 256, 4096: 256}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_fuse")


def test_fuse_kernels_do_not_spill(compiled):
    ks = kernels(compiled[0], r"(fuse_kernel<\d+, \d+>)")
    names = {n: "fuse_kernel<%d, %d>" % (n, t) for n, t in THREADS.items()}
    assert sorted(ks) == sorted(names.values()), sorted(ks)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < 1}
    assert not bad, bad
    # the fused row as fp64 (8 N bytes) and four counters (16 bytes)
    assert {n: ks[names[n]]["lds"] for n in THREADS} == {n: 8 * n + 16 for n in THREADS}
    for n in THREADS:
        print(names[n], ks[names[n]])


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_fuse\.hip\b", mk, re.M)
    # the host objects every flavour shares are derived from H_SRCS (tests/test_tracks_resources.py checks that each flavour links them)
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    # the unit sees crn_segments.h (handle_geometry): it is on that header's dependency line
    assert re.search(r"^\$\(O\)/crn_segments\.hip\.o.*\$\(O\)/crn_fuse\.hip\.o.*: \$\(HERE\)crn_segments\.h$", mk, re.M)
