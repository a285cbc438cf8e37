"""The spectrum-hole kernels (csrc/crn_holes.hip) keep everything in registers and LDS: no scratch.  Like tests/test_fuse_resources.py this
test compiles the file itself, for gfx950, with the library's flags and -Rpass-analysis=kernel-resource-usage, and pins the scratch and the
LDS of every kernel in it: one instantiation of each per fft_len."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels

SIZES = (512, 1024, 2048, 4096)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_holes")


def test_hole_kernels_do_not_spill(compiled):
    ks = kernels(compiled[0], r"(holes_\w+_kernel<\d+>)")
    last = {n: "holes_last_kernel<%d>" % n for n in SIZES}
    stream = {n: "holes_stream_kernel<%d>" % (n // 64) for n in SIZES}
    assert sorted(ks) == sorted(list(last.values()) + list(stream.values())), sorted(ks)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < 1}
    assert not bad, bad
    # DESIGN.md §5.  last: the chunk's 64 dilated rows of N / 32 words (8 N bytes).  stream: Pbar and the ages, each N words and 4 words of
    # padding per lane piece (2 x (4 N + 1024) bytes), and the free mask (N / 8 bytes)
    assert {n: ks[last[n]]["lds"] for n in SIZES} == {n: 8 * n for n in SIZES}
    assert {n: ks[stream[n]]["lds"] for n in SIZES} == {n: 8 * n + 2048 + n // 8 for n in SIZES}
    for n in SIZES:
        print(last[n], ks[last[n]])
        print(stream[n], ks[stream[n]])


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_holes\.hip\b", mk, re.M)
    # the host objects every flavour shares are derived from H_SRCS (tests/test_tracks_resources.py checks that each flavour links them)
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    # the unit sees crn_segments.h (handle_geometry): it is on that header's dependency line, behind the fusion
    assert re.search(r"^\$\(O\)/crn_segments\.hip\.o.*\$\(O\)/crn_fuse\.hip\.o \$\(O\)/crn_holes\.hip\.o.*: \$\(HERE\)crn_segments\.h$", mk, re.M)
