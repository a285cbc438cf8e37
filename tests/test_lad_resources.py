"""The excised-floor detector's kernel (csrc/crn_lad.hip) keeps a lane's bins in registers and the row in LDS: no scratch.  Like
tests/test_holes_resources.py this test compiles the file itself, for gfx950, with the library's flags and
-Rpass-analysis=kernel-resource-usage, and pins the scratch and the LDS of every kernel in it: one instantiation per fft_len."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels

SIZES = (512, 1024, 2048, 4096)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_lad")


def test_lad_kernel_does_not_spill(compiled):
    ks = kernels(compiled[0], r"(lad_kernel<\d+>)")
    names = {n: "lad_kernel<%d>" % (n // 64) for n in SIZES}
    assert sorted(ks) == sorted(names.values()), sorted(ks)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < 1}
    assert not bad, bad
    # the row, N words and 4 words of padding per lane piece
    assert {n: ks[names[n]]["lds"] for n in SIZES} == {n: 4 * n + 1024 for n in SIZES}
    for n in SIZES:
        print(names[n], ks[names[n]])


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_holes\.hip crn_lad\.hip\b", mk, re.M)
    # the host objects every flavour shares are derived from H_SRCS (tests/test_tracks_resources.py checks that each flavour links them)
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    # the unit sees crn_segments.h (handle_geometry) and crn_mask_runs.h: it is on both headers' dependency lines, behind the holes
    assert re.search(r"^\$\(O\)/crn_segments\.hip\.o.*\$\(O\)/crn_holes\.hip\.o \$\(O\)/crn_lad\.hip\.o.*: \$\(HERE\)crn_segments\.h$", mk, re.M)
    assert re.search(r"^\$\(O\)/crn_segments\.hip\.o \$\(O\)/crn_holes\.hip\.o \$\(O\)/crn_lad\.hip\.o.*: \$\(HERE\)crn_mask_runs\.h$", mk, re.M)
