"""The resampling kernels (csrc/crn_resample.hip) stage a tile's input span, 4 x 256 + T complex words, in LDS once and read the
polyphase table through the cache.  Like tests/test_extract_resources.py this test compiles the file itself, for gfx950, with the
library's flags and -Rpass-analysis=kernel-resource-usage, and pins the scratch, the LDS and the occupancy DESIGN.md §5 states, from the
compiler's remarks alone."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_resample")


def test_resample_kernels_do_not_spill(compiled):
    ks = {k: v for k, v in kernels(compiled[0], r"resample_kernel<(\d+)>").items() if k.isdigit()}
    cs = {k: v for k, v in kernels(compiled[0], r"carry_kernel<(\d+)>").items() if k.isdigit()}
    for n in ("8", "16", "32"):
        assert n in ks and n in cs, (sorted(ks), sorted(cs))
        print(n, ks[n], cs[n])
        # the span of a tile and nothing else: (1024 + T) complex words to a wave.  It is the LDS that bounds the occupancy, 160 KB to a
        # compute unit: 19 workgroups of one wave, so four waves to every SIMD and a fifth to three of them.  The compiler reports 5, 5
        # and 4 waves to a SIMD with 52, 78 and 98 VGPRs at T = 8, 16 and 32; the registers are held to the next step of
        # eight above those
        occ, vgprs = {"8": (5, 56), "16": (5, 80), "32": (4, 104)}[n]
        assert ks[n]["scratch"] == 0 and ks[n]["lds"] == (1024 + int(n)) * 8 and ks[n]["occ"] >= occ and ks[n]["vgprs"] <= vgprs, (n, ks[n])
        assert cs[n]["scratch"] == 0 and cs[n]["lds"] == 0 and cs[n]["occ"] >= 8, (n, cs[n])
    assert sorted(ks, key=int) == ["8", "16", "32"] == sorted(cs, key=int)


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_hops\.hip crn_extract\.hip crn_resample\.hip\b", mk, re.M)
    # the host objects every flavour shares are derived from H_SRCS (tests/test_tracks_resources.py checks that each flavour links them)
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    # the unit sees crn_segments.h (handle_geometry, in_grids)
    assert re.search(r"^\$\(O\)/crn_segments\.hip\.o.*\$\(O\)/crn_extract\.hip\.o \$\(O\)/crn_resample\.hip\.o.*: \$\(HERE\)crn_segments\.h$", mk, re.M)
    src = open(os.path.join(CSRC, "crn_resample.hip")).read()
    assert "atomic" not in re.sub(r"//.*", "", src)
