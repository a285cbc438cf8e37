"""The hop-count kernels (csrc/crn_hops.hip) keep a 64 x 64 matrix as one column per lane in registers: no scratch, no LDS.  Like
tests/test_occmap_resources.py this test compiles the file itself, for gfx950, with the library's flags and
-Rpass-analysis=kernel-resource-usage, and pins the scratch, the LDS and the occupancy DESIGN.md §5 states, from the compiler's remarks
alone."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_hops")


def test_hops_kernels_do_not_spill(compiled):
    ks = kernels(compiled[0], r"(hops_\w+_kernel)")
    assert sorted(ks) == ["hops_chunk_kernel", "hops_join_kernel"], sorted(ks)
    for n, k in ks.items():
        print(n, k)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < 1}
    assert not bad, bad
    # chunk: the lane's column of the matrix, 64 counts, next to the time words: registers only, five waves to a SIMD
    assert ks["hops_chunk_kernel"]["lds"] == 0 and ks["hops_chunk_kernel"]["occ"] >= 5 and ks["hops_chunk_kernel"]["vgprs"] >= 64
    # join: four cells of eight parts in flight per thread, no LDS (no thread needs another's sum), six waves to a SIMD
    assert ks["hops_join_kernel"]["lds"] == 0 and ks["hops_join_kernel"]["occ"] >= 6


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_occmap\.hip crn_cyclo\.hip crn_hops\.hip\b", mk, re.M)
    # the host objects every flavour shares are derived from H_SRCS (tests/test_tracks_resources.py checks that each flavour links them)
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    # the unit sees crn_segments.h (handle_geometry, in_grids, CHUNK) and not crn_mask_runs.h: it reads busy words, not the bin mask
    assert re.search(r"^\$\(O\)/crn_segments\.hip\.o.*\$\(O\)/crn_cyclo\.hip\.o \$\(O\)/crn_hops\.hip\.o.*: \$\(HERE\)crn_segments\.h$", mk, re.M)
    assert not re.search(r"crn_hops\.hip\.o.*: \$\(HERE\)crn_mask_runs\.h$", mk, re.M)
    src = open(os.path.join(CSRC, "crn_hops.hip")).read()
    assert "crn_mask_runs.h" not in src
    # integers only on the device: no floating-point type in any kernel or device function (the host's crn_hop_forecast is the one user)
    device = src[: src.index("const char *hop_params_refusal")]
    assert not re.search(r"\b(float|double)\b", re.sub(r"//.*", "", device))
