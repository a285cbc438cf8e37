"""The kernel of the cyclic-spectrum stage (csrc/crn_cyclo.hip): a lane keeps the F products of a pair and the F fp64 sums of its
separation in registers, every index a compile-time constant: no scratch at any F.  Like tests/test_measure_resources.py this test
compiles the file itself, for gfx950, with the library's flags and -Rpass-analysis=kernel-resource-usage, and pins the scratch, the LDS
and the occupancy that DESIGN.md §5 states, from the compiler's remarks alone (the assembly is not searched)."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_cyclo")


# LDS bytes per workgroup = F (2 T + 68) 8 of staging (T = 32 offsets a tile, 16 at F = 64) and 16 F of border rows; the waves
# per SIMD that the registers leave, pinned as stated: a change either way is a change of DESIGN.md's table
STATED = {8: (8576, 5), 16: (17152, 2), 32: (34304, 2), 64: (52224, 1)}


def test_cyclo_kernels_do_not_spill(compiled):
    ks = kernels(compiled[0], r"cyclo_kernel<(\d+)>")
    assert sorted(ks, key=int) == ["8", "16", "32", "64"], sorted(ks)
    for F, (lds, occ) in STATED.items():
        k = ks[str(F)]
        print(F, k)
        assert k["scratch"] == 0, (F, k)
        T = 16 if F == 64 else 32
        assert k["lds"] == lds == F * (2 * T + 68) * 8 + 16 * F, (F, k)
        assert k["lds"] <= 64 * 1024
        assert k["occ"] == occ, (F, k)


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_measure\.hip crn_occmap\.hip crn_cyclo\.hip\b", mk, re.M)
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    # the unit sees crn_segments.h (handle_geometry, in_grids) and not crn_mask_runs.h: it never looks at a mask
    assert re.search(r"^\$\(O\)/crn_segments\.hip\.o.*\$\(O\)/crn_occmap\.hip\.o \$\(O\)/crn_cyclo\.hip\.o.*: \$\(HERE\)crn_segments\.h$", mk, re.M)
    assert not re.search(r"crn_cyclo\.hip\.o.*: \$\(HERE\)crn_mask_runs\.h$", mk, re.M)
    assert "crn_mask_runs.h" not in open(os.path.join(CSRC, "crn_cyclo.hip")).read()
