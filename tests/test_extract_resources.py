"""The extraction kernels (csrc/crn_extract.hip) hold a transform's 16 values per lane, the lane's taper and its twiddle factors in
registers and exchange one 64 x 16 block of complex words per wave through LDS.  Like tests/test_hops_resources.py this test compiles
the file itself, for gfx950, with the library's flags and -Rpass-analysis=kernel-resource-usage, and pins the scratch, the LDS and the
occupancy DESIGN.md §5 states, from the compiler's remarks alone."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_extract")


def test_extract_kernels_do_not_spill(compiled):
    ks = kernels(compiled[0], r"extract_kernel<(\d+)>")
    assert sorted(ks, key=int) == ["16", "32", "64", "128", "256"], sorted(ks)
    for n, k in ks.items():
        print(n, k)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < 1}
    assert not bad, bad
    # M = 16: a lane holds the whole transform, no second pass and no LDS; seven waves to a SIMD
    assert ks["16"]["lds"] == 0 and ks["16"]["occ"] >= 7
    # M >= 32: 16 rows of 65 complex words, 8320 bytes to a wave; the taper (16) and the twiddle factors (32) stay in registers next to the
    # 32 of the transform: three waves to a SIMD
    for m in ("32", "64", "128", "256"):
        assert ks[m]["lds"] == 16 * 65 * 8 and ks[m]["occ"] >= 3 and ks[m]["vgprs"] <= 160, (m, ks[m])


def test_no_atomics_and_plain_vector_stores(compiled):
    asm = compiled[1]
    assert "extract_kernel" in asm
    assert not re.search(r"\b(global|flat|ds|buffer)_atomic|\bds_(add|min|max|cmpst)", asm)
    assert "global_store_dwordx4" in asm and "global_load_dwordx2" in asm


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_cyclo\.hip crn_hops\.hip crn_extract\.hip\b", mk, re.M)
    # the host objects every flavour shares are derived from H_SRCS (tests/test_tracks_resources.py checks that each flavour links them)
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    # the unit sees crn_segments.h (handle_geometry, in_grids) and not crn_mask_runs.h: it reads spectra, not the bin mask
    assert re.search(r"^\$\(O\)/crn_segments\.hip\.o.*\$\(O\)/crn_hops\.hip\.o \$\(O\)/crn_extract\.hip\.o.*: \$\(HERE\)crn_segments\.h$", mk, re.M)
    src = open(os.path.join(CSRC, "crn_extract.hip")).read()
    assert "crn_mask_runs.h" not in src and "atomic" not in re.sub(r"//.*", "", src)
