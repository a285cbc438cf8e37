"""The kernel of the segment measurement (csrc/crn_measure.hip): a wave holds a segment's running figures in registers and the epoch's row
in LDS: no scratch, and no atomic of any kind (every slot has one writer).  Like tests/test_tcfar_resources.py this test compiles the file
itself, for gfx950, with the library's flags and -Rpass-analysis=kernel-resource-usage, and pins the scratch and the LDS."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_measure")


def test_measure_kernel_does_not_spill(compiled):
    ks = kernels(compiled[0], r"(measure_\w*kernel)")
    # one instantiation serves every fft_len
    assert sorted(ks) == ["measure_kernel"], sorted(ks)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < 1}
    assert not bad, bad
    # the row of the largest fft_len, unpadded: lane l reads offset c 64 + l
    assert ks["measure_kernel"]["lds"] == 4096 * 4
    # four waves to a workgroup and a row each: the LDS of a compute unit (160 KB) holds ten rows, so the registers decide, and they leave
    # at least four waves to a SIMD
    assert ks["measure_kernel"]["occ"] >= 4
    for n, k in ks.items():
        print(n, k)


def test_no_atomics(compiled):
    body = compiled[1]
    atomics = re.findall(r"^\s*(\w*atomic\w*|ds_\w*(?:add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*)", body, re.M)
    assert not atomics, atomics
    # the records leave as plain 16-byte vector stores
    assert re.findall(r"^\s*(global_store_dwordx4|flat_store_dwordx4)", body, re.M)
    assert "scratch_" not in body and "buffer_store" not in body


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_lad\.hip crn_tcfar\.hip crn_measure\.hip\b", mk, re.M)
    # the host objects every flavour shares are derived from H_SRCS (tests/test_tracks_resources.py checks that each flavour links them)
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    # the unit sees crn_segments.h (handle_geometry, in_grids, MAX_N) and not crn_mask_runs.h: it never looks at a mask
    assert re.search(r"^\$\(O\)/crn_segments\.hip\.o.*\$\(O\)/crn_tcfar\.hip\.o \$\(O\)/crn_measure\.hip\.o.*: \$\(HERE\)crn_segments\.h$", mk, re.M)
    assert not re.search(r"crn_measure\.hip\.o.*: \$\(HERE\)crn_mask_runs\.h$", mk, re.M)
    assert "crn_mask_runs.h" not in open(os.path.join(CSRC, "crn_measure.hip")).read()
