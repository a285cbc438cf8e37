"""The kernels of the CFAR along time (csrc/crn_tcfar.hip): the tile kernel keeps four test values and four counts per lane in registers
and the staged rows in LDS: no scratch.  Like tests/test_lad_resources.py this test compiles the file itself, for gfx950, with the
library's flags and -Rpass-analysis=kernel-resource-usage, and pins the scratch and the LDS of every kernel in it."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_tcfar")


def test_tcfar_kernels_do_not_spill(compiled):
    ks = kernels(compiled[0], r"(tcfar_\w*kernel)")
    assert sorted(ks) == ["tcfar_hist_kernel", "tcfar_kernel", "tcfar_open_kernel"], sorted(ks)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < 1}
    assert not bad, bad
    # one instantiation serves every fft_len; a tile is 256 staged rows of 64 bins, the most a workgroup may declare
    assert {n: k["lds"] for n, k in ks.items()} == {"tcfar_kernel": 256 * 64 * 4, "tcfar_open_kernel": 0, "tcfar_hist_kernel": 0}
    # two tiles to a compute unit (160 KB of LDS), four waves each
    assert ks["tcfar_kernel"]["occ"] >= 2
    for n, k in ks.items():
        print(n, k)


def test_the_header_counts_are_the_only_atomics(compiled):
    """A header sums the bits of fft_len / 64 workgroups: one 64-bit integer add per (epoch, strip), nothing else."""
    body = compiled[1]
    atomics = re.findall(r"^\s*(global_atomic_\w+|flat_atomic_\w+|buffer_atomic_\w+|ds_\w*(?:add|cmpst|wrxchg)\w*)", body, re.M)
    assert atomics and set(atomics) == {"global_atomic_add_x2"}, atomics
    assert len(atomics) == 1, atomics


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_holes\.hip crn_lad\.hip crn_tcfar\.hip\b", mk, re.M)
    # the host objects every flavour shares are derived from H_SRCS (tests/test_tracks_resources.py checks that each flavour links them)
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    # the unit sees crn_segments.h (handle_geometry, in_grids) and not crn_mask_runs.h: it is on the first header's dependency line, behind
    # the excised-floor detector
    assert re.search(r"^\$\(O\)/crn_segments\.hip\.o.*\$\(O\)/crn_lad\.hip\.o \$\(O\)/crn_tcfar\.hip\.o.*: \$\(HERE\)crn_segments\.h$", mk, re.M)
    assert not re.search(r"crn_tcfar\.hip\.o.*: \$\(HERE\)crn_mask_runs\.h$", mk, re.M)
    assert "crn_mask_runs.h" not in open(os.path.join(CSRC, "crn_tcfar.hip")).read()
