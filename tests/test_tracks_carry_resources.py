"""The kernels that carry tracks across batches (csrc/crn_tracks_carry.hip) keep everything in registers and a little LDS: no scratch.
Like tests/test_tracks_resources.py this test compiles the file itself, for gfx950, with the library's flags and
-Rpass-analysis=kernel-resource-usage, and pins the scratch, the occupancy and the LDS of every kernel in it, and the file's place in
the Makefile.  Resource remarks only."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels

# LDS bytes per workgroup: link holds two lists of 256 (lo, width) pairs, gather the 256 roots of its row, scan four words per wave
LDS = {"carry_init_kernel": 0, "carry_link_kernel": 4096, "carry_gather_kernel": 1024, "carry_count_kernel": 0,
       "carry_scan_kernel": 256, "carry_emit_kernel": 0, "carry_tail_kernel": 0}


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_tracks_carry")[0]


def _kernels(txt):
    return kernels(txt, r"(carry_\w+_kernel)")


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
