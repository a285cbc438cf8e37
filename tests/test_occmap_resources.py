"""The occupancy-map kernels (csrc/crn_occmap.hip) keep everything in registers and, for the join, LDS: no scratch, and no atomic of any
kind (every word has one writer).  Like tests/test_channels_resources.py this test compiles the file itself, for gfx950, with the
library's flags and -Rpass-analysis=kernel-resource-usage, and pins the scratch, the LDS and the occupancy DESIGN.md §5 states."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_occmap")


def test_occmap_kernels_do_not_spill(compiled):
    ks = kernels(compiled[0], r"(occmap_\w+_kernel(?:<\w+>)?)")
    assert sorted(ks) == ["occmap_chunk_kernel<false>", "occmap_chunk_kernel<true>", "occmap_header_kernel", "occmap_join_kernel"], sorted(ks)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < 1}
    assert not bad, bad
    for n, k in ks.items():
        print(n, k)
    # chunk: 16 rows of 16 bytes and 16 mask words in flight per lane next to four bins' time words, holds and fp64 sums: registers only,
    # and few enough of them for four waves to a SIMD
    assert ks["occmap_chunk_kernel<true>"]["lds"] == 0 and ks["occmap_chunk_kernel<false>"]["lds"] == 0
    assert ks["occmap_chunk_kernel<true>"]["occ"] >= 4 and ks["occmap_chunk_kernel<false>"]["occ"] >= 4
    # join: per wave (8) and bin (64) a summary of 64 bytes; eight 32-byte summaries loaded ahead of the fold still leave four waves
    assert ks["occmap_join_kernel"]["lds"] == 8 * 64 * 64 and ks["occmap_join_kernel"]["occ"] >= 4
    assert ks["occmap_header_kernel"]["lds"] == 0


def test_no_atomics_and_vector_stores(compiled):
    body = compiled[1]
    atomics = re.findall(r"^\s*(\w*atomic\w*|ds_\w*(?:add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*)", body, re.M)
    assert not atomics, atomics
    # the rows come in and the summaries and records leave as 16-byte vector accesses
    assert len(re.findall(r"^\s*global_load_dwordx4", body, re.M)) >= 64
    assert len(re.findall(r"^\s*global_store_dwordx4", body, re.M)) >= 8 + 4 + 2
    assert "scratch_" not in body and "buffer_store" not in body


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_tcfar\.hip crn_measure\.hip crn_occmap\.hip\b", mk, re.M)
    # the host objects every flavour shares are derived from H_SRCS (tests/test_tracks_resources.py checks that each flavour links them)
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    # the unit sees crn_segments.h (handle_geometry, in_grids, CHUNK) and not crn_mask_runs.h: a lane owns four bins of a tile here
    assert re.search(r"^\$\(O\)/crn_segments\.hip\.o.*\$\(O\)/crn_measure\.hip\.o \$\(O\)/crn_occmap\.hip\.o.*: \$\(HERE\)crn_segments\.h$", mk, re.M)
    assert not re.search(r"crn_occmap\.hip\.o.*: \$\(HERE\)crn_mask_runs\.h$", mk, re.M)
    assert "crn_mask_runs.h" not in open(os.path.join(CSRC, "crn_occmap.hip")).read()
