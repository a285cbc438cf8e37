"""The track-linking kernels (csrc/crn_tracks.hip) keep everything in registers and a little LDS: no scratch.  Like
tests/test_segments_resources.py this test compiles the file itself, for gfx950, with the library's flags and
-Rpass-analysis=kernel-resource-usage, and pins the scratch and the LDS of every kernel in it; the same compilation's assembly shows
that the union hooks with one vector compare-and-swap, that the fp64 sums are native vector atomic adds (no compare-and-swap loop),
and that nothing but vector instructions writes memory."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels

# LDS bytes per workgroup: link holds two lists of 256 (lo, width) pairs, gather the 256 roots of its epoch, scan two words per wave
LDS = {"tracks_init_kernel": 0, "tracks_link_kernel": 4096, "tracks_gather_kernel": 1024, "tracks_count_kernel": 0,
       "tracks_scan_kernel": 128, "tracks_emit_kernel": 0, "tracks_labels_kernel": 0}


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_tracks")


def _kernels(txt):
    return kernels(txt, r"(tracks_\w+_kernel)")


def test_track_kernels_do_not_spill(compiled):
    ks = _kernels(compiled[0])
    assert sorted(ks) == sorted(LDS), sorted(ks)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < 1}
    assert not bad, bad
    assert {n: k["lds"] for n, k in ks.items()} == LDS


def test_memory_is_written_by_vector_instructions_only(compiled):
    asm = "\n".join(ln.split(";")[0] for ln in compiled[1].splitlines())
    ops = set(re.findall(r"^\s+([a-z][a-z0-9_]+)\s", asm, re.M))
    scalar_mem = {o for o in ops if o.startswith("s_") and any(w in o for w in ("store", "atomic", "dcache"))}
    assert not scalar_mem, scalar_mem
    assert not {o for o in ops if o.startswith("scratch_")}
    assert len(re.findall(r"global_atomic_cmpswap", asm)) == 1          # the hook of the union; every other atomic is a native one
    assert len(re.findall(r"global_atomic_add_f64", asm)) == 2          # power_sum and the centre's moment


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_segments\.hip crn_tracks\.hip\b", mk, re.M)
    # the host objects every flavour shares are derived from H_SRCS, and each flavour links them
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    for objs in ("OBJS", "OBJS_AB", "OBJS_SC", "OBJS_PL"):
        assert re.search(r"^%s\s*:=.*(\$\(REST\)|\$\(H_SRCS:%%=\$\(O\)/%%\.o\))" % objs, mk, re.M), objs
    assert re.search(r"^ASM_SRC \?= \$\(HERE\)crn_kernels\.hip$", mk, re.M)
