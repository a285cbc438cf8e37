"""The channel-statistics kernels (csrc/crn_channels.hip) keep everything in registers and LDS: no scratch.  Like
tests/test_segments_resources.py this test compiles the file itself, for gfx950, with the library's flags and
-Rpass-analysis=kernel-resource-usage, and pins the scratch and the LDS of every kernel in it: the four epoch kernels (one instantiation
per fft_len) and the two kernels of the time stage (chunk summaries, and their join into the records)."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_channels")


def test_channel_kernels_do_not_spill(compiled):
    ks = kernels(compiled[0], r"(channels_\w+_kernel(?:<\d+>)?)")
    assert sorted(ks) == ["channels_epoch_kernel<%d>" % b for b in (16, 32, 64, 8)] + ["channels_join_kernel", "channels_time_kernel"], sorted(ks)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < 1}
    assert not bad, bad
    # epoch: the row in LDS padded by 4 floats per lane piece (4 N + 1 KiB, as the segment kernels), one fp64 sum and one 64-bit mask
    # piece per lane (1 KiB)
    assert {b: ks["channels_epoch_kernel<%d>" % b]["lds"] for b in (8, 16, 32, 64)} == {b: 4 * 64 * b + 1024 + 1024 for b in (8, 16, 32, 64)}
    # time: a wave's ballots and registers, no LDS
    assert ks["channels_time_kernel"]["lds"] == 0
    # join: 16 histogram bins x 64 channels (4 KiB); per wave (8) and channel (64) a summary of 15 ints and two fp64 sums (76 bytes)
    assert ks["channels_join_kernel"]["lds"] == 16 * 64 * 4 + 8 * 64 * (15 * 4 + 2 * 8)


def test_the_file_is_in_every_library_flavour():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^H_SRCS\s*:=.*\bcrn_channels\.hip\b", mk, re.M)
    # the host objects every flavour shares are derived from H_SRCS (tests/test_tracks_resources.py checks that each flavour links them);
    # `make asm` still lists the sensing kernels only
    assert re.search(r"^REST\s*:=.*\$\(O\)/%\.o.*\$\(H_SRCS\)", mk, re.M)
    assert re.search(r"^ASM_SRC \?= \$\(HERE\)crn_kernels\.hip$", mk, re.M)
