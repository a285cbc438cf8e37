"""The segment-extraction kernels (csrc/crn_segments.hip, one instantiation per fft_len) keep everything in registers and LDS: no
scratch.  `make asm` writes the resource remarks of the sensing kernels only, so this test compiles the new file itself, for gfx950,
with the library's flags and -Rpass-analysis=kernel-resource-usage (the same parse as tests/test_cfar_resources.py)."""
import os
import re

import pytest

from hip_resources import CSRC, compile_unit, kernels as _kernels


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    return compile_unit(tmp_path_factory, "crn_segments")[0]


def test_segment_kernels_do_not_spill(remarks):
    ks = {n: k for n, k in _kernels(remarks).items() if "segments_kernel" in n}
    # one instantiation per fft_len: 8, 16, 32 and 64 bins per lane
    assert sorted(int(re.search(r"segments_kernel<(\d+)>", n).group(1)) for n in ks) == [8, 16, 32, 64], sorted(ks)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < 1}
    assert not bad, bad
    # the row in LDS, padded by 4 floats per lane piece: 4 N + 1 KiB per epoch
    assert sorted(k["lds"] for k in ks.values()) == [4 * n + 1024 for n in (512, 1024, 2048, 4096)]


def test_make_asm_still_lists_the_sensing_kernels_only():
    """What `make asm` writes for tests/test_cfar_resources.py does not change: the new file is not part of that listing."""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^ASM_SRC \?= \$\(HERE\)crn_kernels\.hip$", mk, re.M)
