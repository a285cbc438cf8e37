"""The CA-CFAR kernels (kCfar instantiations of sense_kernel) keep everything in registers: no scratch, and at least the occupancy their
launch bound asks for.  Read from the compiler's resource remarks of `make -C cognitive-radio-network_amd/csrc asm` (the same parse as
tools/kernel_resources.py)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cognitive-radio-network_amd", "csrc")
K_CFAR = 2097152   # csrc/crn_frame.h


@pytest.fixture(scope="module")
def remarks():
    subprocess.run(["make", "-C", CSRC, "asm"], check=True, stdout=subprocess.DEVNULL)
    return open(os.path.join(CSRC, "build", "resource_usage.txt")).read()


def _kernels(txt):
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
        name = b.split('\n')[0].strip().split(' ')[0]
        if 'sense_kernel' not in name:
            continue

        def g(k):
            m = re.search(k + r": (\d+)", b)
            return int(m.group(1)) if m else None
        dem = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
        a = [x.strip() for x in re.search(r"Cfg<(.*?)> ?>", dem).group(1).split(',')]
        out[dem] = {"r3": int(a[0]), "win": a[5] == "true", "occ_bound": int(a[7]), "opt": int(a[-1]),
                    "scratch": g(r"ScratchSize \[bytes/lane\]"), "occ": g(r"Occupancy \[waves/SIMD\]")}
    return out


def test_cfar_kernels_do_not_spill(remarks):
    ks = {n: k for n, k in _kernels(remarks).items() if k["opt"] & K_CFAR}
    # plain and windowed forms (table window, periodic Hann folded into pass 1) at every size, plus the 4096-point whole-frame form
    assert {k["r3"] for k in ks.values()} == {2, 4, 8, 16}
    assert sum(1 for k in ks.values() if k["win"]) == 8 and sum(1 for k in ks.values() if not k["win"]) == 5, sorted(ks)
    bad = {n: k for n, k in ks.items() if k["scratch"] != 0 or k["occ"] is None or k["occ"] < k["occ_bound"]}
    assert not bad, bad
