"""What the tests/test_*_resources.py files share: one csrc/ translation unit compiled for gfx950 with the library's flags and
-Rpass-analysis=kernel-resource-usage, and the parse of the compiler's resource remarks."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cognitive-radio-network_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def compile_unit(tmp_path_factory, unit):
    """csrc/<unit>.hip, device side only.  Returns (the compiler's remarks, the assembly)."""
    out = tmp_path_factory.mktemp(unit) / (unit + ".s")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS\s*:=\s*(.*?)\n(?=#)", mk, re.S | re.M).group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    r = subprocess.run([HIPCC, *flags, "--cuda-device-only", "-Wno-unused-command-line-argument", "-Rpass-analysis=kernel-resource-usage",
                        "-S", "-o", str(out), os.path.join(CSRC, unit + ".hip")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stderr, open(out).read()


def kernels(txt, short=None):
    """{kernel: scratch, occupancy, VGPRs, LDS} from the remarks, keyed by the demangled name or, where the regex `short` matches it, by
    its first group."""
    out = {}
    for b in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
        name = b.split('\n')[0].strip().split(' ')[0]

        def g(k):
            m = re.search(k + r": (\d+)", b)
            return int(m.group(1)) if m else None
        dem = subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip()
        m = re.search(short, dem) if short else None
        out[m.group(1) if m else dem] = {"scratch": g(r"ScratchSize \[bytes/lane\]"), "occ": g(r"Occupancy \[waves/SIMD\]"), "vgprs": g(r" VGPRs"),
                                         "lds": g(r"LDS Size \[bytes/block\]")}
    return out
