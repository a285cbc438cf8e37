"""libcrnliquidfft in front of "liquid" in the link order INTEGRATION.md §6 prescribes (VERDICT r01 weak #9,
ADVICE r01 medium): the shim must take only the sensing path's plans (forward, N in {512..4096}) and hand
every other plan — liquid's own internal OFDM framing plans included (reference:
src/extensible_cognitive_radio.cpp:113,123: backward, N = subcarriers) — to the library behind it, instead of
exiting.  tests/harness/libstub_liquid.so stands in for liquid (own plan struct, O(n^2) DFT, and a function
that creates a backward plan through the public symbol the way ofdmflexframegen_create does)."""
import os
import subprocess

import pytest

HARNESS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "harness")
EXE = os.path.join(HARNESS, "liquid_shim_check")


def _run(*args):
    if not os.path.exists(EXE):   # like tests/test_host_logic.py: the `built` fixture looks at the library and the oracle only
        subprocess.check_call(["make", "-C", HARNESS, EXE], stdout=subprocess.DEVNULL)
    out = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    return {ln.split()[0]: ln.split()[1:] for ln in out.stdout.splitlines()}


def test_unsupported_plans_go_to_the_next_library(built):
    """No GPU needed: a 64-point BACKWARD plan made inside "liquid" and one made by the application both
    bind to the shim first (it precedes liquid on the link line) and both end up in the stub."""
    r = _run()
    assert float(r["internal_backward_err"][0]) < 1e-5 and float(r["public_backward_err"][0]) < 1e-5
    assert r["next_library_plans"] == ["created", "2", "executed", "2", "destroyed", "2"]
    assert r["forwarded_by_shim"] == ["2"]      # both creations passed through the shim's symbol


@pytest.mark.gpu
def test_sensing_plan_runs_on_the_gpu_beside_liquids_own(built):
    r = _run("gpu")
    assert float(r["gpu_forward_rel_err"][0]) < 1e-5
    assert r["next_library_plans"] == ["created", "2", "executed", "2", "destroyed", "2"]   # the 512-pt plan never reached the stub
    assert r["forwarded_by_shim"] == ["2"]
