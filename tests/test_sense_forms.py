"""The list of compiled sensing-kernel forms and the rule that selects one (csrc/crn_forms.h / crn_forms.cpp), without a GPU.
tests/harness/forms_unit.cpp is built with g++ under AddressSanitizer + UBSan, as a stand-alone program, twice: as the shipped libraries
see the tables (float and wire-format units) and with -DCRN_AB_VARIANTS (the measurement library).  It walks the grid of
tests/golden/sense_forms.txt — 4 sizes x mode, window, periodic Hann, whole / short frames, CFAR, aligned bands, spectrum request x a
launch of a few epochs (no, yes, yes and refused by the device) x every variant the unit accepts x 3 x 3 band-plan classes — and
requires select_form to name the form the dispatch code before it launched (recorded there: 41 472 queries and 72 forms for float
samples, 41 472 and 48 for the wire format, 152 064 and 92 for the measurement unit), that form to be a row of the unit's table, every
row of every table to be reached, and the CLOSE= / PASS3_ROWS fields crn_sense_kernel_info prints from the selected form to be the
recorded ones for every handle state of the product's variants."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HARNESS = os.path.join(ROOT, "tests", "harness")
FIXTURE = os.path.join(ROOT, "tests", "golden", "sense_forms.txt")


def _run(name):
    exe = os.path.join(HARNESS, name)
    subprocess.check_call(["make", "-C", HARNESS, exe], stdout=subprocess.DEVNULL)
    out = subprocess.run([exe, FIXTURE], capture_output=True, text=True, timeout=300, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    print(out.stdout)
    assert out.returncode == 0 and "forms_unit: ok" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
    assert "ERROR" not in out.stderr and "runtime error" not in out.stderr, out.stderr[:3000]
    return out.stdout


def test_product_tables_and_selection_rule_match_the_record():
    out = _run("forms_unit")
    assert "float       41472 queries, 72 forms (all reached), 10368 without a form, 3456 handle states (0 where" in out
    assert "wire        41472 queries, 48 forms (all reached), 0 without a form" in out


def test_measurement_table_and_selection_rule_match_the_record():
    out = _run("forms_unit_ab")
    assert "measurement 152064 queries, 92 forms (all reached), 38016 without a form, 12672 handle states" in out
