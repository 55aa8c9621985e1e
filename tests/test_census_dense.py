"""The dense row-tile hop's compiled code (tools/kernarg_census.py; host only: a device-only
compile of the kernel translation units, cached by source hash and shared with
tests/test_kernarg_census.py): k_hop_dense at NT = 1, 2, the middle hop and the last hop with
the compile-time PReLU and the run-time activation,
  * has no scratch and spills no SGPRs into VGPR lanes;
  * makes one serial scalar-load round trip before its first vector memory load.
The record goes to profiles/densehop/census.txt.
"""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")

FAMILIES = ("k_hop_dense",)
EXPECTED = {(f"kernels_nt{nt}", f"k_hop_dense<{nt}, {act}, {last}>")
            for nt in (1, 2) for act, last in ((1, "false"), (1, "true"), (-1, "true"))}


@pytest.fixture(scope="module")
def rows():
    import kernarg_census as kc
    r = [x for x in kc.census(all_kernels=True) if x[2] in FAMILIES]
    table = kc.format_rows(r)
    print("\n" + table)
    try:  # the record (a read-only checkout keeps the committed one)
        out = os.path.join(ROOT, "profiles", "densehop")
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "census.txt"), "w") as f:
            f.write(table + "\n")
    except OSError:
        pass
    return r


def test_every_instantiation_is_there(rows):
    assert {(unit, k) for unit, k, _, _ in rows} == EXPECTED


def test_no_scratch_no_spills(rows):
    bad = [(unit, k, r["scratch"], r["sgpr_spill"], r["vgpr_spill"]) for unit, k, _, r in rows
           if r["scratch"] or r["sgpr_spill"] or r["vgpr_spill"]]
    assert not bad, f"(unit, kernel, scratch bytes, SGPR spills, VGPR spills): {bad}"


def test_one_round_trip_before_the_first_vector_load(rows):
    bad = [(unit, k, r["trips"]) for unit, k, _, r in rows if r["trips"] > 1]
    assert not bad, f"(unit, kernel, round trips): {bad}"

