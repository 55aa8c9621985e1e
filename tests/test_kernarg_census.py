"""How every step kernel fetches its arguments, from its compiled code (tools/kernarg_census.py;
host only: a device-only compile of the three kernel translation units, cached by source hash).

For every kernel a schedule can launch at NT = 1, 2, 4:
  * no scratch -- except the six kernels that had some in the parent commit (PARENT_SCRATCH,
    8 to 68 bytes, from profiles/args/census_parent.txt), which may keep at most what they had;
  * no VGPR count above the parent's recorded one by more than the allocation granule (8), and
    no kernel in a lower occupancy class (waves per SIMD) than in the parent's record;
  * no kernel that spilled no SGPRs into VGPR lanes in the parent's record spills any;
  * at most one serial scalar-load round trip before the first vector memory load, at most two
    in the decoding encoders (the arguments, then the rollout I/O record).

The record of this tree is profiles/args/census.txt (python tools/kernarg_census.py).
"""
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="needs hipcc")

VGPR_GRANULE = 8  # gfx950 allocates VGPRs in blocks of 8
# the parent commit's kernels with scratch (bytes): the only ones that may have any
PARENT_SCRATCH = {("kernels_nt2", "k_edge_hop<2, -1, true, 0>"): 28, ("kernels_nt2", "k_edge_hop<2, -1, true, 1>"): 8,
                  ("kernels_nt2", "k_edge_hop<2, 1, true, 0>"): 20, ("kernels_nt2", "k_edge_hop<2, 1, true, 1>"): 8,
                  ("kernels_nt4", "k_encode_coop<4, -1, true, 2, 4>"): 68,
                  ("kernels_nt4", "k_encode_coop<4, 1, true, 2, 4>"): 28}


def waves_per_simd(vgprs):
    """Occupancy class of a kernel on gfx950: 512 VGPRs per SIMD lane, blocks of 8, at most 8 waves."""
    return min(8, 512 // (-(-vgprs // VGPR_GRANULE) * VGPR_GRANULE))


@pytest.fixture(scope="module")
def rows():
    import kernarg_census as kc
    r = kc.census()
    print("\n" + kc.format_rows(r))
    return r


@pytest.fixture(scope="module")
def parent():
    import kernarg_census as kc
    return kc.parse_table(os.path.join(ROOT, "profiles", "args", "census_parent.txt"))


def test_every_family_and_width_is_there(rows):
    import kernarg_census as kc
    seen = {(unit, fam) for unit, _, fam, _ in rows}
    for fam in kc.FAMILIES:
        units = {"k_edge_coop": ["kernels_nt2"], "k_edge_coop4": ["kernels_nt4"], "k_hop_coop": ["kernels_nt2", "kernels_nt4"],
                 "k_hop_split": ["kernels_nt2", "kernels_nt4"], "k_encode_coop": ["kernels_nt2", "kernels_nt4"]}.get(
                     fam, ["kernels_nt1", "kernels_nt2", "kernels_nt4"])
        for u in units:
            assert (u, fam) in seen, f"{fam} has no kernel in {u}"


def test_no_kernel_gains_scratch(rows, parent):
    assert {k: parent[k]["scratch"] for k in parent if parent[k]["scratch"]} == PARENT_SCRATCH
    bad = []
    for unit, k, _, r in rows:
        had = PARENT_SCRATCH.get((unit, k), 0)
        print(f"{unit} {k}: scratch {r['scratch']} (allowed {had})")
        if r["scratch"] > had:
            bad.append((unit, k, r["scratch"], had))
    assert not bad, f"kernels with scratch (unit, kernel, bytes, allowed): {bad}"


def test_vgprs_within_a_granule_of_the_parent(rows, parent):
    bad = []
    for unit, k, _, r in rows:
        assert (unit, k) in parent, f"{unit} {k}: not in the parent's record"
        was = parent[(unit, k)]["vgpr"]
        print(f"{unit} {k}: vgpr {r['vgpr']} (parent {was})")
        if r["vgpr"] > was + VGPR_GRANULE:
            bad.append((unit, k, r["vgpr"], was))
    assert not bad, f"kernels above the parent's VGPRs by more than {VGPR_GRANULE}: {bad}"


def test_no_kernel_drops_an_occupancy_class(rows, parent):
    bad = []
    for unit, k, _, r in rows:
        was, now = waves_per_simd(parent[(unit, k)]["vgpr"]), waves_per_simd(r["vgpr"])
        print(f"{unit} {k}: {now} waves per SIMD at {r['vgpr']} VGPRs (parent {was} at {parent[(unit, k)]['vgpr']})")
        if now < was:
            bad.append((unit, k, r["vgpr"], now, parent[(unit, k)]["vgpr"], was))
    assert not bad, f"kernels in a lower occupancy class (unit, kernel, VGPRs, waves, parent's VGPRs, waves): {bad}"


def test_no_kernel_starts_to_spill_sgprs(rows, parent):
    bad = []
    for unit, k, _, r in rows:
        was = parent[(unit, k)]["sgpr_spill"]
        print(f"{unit} {k}: {r['sgpr_spill']} SGPR spills (parent {was})")
        if was == 0 and r["sgpr_spill"] > 0:
            bad.append((unit, k, r["sgpr_spill"]))
    assert not bad, f"kernels that spill SGPRs into VGPR lanes and did not in the parent: {bad}"


def test_one_round_trip_before_the_first_vector_load(rows):
    bad = []
    for unit, k, fam, r in rows:
        decoding = fam in ("k_encode", "k_encode_coop") and k.split(",")[2].strip().startswith("true")  # DEC
        bound = 0 if r["preload"] > 0 else 2 if decoding else 1
        print(f"{unit} {k}: {r['trips']} round trips (bound {bound}), {r['after']} scalar loads after the first vector load")
        if r["trips"] > bound:
            bad.append((unit, k, r["trips"], bound))
    assert not bad, f"{len(bad)} kernels above the bound (unit, kernel, round trips, bound): {bad}"
