"""Flood maps and chunked rollouts without a GPU: the torch restatement ``_maps_torch`` against the
reference's own functions (tests/golden/fx_floodmaps.npz, tools/gen_golden_floodmaps.py, and the
reference tree itself where present), ``rollout_chunks`` on the torch path against the whole
rollout bit for bit, and the host side of the C ABI (error returns, no-ops, the launch query).
Then the kernel's test cases themselves (tests/floodmaps_cases.py): a census of the staging
geometries the launch query reports against the windows the GPU sweep runs, the part-by-part
restatement against ``_maps_torch``, and every wrong variant of it caught in every class.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

import floodmaps_cases as fc
from conftest import ROOT, build_msgnn, golden, weights
from mswegnn import _lib
from mswegnn import floodmaps as fmod
from mswegnn.batch import collate
from mswegnn.floodmaps import FloodMaps, flood_maps, rollout_chunks, rollout_flood_maps
from mswegnn.mesh import make_multiscale_mesh, mesh_config, wet_state
from mswegnn.metrics import finest_ranges
from mswegnn.rollout import adapt_batch_training

REF = "/root/reference"
FX = golden("fx_floodmaps")
ROLLOUTS = [str(n) for n in FX["rollouts"]]


def _rollout(name):
    return torch.from_numpy(golden(name)["rollout"])


@pytest.mark.parametrize("name", ROLLOUTS)
def test_maps_torch_equals_reference_fixture(name):
    thr = (0.0, 0.05, 0.3)
    assert np.array_equal(FX["thresholds"], np.array(thr, np.float32))
    m = fmod._maps_torch(_rollout(name), thr)
    for k in ("h_max", "t_h_max", "q_max", "t_q_max", "vel_max", "froude_max"):
        assert torch.equal(m[k], torch.from_numpy(FX[f"{name}/{k}"])), k
    for i, t in enumerate(thr):
        for k in ("wet_steps", "first_wet", "last_wet"):
            assert torch.equal(m[k][i], torch.from_numpy(FX[f"{name}/{k}_{t}"])), (k, t)
    # the public result, with the reference's WD_to_FAT expression
    tres = torch.from_numpy(FX["temporal_res"])
    for ts in (int(v) for v in FX["time_starts"]):
        res = flood_maps(_rollout(name), thresholds=thr, temporal_res=tres, time_start=ts)
        for t in thr:
            assert torch.equal(res["fat_hours"][t], torch.from_numpy(FX[f"{name}/fat_{t}_{ts}"])), (t, ts)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "utils")), reason="reference checkout not present (GPU box)")
@pytest.mark.parametrize("name", ROLLOUTS)
def test_maps_torch_equals_reference_functions(name):
    added = [os.path.join(ROOT, "oracle", "refstubs"), REF]
    sys.path[:0] = added
    dont = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        from utils.miscellaneous import WD_to_FAT, get_Froude, get_velocity
    finally:
        sys.dont_write_bytecode = dont
        for p in added:
            sys.path.remove(p)
    r = _rollout(name)
    h, q = r[:, 0, :], r[:, 1, :].abs()
    thr = (0.0, 0.05, 0.3)
    m = fmod._maps_torch(r, thr)
    vel = get_velocity(q.clone(), h.clone())
    assert torch.equal(m["vel_max"], vel.max(1).values)
    assert torch.equal(m["froude_max"], get_Froude(vel.clone(), h.clone()).max(1).values)
    res = flood_maps(r, thresholds=thr, temporal_res=30, time_start=2)
    for t in thr:
        assert torch.equal(res["fat_hours"][t], WD_to_FAT(h.clone(), 30, t, 2))


@pytest.mark.parametrize("name", ROLLOUTS[:2])
def test_arrival_equals_fat_only_where_cells_stay_wet(name):
    r = _rollout(name)
    T = r.shape[-1]
    res = flood_maps(r, thresholds=(0.05,), temporal_res=30)
    wet, first, last = (res[k][0.05] for k in ("wet_steps", "first_wet", "last_wet"))
    ever = first >= 0
    stays = ever & (wet == T - first)          # wet at every step from the first on
    redries = ever & ~stays
    assert stays.any() and redries.any()
    arr, fat = res["arrival_hours"][0.05], res["fat_hours"][0.05]
    assert torch.equal(arr[stays], fat[stays])
    assert bool((arr[redries] != fat[redries]).all())
    assert bool(torch.isnan(arr[~ever]).all())
    assert bool((last[stays] == T - 1).all())


def test_cpu_carry_over_equals_one_shot():
    r = _rollout(ROLLOUTS[0])
    whole = FloodMaps(r.shape[0] - 7, 7).update(r).maps
    for split in ((16, 16, 16), (5, 43), (47, 1), (1,) * 48):
        fm = FloodMaps(r.shape[0] - 7, 7)
        t0 = 0
        for n in split:
            fm.update(r[:, :, t0:t0 + n])
            t0 += n
        assert fm.steps_seen == 48
        for k, v in whole.items():
            assert torch.equal(fm.maps[k], v), (split, k)


@pytest.fixture(scope="module")
def tiny_model():
    return build_msgnn(num_scales=4, hid=32, K=4, state=weights("K4_F32"))


@pytest.fixture(scope="module")
def tiny_graphs():
    dry = make_multiscale_mesh(**mesh_config("tiny"), T=9)
    return {"dry": dry, "wet": wet_state(dry, seed=1)}


@pytest.fixture(scope="module")
def tiny_whole(tiny_model, tiny_graphs):
    return {k: tiny_model.rollout(g, 9) for k, g in tiny_graphs.items()}


@pytest.mark.parametrize("start", ["dry", "wet"])
@pytest.mark.parametrize("chunk", [1, 2, 3, 4, 9])
def test_rollout_chunks_equal_whole_rollout(tiny_model, tiny_graphs, tiny_whole, start, chunk):
    assert tiny_model.previous_t == 3
    g = tiny_graphs[start]
    x0 = g.x.clone()
    pieces = list(rollout_chunks(tiny_model, g, 9, chunk))
    assert [t0 for t0, _ in pieces] == list(range(0, 9, chunk))
    assert torch.equal(torch.cat([p for _, p in pieces], -1), tiny_whole[start])
    assert torch.equal(g.x, x0)


@pytest.mark.parametrize("chunk", [2, 4])
def test_rollout_chunks_on_a_batch(tiny_model, tiny_graphs, chunk):
    other = wet_state(make_multiscale_mesh(n_coarse=3, num_scales=4, seed=5, T=9), seed=2)
    b = adapt_batch_training(collate([tiny_graphs["wet"], other]))
    whole = tiny_model.rollout(b, 9)
    assert torch.equal(torch.cat([p for _, p in rollout_chunks(tiny_model, b, 9, chunk)], -1), whole)
    # one result per simulation, finest scale, equal to the mesh run alone
    per_sim = rollout_flood_maps(tiny_model, b, 9, chunk=chunk, ranges=finest_ranges(b))
    for g, res in zip((tiny_graphs["wet"], other), per_sim):
        alone = flood_maps(tiny_model.rollout(g, 9), ranges=finest_ranges(g))[0]
        for k in ("h_max", "t_h_max", "froude_max"):
            assert torch.equal(res[k], alone[k]), k
        assert torch.equal(res["wet_steps"][0.05], alone["wet_steps"][0.05])


def test_rollout_flood_maps_chunked_equals_whole(tiny_model, tiny_graphs, tiny_whole):
    g = tiny_graphs["wet"]
    a, ra = rollout_flood_maps(tiny_model, g, 9, chunk=None, keep_rollout=True, temporal_res=30)
    b, rb = rollout_flood_maps(tiny_model, g, 9, chunk=4, keep_rollout=True, temporal_res=30)
    assert torch.equal(ra, tiny_whole["wet"]) and torch.equal(rb, ra)
    assert a.keys() == b.keys() and a["steps"] == b["steps"] == 9

    def same(u, v):
        if isinstance(u, dict):
            return u.keys() == v.keys() and all(same(u[k], v[k]) for k in u)
        if torch.is_floating_point(u):  # arrival_hours holds NaN where a cell was never wet
            u, v = torch.nan_to_num(u, nan=-7.0), torch.nan_to_num(v, nan=-7.0)
        return torch.equal(u, v)
    for k in a:
        if k != "steps":
            assert same(a[k], b[k]), k


# ------------------------------------------------------------------ C ABI, host side only
@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def _update(lib, pred=1, T=8, t_begin=0, t_count=8, nrows=4, thr=True, n_thr=2, maps=True, row0=0):
    """msw_flood_maps_update with dummy non-NULL addresses: every call here must return before
    anything is launched or dereferenced."""
    m = _lib.MswFloodMaps()
    th = (C.c_float * 4)(0.05, 0.3, 0, 0)
    return lib.msw_flood_maps_update(C.c_void_p(4096 if pred else 0), T, t_begin, t_count, 0, row0, nrows,
                                     th if thr else None, n_thr, 0.01, 1, C.byref(m) if maps else None, None)


@pytest.mark.parametrize("kw, text", [
    (dict(pred=0), "null"), (dict(maps=False), "null"), (dict(thr=False), "null"),
    (dict(n_thr=5), "n_thr"), (dict(n_thr=-1), "n_thr"),
    (dict(t_begin=-1), "window"), (dict(t_begin=4, t_count=5), "window"), (dict(t_count=-1), "window"),
    (dict(T=-1, t_count=0), "window"), (dict(nrows=-1), "nrows"), (dict(row0=-1), "row0"),
])
def test_abi_update_rejects_bad_arguments(lib, kw, text):
    assert _update(lib, **kw) == -1  # MSW_ERR_INVALID
    assert text in lib.msw_last_error().decode()


@pytest.mark.parametrize("kw", [dict(t_count=0), dict(nrows=0), dict(thr=False, n_thr=0, nrows=0)])
def test_abi_update_no_ops(lib, kw):
    assert _update(lib, **kw) == _lib.MSW_OK


@pytest.mark.parametrize("t_count", [1, 4, 31, 32, 48, 100, 1024, 5000])
@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 1499, 10369, 300001, 1 << 20, 1 << 33])
def test_abi_launch_is_consistent(lib, nrows, t_count):
    g, r, it = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.msw_flood_maps_launch(nrows, t_count, C.byref(g), C.byref(r), C.byref(it)) == _lib.MSW_OK
    g, r, it = g.value, r.value, it.value
    assert g >= 1 and it >= 1 and 1 <= r <= 64 and r & (r - 1) == 0
    assert g * r * it >= nrows
    assert g * r * (it - 1) < nrows, "iters is not minimal"
    assert g <= -(-nrows // r), "more workgroups than rounds"


def test_abi_launch_edge_cases(lib):
    g, r, it = C.c_int32(7), C.c_int32(7), C.c_int32(7)
    assert lib.msw_flood_maps_launch(0, 8, C.byref(g), C.byref(r), C.byref(it)) == _lib.MSW_OK
    assert (g.value, it.value) == (0, 0)
    assert lib.msw_flood_maps_launch(8, 0, C.byref(g), C.byref(r), C.byref(it)) == _lib.MSW_OK
    assert (g.value, it.value) == (0, 0)
    assert lib.msw_flood_maps_launch(-1, 8, C.byref(g), C.byref(r), C.byref(it)) == -1
    assert lib.msw_flood_maps_launch(8, 8, None, C.byref(r), C.byref(it)) == -1


# ------------------------------------------------------------------ the kernel's test cases
def test_census_of_staging_geometries(lib):
    """Every rows-per-round class of the launch query runs with both loaders, and both sides of
    every class edge are windows of the sweep: retuning the kernel's LDS budget without extending
    tests/floodmaps_cases.py fails here."""
    r = {tc: fc.rows_per_wg(tc) for tc in range(1, fc.SLAB + 1)}
    classes = sorted(set(r.values()))
    edges = [tc for tc in range(2, fc.SLAB + 1) if r[tc] != r[tc - 1]]      # the first t_count of a class
    assert len(classes) >= 2 and len(edges) == len(classes) - 1
    assert fc.rows_per_wg(fc.SLAB + 1) == r[fc.SLAB] and fc.rows_per_wg(5 * fc.SLAB) == r[fc.SLAB]
    ran = {(tc, vec) for c in fc.CASES for tc, _, vec in c.launches()}
    steps = {tc for tc, _ in ran}
    for e in edges:
        assert e - 1 in steps and e in steps, f"no window on both sides of the class edge {e - 1} | {e}"
    for R in classes:
        for vec in (False, True):
            assert any(r[tc] == R and v == vec for tc, v in ran), f"rows_per_wg {R} never runs with vec={vec}"
    # the loaders are what the cases say: the 16-byte one needs the whole window of an even T
    assert all(c.vec == (c.T in fc.VEC_T and c.t_begin == 0 and c.t_count == c.T and not c.shift) for c in fc.CASES)
    # the carry-over cases are one class each of 4, 2 and 1 rows per round
    assert {fc.rows_per_wg(min(T, fc.SLAB)) for T, _ in fc.CARRY} == {4, 2, 1}
    assert all(sum(pieces) == T for T, pieces in fc.CARRY)


def test_planted_rows_sit_where_the_geometry_says():
    assert fc.part_starts(132) == list(range(0, 132, 9)) and len(fc.part_starts(132)) == 15   # the 16th part is empty
    assert fc.part_starts(200) == list(range(0, 200, 13))
    assert fc.part_starts(1025) == list(range(0, 1024, 16)) + [1024]
    r = fc.planted_rollout(fc.PERIOD, 132, 0, 132, seed=1)
    h = r[:, 0, :]
    assert int(h[8 + 7].argmax()) == 131 and float(h[8 + 7].max()) == 3.0
    assert h[8 + 2, 125] == h[8 + 2, 126] == 3.0                 # across the last non-empty boundary
    assert bool((h[8 + 6, 63:72] == 0).all()) and float(h[8 + 6, 62]) > 0 and float(h[8 + 6, 72]) > 0
    r = fc.planted_rollout(fc.PERIOD, 2049, 0, 2049, seed=1)
    assert r[8 + 8, 0, 1023] == r[8 + 8, 0, 1024] == 3.0 and r[8 + 10, 0, 2047] == r[8 + 10, 0, 2048] == 3.0
    assert bool((r[8 + 9, 0, :1024] == 0).all()) and float(r[8 + 9, 0, 1024]) > 0.05


@pytest.mark.parametrize("case", fc.CASES, ids=[c.id for c in fc.CASES])
def test_restatement_and_sensitivity(case):
    """On the planted rows of the case: the part-by-part restatement equals ``_maps_torch``, and
    every wrong variant of it changes a map that the GPU sweep asserts."""
    host = fc.case_rollout(case, fc.PERIOD)
    rows = host[8:, :, case.t_begin:case.t_begin + case.t_count]
    want = fc.yardstick(rows)
    starts = fc.part_starts(case.t_count)
    got = fc.maps_by_parts(rows, fc.THR4, fc.EPS, fc.T_OFFSET, starts)
    assert fc.changed_maps(got, want) == []
    assert fc.changed_maps(fc.maps_by_parts(rows, fc.THR4, fc.EPS, fc.T_OFFSET, [0]), want) == []
    for v in fc.VARIANTS:
        assert fc.changed_maps(fc.maps_by_parts(rows, fc.THR4, fc.EPS, fc.T_OFFSET, starts, v), want), v
