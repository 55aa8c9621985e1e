"""Zone series without a GPU: the torch restatement ``_series_torch`` against hand-computed
values, the ``Zones`` constructors, chunked against whole on the torch path, ``rollout_products``
against the two separate passes, and the host side of the C ABI (error returns, no-ops, the launch
query: all of them return before any HIP call; a host-only zone set, device -1, stands in for a
device one).  Then the kernel's test cases themselves (tests/series_cases.py): the order-exact
restatement against ``_series_torch``, the condition on the data that makes the order of additions
visible, and a census of the steps per launch of the multi-launch zone sets.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import series_cases as sc
from conftest import build_msgnn, weights
from mswegnn import _lib
from mswegnn.floodmaps import FloodMaps, rollout_flood_maps
from mswegnn.mesh import make_multiscale_mesh, mesh_config, wet_state
from mswegnn.batch import collate
from mswegnn.metrics import finest_ranges
from mswegnn.rollout import adapt_batch_training
from mswegnn.series import (SERIES_NAMES, ZoneSeries, Zones, _series_torch, rollout_products, rollout_zone_series,
                            zone_series)

F05 = float(torch.tensor(0.05, dtype=torch.float32))  # the float32 threshold, exactly


def hand_example():
    """5 rows, 3 steps.  Zones: 0 = rows (0, 1, 2); 1 = rows (2, 3, 3): overlaps zone 0 and lists
    row 3 twice; 2 = empty; 3 = row 4.  Depths sit exactly at both thresholds (strict >)."""
    h = torch.tensor([[0.0, F05, 1.0], [0.5, 0.25, 0.0], [0.75, 0.5, 2.0], [0.0, 1.5, F05], [3.0, 0.0, 0.5]])
    q = torch.tensor([[-1.0, 0.5, 0.0], [0.25, -2.0, 0.0], [0.0, 0.0, -0.5], [4.0, -0.125, 0.0], [0.0, 0.0, -8.0]])
    pred = torch.stack((h, q), 1)
    area = torch.tensor([1.0, 2.0, 3.0, 4.0, 0.5])
    zones = Zones.from_lists([[0, 1, 2], [2, 3, 3], [], [4]], 5)
    want = {
        "volume": [[3.25, F05 + 2.0, 7.0], [2.25, 13.5, 6.0 + 8.0 * F05], [0.0, 0.0, 0.0], [1.5, 0.0, 0.25]],
        "h_max": [[0.75, 0.5, 2.0], [0.75, 1.5, 2.0], [0.0, 0.0, 0.0], [3.0, 0.0, 0.5]],
        "q_max": [[1.0, 2.0, 0.5], [4.0, 0.125, 0.5], [0.0, 0.0, 0.0], [0.0, 0.0, 8.0]],
        "wet_cells": [[[2, 2, 2], [1, 3, 1], [0, 0, 0], [1, 0, 1]],      # h > 0.05
                      [[1, 0, 2], [1, 2, 1], [0, 0, 0], [1, 0, 0]]],     # h > 0.5
        "wet_area": [[[5.0, 5.0, 4.0], [3.0, 11.0, 3.0], [0.0, 0.0, 0.0], [0.5, 0.0, 0.5]],
                     [[3.0, 0.0, 4.0], [3.0, 8.0, 3.0], [0.0, 0.0, 0.0], [0.5, 0.0, 0.0]]],
        "zone_area": [6.0, 11.0, 0.0, 0.5],
    }
    return pred, area, zones, want


def test_series_torch_equals_hand_computed_values():
    pred, area, zones, want = hand_example()
    zone, rows = zones.lists("cpu")
    got = _series_torch(pred, zone, rows, 4, area, (0.05, 0.5))
    assert set(got) == set(SERIES_NAMES)
    for k in ("volume", "wet_area"):
        assert got[k].dtype == torch.float64
        assert torch.equal(got[k], torch.tensor(want[k], dtype=torch.float64)), k
    assert got["wet_cells"].dtype == torch.int32
    assert torch.equal(got["wet_cells"], torch.tensor(want["wet_cells"], dtype=torch.int32))
    for k in ("h_max", "q_max"):
        assert got[k].dtype == torch.float32 and torch.equal(got[k], torch.tensor(want[k])), k
    # no thresholds: empty threshold series of the right shape; no area: every cell counts 1
    got = _series_torch(pred, zone, rows, 4, None, ())
    assert got["wet_area"].shape == (0, 4, 3) and got["wet_cells"].shape == (0, 4, 3)
    assert torch.equal(got["volume"][1], pred[2, 0].double() + 2 * pred[3, 0].double())


def test_public_result_of_the_hand_example():
    pred, area, zones, want = hand_example()
    res = zone_series(pred, zones, area=area, thresholds=(0.05, 0.5))
    assert res["steps"] == 3
    assert torch.equal(res["zone_area"], torch.tensor(want["zone_area"], dtype=torch.float64))
    assert torch.equal(res["volume"], torch.tensor(want["volume"], dtype=torch.float64))
    for i, t in enumerate((0.05, 0.5)):
        assert torch.equal(res["wet_cells"][t], torch.tensor(want["wet_cells"][i], dtype=torch.int32))
        assert torch.equal(res["wet_area"][t], torch.tensor(want["wet_area"][i], dtype=torch.float64))
    hm = res["h_mean"]
    assert hm.dtype == torch.float64 and torch.equal(hm[0], res["volume"][0] / 6.0)
    assert bool(torch.isnan(hm[2]).all())                       # the empty zone
    # a subset of the series, and the guards of the interface
    sub = zone_series(pred, zones, want=("h_max",))
    assert "volume" not in sub and "h_mean" not in sub and torch.equal(sub["h_max"], res["h_max"])
    with pytest.raises(ValueError):
        ZoneSeries(zones, 3, want=("depth",))
    with pytest.raises(ValueError):
        ZoneSeries(zones, 3, thresholds=(0.1,) * 5)
    with pytest.raises(ValueError):
        ZoneSeries(zones, 3, area=area[:4])
    with pytest.raises(ValueError):
        ZoneSeries(zones, 2).update(pred)                      # more steps than the series hold
    with pytest.raises(ValueError):
        ZoneSeries(zones, 3).update(pred[:4])                  # other rows than the zones are over


def test_zones_constructors():
    z = Zones.from_labels([2, -1, 0, 2, 0, -1, 2])
    assert z.num_rows == 7 and z.num_zones == 3 and len(z) == 3
    assert z.ptr.tolist() == [0, 2, 2, 5] and z.rows.tolist() == [2, 4, 0, 3, 6]
    assert z.sizes.tolist() == [2, 0, 3]
    assert Zones.from_labels([0, -1], num_zones=3).ptr.tolist() == [0, 1, 1, 1]
    assert Zones.from_labels(torch.full((4,), -1)).num_zones == 0
    with pytest.raises(ValueError):
        Zones.from_labels([0, -2])
    with pytest.raises(ValueError):
        Zones.from_labels([0, 3], num_zones=2)

    z = Zones.from_lists([[3, 1, 1], [], torch.tensor([0, 3])], 4)        # unsorted, duplicated, overlapping
    assert z.ptr.tolist() == [0, 3, 3, 5] and z.rows.tolist() == [3, 1, 1, 0, 3] and z.rows.dtype == torch.int32
    assert Zones.from_lists([], 4).num_zones == 0
    for bad in ([[4]], [[-1]]):
        with pytest.raises(ValueError):
            Zones.from_lists(bad, 4)

    g = Zones.gauges([5, 0, 5], 6)
    assert g.ptr.tolist() == [0, 1, 2, 3] and g.rows.tolist() == [5, 0, 5]

    both = Zones.from_lists([[1, 2], [0]], 6) + g
    assert both.ptr.tolist() == [0, 2, 3, 4, 5, 6] and both.rows.tolist() == [1, 2, 0, 5, 0, 5]
    with pytest.raises(ValueError):
        both + Zones.gauges([0], 7)
    zone, rows = both.lists("cpu")
    assert zone.tolist() == [0, 0, 1, 2, 3, 4] and rows.dtype == torch.int64


def test_zones_finest_on_a_graph_and_a_batch():
    g1 = make_multiscale_mesh(**mesh_config("tiny"), T=4)
    g2 = make_multiscale_mesh(n_coarse=3, num_scales=4, seed=5, T=4)
    z = Zones.finest(g1)
    (s, e), = finest_ranges(g1)
    assert z.num_zones == 1 and z.num_rows == g1.x.shape[0] and z.rows.tolist() == list(range(s, e))
    b = adapt_batch_training(collate([g1, g2]))
    z = Zones.finest(b)
    assert z.num_zones == 2 and z.num_rows == b.x.shape[0]
    for k, (s, e) in enumerate(finest_ranges(b)):
        assert z.rows[z.ptr[k]:z.ptr[k + 1]].tolist() == list(range(s, e))


def _random_case(n=40, T=19, seed=0):
    gen = torch.Generator().manual_seed(seed)
    pred = torch.rand(n, 2, T, generator=gen) - 0.3
    area = torch.rand(n, generator=gen) + 0.5
    labels = torch.randint(-1, 4, (n,), generator=gen)
    zones = Zones.from_labels(labels, num_zones=5) + Zones.gauges([3, 3, 17], n)
    return pred, area, zones


@pytest.mark.parametrize("chunk", [1, 3, 16])
def test_cpu_chunked_equals_whole(chunk):
    pred, area, zones = _random_case()
    whole = zone_series(pred, zones, area=area)
    for how in ("windows", "pieces"):
        zs = ZoneSeries(zones, pred.shape[2], area=area)
        for t0 in range(0, pred.shape[2], chunk):
            n = min(chunk, pred.shape[2] - t0)
            if how == "windows":
                zs.update(pred, t0, n)
            else:
                zs.update(pred[:, :, t0:t0 + n].contiguous())
        assert _same(zs.result(), whole), (how, chunk)


def _same(u, v):
    if isinstance(u, dict):
        return u.keys() == v.keys() and all(_same(u[k], v[k]) for k in u)
    if isinstance(u, (list, tuple)):
        return len(u) == len(v) and all(_same(a, b) for a, b in zip(u, v))
    if not isinstance(u, torch.Tensor):
        return u == v
    if torch.is_floating_point(u):  # h_mean of an empty zone, arrival_hours of a dry cell
        u, v = torch.nan_to_num(u, nan=-7.0), torch.nan_to_num(v, nan=-7.0)
    return u.dtype == v.dtype and torch.equal(u, v)


@pytest.fixture(scope="module")
def tiny():
    m = build_msgnn(num_scales=4, hid=32, K=4, state=weights("K4_F32"))
    g = wet_state(make_multiscale_mesh(**mesh_config("tiny"), T=9), seed=1)
    return m, g


@pytest.mark.parametrize("chunk", [None, 4])
def test_rollout_products_equal_the_two_passes(tiny, chunk):
    m, g = tiny
    n = g.x.shape[0]
    zones = Zones.finest(g) + Zones.from_labels(torch.arange(n) % 3) + Zones.gauges([0, n - 1], n)
    area = torch.rand(n, generator=torch.Generator().manual_seed(3)) + 0.5
    maps_alone = rollout_flood_maps(m, g, 9, chunk=chunk)
    series_alone = rollout_zone_series(m, g, zones, 9, chunk=chunk, area=area)
    assert _same(series_alone, zone_series(m.rollout(g, 9), zones, area=area))
    maps, series = rollout_products(m, g, maps=FloodMaps(n), series=ZoneSeries(zones, 9, area=area), steps=9,
                                    chunk=chunk)
    assert _same(maps, maps_alone) and _same(series, series_alone)
    # a list of maps, one product only
    ranges = finest_ranges(g)
    maps, series = rollout_products(m, g, maps=[FloodMaps(e - s, s) for s, e in ranges], steps=9, chunk=chunk)
    assert series is None and _same(maps, rollout_flood_maps(m, g, 9, chunk=chunk, ranges=ranges))
    maps, series = rollout_products(m, g, series=ZoneSeries(zones, 9, area=area), steps=9, chunk=chunk)
    assert maps is None and _same(series, series_alone)


# ------------------------------------------------------------------ C ABI, host side only
MSW_ERR_INVALID = -1


@pytest.fixture(scope="module")
def lib():
    return _lib.lib()


def _create(lib, ptr, rows, num_rows, device=-1, null=()):
    p = (C.c_int64 * len(ptr))(*ptr)
    r = (C.c_int32 * max(len(rows), 1))(*rows)
    out = C.c_void_p(1234)
    rc = lib.msw_zones_create(None if "ptr" in null else p, None if "rows" in null else r, len(ptr) - 1, num_rows,
                              device, None if "out" in null else C.byref(out))
    return rc, out


@pytest.fixture(scope="module")
def host_zones(lib):
    """A host-only zone set: sizes 300 (two chunks), 0, 1."""
    rc, h = _create(lib, [0, 300, 300, 301], list(range(300)) + [7], 400)
    assert rc == _lib.MSW_OK and h.value
    yield h
    assert lib.msw_zones_destroy(h) == _lib.MSW_OK


@pytest.mark.parametrize("kw, text", [
    (dict(rows=[0, 1, 5]), "row id"), (dict(rows=[0, -1, 2]), "row id"),      # 5 == num_rows
    (dict(ptr=[0, 2, 1, 3]), "monotone"), (dict(ptr=[1, 2, 3]), "start at 0"),
    (dict(null=("ptr",)), "null"), (dict(null=("rows",)), "null"), (dict(null=("out",)), "null"),
    (dict(num_rows=-1), "out of range"), (dict(device=-2), "out of range"),
])
def test_abi_zones_create_rejects_bad_arguments(lib, kw, text):
    a = dict(ptr=[0, 1, 3], rows=[0, 1, 2], num_rows=5)
    a.update(kw)
    rc, out = _create(lib, **a)
    assert rc == MSW_ERR_INVALID and text in lib.msw_last_error().decode()
    if "out" not in a.get("null", ()):
        assert not out.value, "a handle came back with the error"


def test_abi_zones_destroy_accepts_null(lib):
    assert lib.msw_zones_destroy(None) == _lib.MSW_OK


def _update(lib, zones, pred=1, T=8, t_begin=0, t_count=8, thr=True, n_thr=2, T_out=8, t_out0=0, out=True):
    """msw_zone_series_update with dummy non-NULL addresses: every call here must return before
    anything is launched or dereferenced."""
    o = _lib.MswZoneSeries()
    th = (C.c_float * 4)(0.05, 0.3, 0, 0)
    return lib.msw_zone_series_update(zones, C.c_void_p(4096 if pred else 0), T, t_begin, t_count, None,
                                      th if thr else None, n_thr, T_out, t_out0, C.byref(o) if out else None, None)


@pytest.mark.parametrize("kw, text", [
    (dict(pred=0), "null"), (dict(out=False), "null"), (dict(thr=False), "null"), (dict(zones=None), "null"),
    (dict(n_thr=5), "n_thr"), (dict(n_thr=-1), "n_thr"),
    (dict(t_begin=-1), "window"), (dict(t_begin=4, t_count=5), "window"), (dict(t_count=-1), "window"),
    (dict(T=-1, t_count=0), "window"),
    (dict(t_out0=1), "output columns"), (dict(T_out=7), "output columns"), (dict(t_out0=-1, t_count=4), "output columns"),
    (dict(), "without a device"),                               # a host-only set cannot be updated
])
def test_abi_update_rejects_bad_arguments(lib, host_zones, kw, text):
    kw = dict(kw)
    zones = kw.pop("zones", host_zones)
    assert _update(lib, zones, **kw) == MSW_ERR_INVALID
    assert text in lib.msw_last_error().decode()


def test_abi_update_no_ops(lib, host_zones):
    assert _update(lib, host_zones, t_count=0) == _lib.MSW_OK
    assert _update(lib, host_zones, t_count=0, thr=False, n_thr=0, T_out=0) == _lib.MSW_OK
    rc, empty = _create(lib, [0], [], 10)
    assert rc == _lib.MSW_OK
    assert _update(lib, empty) == _lib.MSW_OK                    # no zones
    assert lib.msw_zones_destroy(empty) == _lib.MSW_OK


def _launch(lib, zones, t_count):
    g, u, it = C.c_int32(7), C.c_int32(7), C.c_int32(7)
    assert lib.msw_zone_series_launch(zones, t_count, C.byref(g), C.byref(u), C.byref(it)) == _lib.MSW_OK
    return g.value, u.value, it.value


def test_abi_launch_query(lib, host_zones):
    # chunks: 2 + 1 (the empty zone still writes its zeros) + 1; one tile per 64 steps
    assert _launch(lib, host_zones, 1) == (4, 1, 1)
    assert _launch(lib, host_zones, 64) == (4, 1, 1)
    assert _launch(lib, host_zones, 65) == (8, 1, 1)
    assert _launch(lib, host_zones, 0) == (0, 1, 0)
    g, u, it = C.c_int32(), C.c_int32(), C.c_int32()
    assert lib.msw_zone_series_launch(host_zones, -1, C.byref(g), C.byref(u), C.byref(it)) == MSW_ERR_INVALID
    assert lib.msw_zone_series_launch(None, 8, C.byref(g), C.byref(u), C.byref(it)) == MSW_ERR_INVALID
    assert lib.msw_zone_series_launch(host_zones, 8, None, C.byref(u), C.byref(it)) == MSW_ERR_INVALID


@pytest.mark.parametrize("gauges, t_count", [(1, 4), (4096, 4), (4097, 4), (10000, 4), (3000, 130), (100000, 2000)])
def test_abi_launch_is_consistent(gauges, t_count):
    zones = Zones.gauges(torch.zeros(gauges, dtype=torch.int64), 1) + Zones.from_lists([[0] * 1000], 1)
    g, u, it = zones.launch(t_count)
    per_launch = min(t_count, 1024)                              # 4 partial chunks: the scratch allows 1024 steps
    units = (gauges + 4) * -(-per_launch // 64)
    assert u == 1 and 1 <= g <= units
    assert g * it >= units and g * (it - 1) < units, "iters is not minimal"
    zones.close()


def test_struct_size(lib):
    assert lib.msw_struct_size(b"msw_zone_series") == C.sizeof(_lib.MswZoneSeries) == 40


# ------------------------------------------------------------------ the kernel's test cases
def test_series_ref_equals_series_torch():
    """``series_ref`` against the yardstick of the other tests: bit for bit on data whose sums are
    exact in any order (depths on a 2^-12 grid, areas on a 2^-4 grid: every term a multiple of
    2^-16 below 2^18), and on the wide data the order-free series bit for bit, the sums within
    2 m 2^-53 sum|terms|."""
    n, T = 300, 37
    zones = sc.default_slab_zones() + Zones.gauges([5, 5, 299], n)
    zone, rows = zones.lists("cpu")
    wide, area = sc.make_pred_wide(n, T, seed=2), sc.make_area_wide(n, seed=3)
    grid = torch.round(wide * 4096) / 4096
    area_grid = torch.round(area * 16) / 16
    for a in (area_grid, None):
        want = _series_torch(grid, zone, rows, zones.num_zones, a, sc.THR4)
        got = sc.series_ref(grid, zones, a, sc.THR4)
        assert set(got) == set(SERIES_NAMES)
        for k in SERIES_NAMES:
            assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    want = _series_torch(wide, zone, rows, zones.num_zones, area, sc.THR4)
    got = sc.series_ref(wide, zones, area, sc.THR4)
    for k in ("wet_cells", "h_max", "q_max"):
        assert torch.equal(got[k], want[k]), k
    m = zones.sizes.double()[:, None]
    for k in ("volume", "wet_area"):     # non-negative terms: sum|terms| is the sum itself
        assert bool(((got[k] - want[k]).abs() <= 2 * m * 2.0 ** -53 * want[k]).all()), k
    assert not torch.equal(got["volume"], want["volume"])      # and the order does show


def test_series_exact_by_hand():
    """The documented order restated entry by entry in plain Python floats, on a zone of three
    chunks (600 entries) and one of one entry."""
    n, T = 40, 3
    pred, area = sc.make_pred_wide(n, T, seed=4), sc.make_area_wide(n, seed=5)
    rows = torch.randint(0, n, (601,), generator=torch.Generator().manual_seed(6))
    zones = Zones.from_lists([rows[:600], rows[600:]], n)
    got = sc.series_exact(pred, zones.ptr, zones.rows, area, (0.05,))
    for t in range(T):
        sums, wet = [], []
        for c0 in range(0, 600, 256):
            v = w = 0.0
            for r in rows[c0:min(c0 + 256, 600)].tolist():
                v += float(area[r]) * float(pred[r, 0, t])
                w += float(area[r]) if float(pred[r, 0, t]) > sc.f32(0.05) else 0.0
            sums.append(v)
            wet.append(w)
        assert got["volume"][0, t] == ((0.0 + sums[0]) + sums[1]) + sums[2]
        assert got["wet_area"][0, 0, t] == ((0.0 + wet[0]) + wet[1]) + wet[2]
        r = int(rows[600])
        assert got["volume"][1, t] == float(area[r]) * float(pred[r, 0, t])


def _order_cases():
    """(label, zones, pred, area) of the GPU tests that compare sums exactly."""
    for n in (17, 64, 65, 1000):
        for T in (47, 48, 65, 130, 132):
            yield f"sweep n={n} T={T}", sc.sweep_zones(n, seed=n + T)[0], sc.make_pred_wide(n, T, seed=T), sc.make_area_wide(n, 8)
    yield "windowing", sc.sweep_zones(1000, seed=77)[0] + sc.permutation_zone(1000), sc.make_pred_wide(1000, 48, seed=4), \
        sc.make_area_wide(1000, 9)
    yield "default slab", sc.default_slab_zones(), sc.make_pred_wide(sc.N_SLAB, 1032, seed=5), sc.make_area_wide(sc.N_SLAB, 6)
    big = sc.make_pred_wide(sc.N_SLAB, 260, seed=7)[:, :, :68].contiguous()
    yield "shrunk slab", sc.big_zones(), big, sc.make_area_wide(sc.N_SLAB, 6)
    yield "floor slab", sc.big_zones(1), big, sc.make_area_wide(sc.N_SLAB, 6)


def test_wide_data_is_order_sensitive():
    """The condition that makes the exact comparisons of tests/test_gpu_series.py mean something:
    in every zone of 16 entries or more, the same terms added in reversed list order, as a
    balanced tree, and (three chunks or more: two chunk sums commute) with the chunk sums in
    reversed order each differ from ``series_exact`` in a quarter of the steps or more.  The
    sweep's cases with one row (every term of a zone is the same number: reversal cannot show) and
    with T = 1 and 3 (no quarter to speak of) are left out.  The smallest fractions are printed."""
    worst = {"reversed": 1.0, "pairwise": 1.0, "chunks reversed": 1.0}
    several = 0
    for label, zones, pred, area in _order_cases():
        ptr, rows = zones.ptr.numpy(), zones.rows.numpy()
        exact = sc.series_exact(pred, ptr, rows, area)["volume"]
        for z in range(zones.num_zones):
            m = int(ptr[z + 1] - ptr[z])
            if m < 16:
                continue
            orders = {"reversed": sc.volume_reversed, "pairwise": sc.volume_pairwise}
            if m > 2 * sc.CHUNK:
                orders["chunks reversed"] = sc.volume_chunks_reversed
                several += 1
            for name, fn in orders.items():
                f = sc.differing_fraction(fn(pred, ptr, rows, area, z), exact[z])
                worst[name] = min(worst[name], f)
                assert f >= 0.25, f"{label}: zone {z} of {m} entries, {name}: only {f:.0%} of the steps differ"
    assert several >= 4
    print("\nwide data, smallest fraction of steps that differ from the documented order: "
          + ", ".join(f"{k} {v:.0%}" for k, v in worst.items()))


def test_wide_areas_make_wet_area_order_sensitive():
    """Areas over 1 .. 1e4 add exactly in any order in zones of this size, so the default data pin
    the order of ``wet_area`` only in the million-entry zone.  With AREA_SPAN the condition above
    holds for ``wet_area`` at threshold 0.0 in the zones of 255 entries and more of the default
    slab set (a few 24-bit terms seldom round, whatever their spread: the small zones are left to
    the volume)."""
    zones = sc.default_slab_zones()
    pred = sc.make_pred_wide(sc.N_SLAB, 48, seed=5)
    ptr, rows = zones.ptr.numpy(), zones.rows.numpy()
    narrow = sc.make_area_wide(sc.N_SLAB, 6)
    wet = sc.wetness(pred, 0.0)
    assert np.array_equal(sc.series_exact(pred, ptr, rows, narrow, (0.0,))["wet_area"][0],
                          sc.series_exact(wet, ptr, rows, narrow)["volume"])
    for z in range(zones.num_zones):
        assert sc.differing_fraction(sc.volume_reversed(wet, ptr, rows, narrow, z),
                                     sc.series_exact(wet, ptr, rows, narrow)["volume"][z]) == 0.0
    area = sc.make_area_wide(sc.N_SLAB, 6, **sc.AREA_SPAN)
    exact = sc.series_exact(pred, ptr, rows, area, (0.0,))["wet_area"][0]
    for z in range(zones.num_zones):
        m = int(ptr[z + 1] - ptr[z])
        if m < 255:
            continue
        orders = [sc.volume_reversed, sc.volume_pairwise] + ([sc.volume_chunks_reversed] if m > 2 * sc.CHUNK else [])
        for fn in orders:
            f = sc.differing_fraction(fn(wet, ptr, rows, area, z), exact[z])
            assert f >= 0.25, f"zone {z} of {m} entries, {fn.__name__}: only {f:.0%} of the steps differ"


def test_census_of_steps_per_launch():
    """The steps per launch S of the three multi-launch zone sets, recovered from the launch
    query, and that every T the GPU tests run on them needs two launches or more."""
    for name, (make, S, Ts) in sc.SLAB_SETS.items():
        zones = make()
        assert sc.steps_per_launch(zones) == S, name
        assert all(T > S for T in Ts), name
        assert zones.launch(S) == zones.launch(10 * S)              # a longer window launches no more at once
        zones.close()
    # exactly 4096 chunks: iters is the tiles of a launch
    only = Zones.from_lists([torch.zeros(sc.BIG, dtype=torch.int64)], 1)
    assert [only.launch(t)[2] for t in (64, 65, 128, 129, 5000)] == [1, 2, 2, 2, 2]
    only.close()
