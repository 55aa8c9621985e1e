"""The zone-series kernel (msw_zone_series_update) on the GPU against ``_series_torch`` evaluated
on the CPU in float64 -- the reference has no counterpart for these series beyond the stored
volume inside its mass-conservation metric.

  * wet_cells, h_max, q_max: ``torch.equal``.
  * volume, wet_area: |got - want| <= 2 m 2^-53 sum|terms| per (zone, step), m the zone's row
    count.  Both sides add m terms that are exact in fp64 (a product of two floats, or a float) in
    some order, and every order is within (m - 1) 2^-53 sum|terms| of the true sum to first order:
    the bound is derived, not measured.  The largest observed ratio to it is printed when the
    module finishes (pytest -s).
  * however a rollout is cut into windows or pieces, and from call to call: ``torch.equal``.
Every output sits between canary words, and columns outside a call's window must keep theirs.

On the grid data of ``make_pred`` / ``make_area`` most sums are exact in fp64 in any order, so the
bound above says little about the order of additions that include/mswegnn.h promises (chunks of
256 list entries summed in list order from 0, then the chunk sums in chunk order).  The tests named
``*_wide`` and the slab tests run on full-mantissa data (tests/series_cases.py; a CPU test checks
that other orders of the same terms differ there in a quarter of the steps or more) and compare
``volume`` and ``wet_area`` with ``torch.equal`` against ``series_exact``, the documented order
restated in numpy.  The bound check stays beside it, and its reported worst ratio is now non-zero:
``_series_torch`` adds in another order.  The slab tests make ``msw_zone_series_update`` cut a window
into launches of S steps: 1024 by default, 128 and 64 for zone sets of 4096 and 4097 partial chunks.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import series_cases as sc
from conftest import build_msgnn, golden, manifest, weights
from mswegnn import _lib
from mswegnn.batch import collate
from mswegnn.floodmaps import FloodMaps, flood_maps, rollout_flood_maps
from mswegnn.mesh import make_multiscale_mesh, mesh_config, wet_state
from mswegnn.metrics import finest_ranges
from mswegnn.rollout import adapt_batch_training
from mswegnn.series import SERIES_NAMES, ZoneSeries, Zones, _series_torch, rollout_products, zone_series
from series_cases import THR4, make_area, make_area_wide, make_pred, make_pred_wide, sweep_zones

pytestmark = pytest.mark.gpu

FX = golden("fx_floodmaps")
PAD = 37          # canary words on each side of every output array
CANARY_F, CANARY_I = -12345.5, -123456789
WORST = {"volume": 0.0, "wet_area": 0.0}   # largest |got - want| / bound seen


@pytest.fixture(scope="module", autouse=True)
def report_worst_ratio():
    yield
    print(f"\nzone series: largest error / bound  volume {WORST['volume']:.3g}  wet_area {WORST['wet_area']:.3g}")


def expected(pred, zones, area, thr):
    """The yardstick on the CPU for pred [N, 2, t] (CPU, NaN allowed in rows no zone lists), plus
    sum|terms| of the volume."""
    zone, rows = zones.lists("cpu")
    want = _series_torch(pred, zone, rows, zones.num_zones, area, thr)
    want["abs_volume"] = _series_torch(pred.abs(), zone, rows, zones.num_zones, area, ())["volume"]
    return want


def check_series(got, want, zones, label=""):
    """got: {name: tensor} on any device, the columns that ``want`` covers."""
    m = zones.sizes.double()[:, None]
    for k, v in got.items():
        v = v.cpu()
        assert bool(torch.isfinite(v.double()).all()), f"{label}: {k} not finite"
        if k in ("volume", "wet_area"):
            assert v.dtype == torch.float64
            bound = 2 * m * 2.0 ** -53 * (want["abs_volume"] if k == "volume" else want[k])
            err = (v - want[k]).abs()
            assert bool((err <= bound).all()), f"{label}: {k} off by up to {float((err - bound).max()):.3g} over the bound"
            if bool((bound > 0).any()):
                WORST[k] = max(WORST[k], float((err[bound > 0] / bound[bound > 0]).max()))
        else:
            assert v.dtype == want[k].dtype and torch.equal(v, want[k]), f"{label}: {k}"


class Buffers:
    """Every output array [.., Z, T_out] inside a canary-filled allocation."""

    def __init__(self, Z, n_thr, T_out, dev, want=SERIES_NAMES):
        self.full, self.view = {}, {}
        for k in want:
            thr = k in ("wet_area", "wet_cells")
            if thr and n_thr == 0:
                continue
            dt = {"volume": torch.float64, "wet_area": torch.float64, "wet_cells": torch.int32}.get(k, torch.float32)
            shape = (n_thr, Z, T_out) if thr else (Z, T_out)
            size = int(np.prod(shape))
            self.full[k] = torch.full((size + 2 * PAD,), CANARY_I if dt == torch.int32 else CANARY_F, device=dev, dtype=dt)
            self.view[k] = self.full[k][PAD:PAD + size].view(shape)

    def struct(self):
        return _lib.MswZoneSeries(**{k: v.data_ptr() for k, v in self.view.items()})

    def check_canaries(self, col0, cols):
        """The pads, and every column outside [col0, col0 + cols)."""
        for k, b in self.full.items():
            c = CANARY_F if b.is_floating_point() else CANARY_I
            assert bool((b[:PAD] == c).all()) and bool((b[-PAD:] == c).all()), f"{k}: canary overwritten"
            v = self.view[k]
            assert bool((v[..., :col0] == c).all()) and bool((v[..., col0 + cols:] == c).all()), \
                f"{k}: a column outside the window was written"

    def window(self, col0, cols):
        return {k: v[..., col0:col0 + cols] for k, v in self.view.items()}


def update(zones, pred, bufs, t_begin, t_count, area, thr, T_out, t_out0, stream=None):
    th = (C.c_float * 4)(*(list(thr) + [0.0] * (4 - len(thr))))
    o = bufs.struct()
    st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    _lib.check(_lib.lib().msw_zone_series_update(zones.handle(pred.device), C.c_void_p(pred.data_ptr()), pred.shape[2],
                                                 t_begin, t_count, C.c_void_p(area.data_ptr() if area is not None else 0),
                                                 th, len(thr), T_out, t_out0, C.byref(o), st))


def check_exact(got, ref, label=""):
    """got: {name: tensor} on any device; ref: ``series_ref`` of the same columns.  Everything
    bit for bit, the sums included."""
    for k, v in got.items():
        assert v.dtype == ref[k].dtype and torch.equal(v.cpu(), ref[k]), f"{label}: {k} differs from the documented order"


def run_case(zones, host, dev, area_host, thr, t_begin, t_count, pad_cols=0, col0=0, label="", exact=False):
    """One raw ABI call into canary buffers, checked against the CPU yardstick (``exact``: and
    bit for bit against the order-exact restatement)."""
    area_dev = None if area_host is None else area_host.to(dev.device)
    bufs = Buffers(zones.num_zones, len(thr), t_count + pad_cols, dev.device)
    update(zones, dev, bufs, t_begin, t_count, area_dev, thr, t_count + pad_cols, col0)
    bufs.check_canaries(col0, t_count)
    want = expected(host[:, :, t_begin:t_begin + t_count], zones, area_host, thr)
    check_series(bufs.window(col0, t_count), want, zones, label)
    if exact:
        check_exact(bufs.window(col0, t_count), sc.series_ref(host[:, :, t_begin:t_begin + t_count], zones, area_host, thr), label)
    if not thr:
        assert not set(bufs.view) & {"wet_area", "wet_cells"}


def fixture_graph(name):
    """The input graph of a committed rollout (tests/test_oracle_golden.py builds them the same way)."""
    if name == "fx_small_K4_F32_rollout48":
        return make_multiscale_mesh(**mesh_config("small"), T=48)
    from mswegnn.mesh import irregularize
    spec = manifest()["fx_irr_spec"][name]
    g = make_multiscale_mesh(**mesh_config(spec["mesh"]), T=spec["T"])
    if spec["wet"] is not None:
        g = wet_state(g, seed=spec["wet"])
    return irregularize(g, spec["seed"], order="canonical")[0]


def fixture_zones(n, seed, graph=None):
    """A seeded random partition into 7 zones, 20 gauges and, with a graph, its finest rows."""
    gen = torch.Generator().manual_seed(seed)
    z = Zones.from_labels(torch.randint(0, 7, (n,), generator=gen), num_zones=7)
    z = z + Zones.gauges(torch.randint(0, n, (20,), generator=gen), n)
    return z if graph is None else z + Zones.finest(graph)


# ------------------------------------------------------------------ 1. the committed rollouts
@pytest.mark.parametrize("name", [str(n) for n in FX["rollouts"]])
def test_fixture_rollouts(cuda, name):
    host = torch.from_numpy(golden(name)["rollout"])
    n, _, T = host.shape
    g = fixture_graph(name)
    assert g.x.shape[0] == n
    zones = fixture_zones(n, 11, g)
    assert zones.num_zones == 28 and int(zones.sizes.max()) > 256     # a zone of several chunks
    dev = host.to(cuda)
    for area in (make_area(n, 5), None):
        for thr in ((), THR4[:2], THR4):
            run_case(zones, host, dev, area, thr, 0, T, label=f"{name} area={area is not None} n_thr={len(thr)}")
    # the public interface, with the cell areas of the graph
    assert g.area.shape == (n,)
    res = zone_series(dev, zones, area=g.area.to(cuda))
    want = expected(host, zones, g.area, (0.05, 0.3))
    check_series({k: res[k] for k in ("volume", "h_max", "q_max")}, want, zones, "zone_series")
    for i, t in enumerate((0.05, 0.3)):
        assert torch.equal(res["wet_cells"][t].cpu(), want["wet_cells"][i])
    zones.close()


# ------------------------------------------------------------------ 2. gauges
def test_gauge_identity(cuda):
    host = torch.from_numpy(golden(str(FX["rollouts"][0]))["rollout"])
    n = host.shape[0]
    rows = torch.randint(0, n, (50,), generator=torch.Generator().manual_seed(2))
    area = make_area(n, 6)
    dev = host.to(cuda)
    res = zone_series(dev, Zones.gauges(rows, n), area=area.to(cuda), thresholds=(0.05,))
    assert torch.equal(res["h_max"].cpu(), host[rows, 0, :])
    assert torch.equal(res["q_max"].cpu(), host[rows, 1, :].abs())
    assert torch.equal(res["volume"].cpu(), area[rows].double()[:, None] * host[rows, 0, :].double())
    wet = host[rows, 0, :] > 0.05
    assert torch.equal(res["wet_cells"][0.05].cpu(), wet.to(torch.int32))
    assert torch.equal(res["wet_area"][0.05].cpu(), torch.where(wet, area[rows].double()[:, None], torch.zeros((), dtype=torch.float64)))
    assert torch.equal(res["zone_area"].cpu(), area[rows].double())


# ------------------------------------------------------------------ 3. shape sweep
def _shape_sweep(cuda, T, wide):
    for n in (1, 17, 64, 65, 1000):
        zones, unlisted = sweep_zones(n, seed=n + T)
        host = make_pred_wide(n, T, seed=T) if wide else make_pred(n, T, seed=T)
        host[unlisted] = float("nan")
        area = make_area_wide(n, 8) if wide else make_area(n, 8)
        area[unlisted] = float("nan")
        store = torch.zeros(n * 2 * T + 8, device=cuda)
        for shift, a, thr in ((0, area, THR4[:2]), (1, None, THR4), (2, area, ()), (4, None, THR4[:1])):
            dev = store[shift:shift + n * 2 * T].view(n, 2, T)     # 4 floats = 16 bytes: aligned again
            dev.copy_(host)
            assert dev.data_ptr() % 16 == (4 * shift) % 16
            run_case(zones, host, dev, a, thr, 0, T, label=f"n={n} T={T} shift={shift}", exact=wide)
        # windows: t_begin > 0 (a multiple of 4, and odd), columns t_out0 > 0 of a wider output
        dev = host.to(cuda)
        for t_begin, t_count in ((T // 4 // 4 * 4, T - T // 4 // 4 * 4 - T // 8), (min(3, T - 1), max((T - 3) // 2, 1))):
            run_case(zones, host, dev, area, THR4[:2], t_begin, t_count, pad_cols=9, col0=5,
                     label=f"n={n} T={T} window=({t_begin}, {t_count})", exact=wide)
        zones.close()


@pytest.mark.parametrize("T", [1, 3, 47, 48, 65, 130, 132])
def test_shape_sweep(cuda, T):
    """T = 48 and 132 take the 16-byte loader from an aligned base (132: two full tiles and one of
    4 steps), every other T and every shifted base the scalar one."""
    _shape_sweep(cuda, T, wide=False)


@pytest.mark.parametrize("T", [1, 3, 47, 48, 65, 130, 132])
def test_shape_sweep_wide(cuda, T):
    """The same sweep on full-mantissa data, the sums compared bit for bit with the documented order."""
    _shape_sweep(cuda, T, wide=True)


# ------------------------------------------------------------------ 4. windows, pieces, repeats
def same_result(a, b):
    for k in ("volume", "h_max", "q_max"):
        assert torch.equal(a[k], b[k]), k
    for k in ("wet_area", "wet_cells"):
        for t in a[k]:
            assert torch.equal(a[k][t], b[k][t]), (k, t)


def result_window(res, thr):
    """A ``ZoneSeries.result`` as {name: tensor}, the threshold series stacked."""
    out = {k: res[k] for k in ("volume", "h_max", "q_max")}
    for k in ("wet_area", "wet_cells"):
        out[k] = torch.stack([res[k][float(t)] for t in thr])
    return out


def fed_in_pieces(zones, dev, split, how, kw):
    zs = ZoneSeries(zones, dev.shape[2], device=dev.device, **kw)
    t0 = 0
    for c in split:
        if how == "windows":
            zs.update(dev, t0, c)
        else:   # a rollout piece of its own, as rollout_chunks yields them
            zs.update(dev[:, :, t0:t0 + c].contiguous())
        t0 += c
    assert t0 == dev.shape[2]
    return zs.result()


def _windowing_invariance(cuda, wide):
    n, T = 1000, 48
    host = make_pred_wide(n, T, seed=4) if wide else make_pred(n, T, seed=4)
    dev = host.to(cuda)
    area = make_area_wide(n, 9) if wide else make_area(n, 9)
    zones = sweep_zones(n, seed=77)[0] + sc.permutation_zone(n)
    kw = dict(area=area.to(cuda), thresholds=THR4[:3])
    whole = zone_series(dev, zones, **kw)
    host_clean = host.clone()
    check_series({k: whole[k] for k in ("volume", "h_max", "q_max")}, expected(host_clean, zones, area, THR4[:3]), zones)
    if wide:
        check_exact(result_window(whole, THR4[:3]), sc.series_ref(host, zones, area, THR4[:3]), "whole")
    again = zone_series(dev, zones, **kw)
    same_result(again, whole)
    for split in ((1,) * 48, (7, 16, 25), (16, 16, 16), (4, 44)):
        for how in ("windows", "pieces"):
            same_result(fed_in_pieces(zones, dev, split, how, kw), whole)
    zones.close()


def test_windowing_invariance(cuda):
    _windowing_invariance(cuda, wide=False)


def test_windowing_invariance_wide(cuda):
    """On full-mantissa data, where another order of additions would show: the whole result bit
    for bit the documented order, and every cut bit for bit the whole."""
    _windowing_invariance(cuda, wide=True)


def test_wet_area_order_with_wide_areas(cuda):
    """Areas over 1 .. 1e4 add exactly in any order in zones of a few hundred entries; over
    1 .. 1e11 they round, and ``wet_area`` must follow the documented order as the volume does."""
    n = sc.N_SLAB
    zones = sc.default_slab_zones()
    area = make_area_wide(n, 6, **sc.AREA_SPAN)
    for T in (48, 47):       # the 16-byte and the scalar loader
        host = make_pred_wide(n, T, seed=5)
        run_case(zones, host, host.to(cuda), area, THR4, 0, T, pad_cols=9, col0=5, label=f"wide areas T={T}", exact=True)
    zones.close()


# ------------------------------------------------------------------ 4b. windows longer than one launch
@pytest.fixture(scope="module")
def slab_data():
    """The three multi-launch zone sets with their rollout (CPU), areas and the order-exact series
    of all its steps, computed once: a step's series depend on no other step, so a shorter T or a
    window is a slice of the columns."""
    out = {}
    for name, (make, S, Ts) in sc.SLAB_SETS.items():
        zones = make()
        assert sc.steps_per_launch(zones) == S
        host = sc.make_pred_wide(sc.N_SLAB, 1032 if name == "default" else 260, seed=5 if name == "default" else 7)
        host = host[:, :, :max(Ts)].contiguous()
        area = sc.make_area_wide(sc.N_SLAB, 6)
        thr = THR4 if name == "default" else THR4[:2]
        out[name] = dict(zones=zones, S=S, host=host, area=area, thr=thr, ref=sc.series_ref(host, zones, area, thr))
    yield out
    for d in out.values():
        d["zones"].close()


def run_slab_case(cuda, d, T, t_begin, t_count, label):
    """Window [t_begin, t_begin + t_count) of the first T steps as a rollout of its own, into
    columns 5.. of a wider canary-filled output, bit for bit against the shared reference."""
    zones, thr = d["zones"], d["thr"]
    dev = d["host"][:, :, :T].contiguous().to(cuda)
    assert dev.data_ptr() % 16 == 0 and t_count > d["S"]                     # two launches or more
    bufs = Buffers(zones.num_zones, len(thr), t_count + 9, cuda)
    update(zones, dev, bufs, t_begin, t_count, d["area"].to(cuda), thr, t_count + 9, 5)
    bufs.check_canaries(5, t_count)
    check_exact(bufs.window(5, t_count), {k: v[..., t_begin:t_begin + t_count] for k, v in d["ref"].items()}, label)


@pytest.mark.parametrize("T, t_begin, t_count", [(1028, 0, 1028), (1027, 0, 1027), (1032, 4, 1025)])
def test_default_slab(cuda, slab_data, T, t_begin, t_count):
    """S = 1024: 1024 + 4 with the 16-byte loader, 1024 + 3 with the scalar one, and a window
    1024 + 1 from step 4 (16-byte loader)."""
    d = slab_data["default"]
    run_slab_case(cuda, d, T, t_begin, t_count, f"T={T}")
    if T == 1028:   # beside it, the derived bound against _series_torch (the small zones make it cheap here)
        run_case(d["zones"], d["host"][:, :, :T].contiguous(), d["host"][:, :, :T].contiguous().to(cuda), d["area"], d["thr"],
                 0, T, pad_cols=9, col0=5, label="default slab")


@pytest.mark.parametrize("T", [132, 131, 260])
def test_shrunk_slab(cuda, slab_data, T):
    """S = 128 (4096 partial chunks): 128 + 4 with the 16-byte loader, 128 + 3 with the scalar
    one, and three launches."""
    run_slab_case(cuda, slab_data["shrunk"], T, 0, T, f"T={T}")


def test_floor_slab(cuda, slab_data):
    """S = 64, the floor (4097 partial chunks): 64 + 4."""
    run_slab_case(cuda, slab_data["floor"], 68, 0, 68, "T=68")


@pytest.mark.parametrize("name", list(sc.SLAB_SETS))
def test_chunked_equals_whole_across_slabs(cuda, slab_data, name):
    """``ZoneSeries.update`` fed in windows and in pieces cut at S - 1, S and S + 1 (so that a
    piece ends before, at and after the boundary between two launches of the whole, and the longer
    piece is itself cut into launches): bit for bit the whole, which is the documented order."""
    d = slab_data[name]
    S, thr = d["S"], d["thr"]
    dev = d["host"].to(cuda)
    T = dev.shape[2]
    kw = dict(area=d["area"].to(cuda), thresholds=thr)
    whole = zone_series(dev, d["zones"], **kw)
    check_exact(result_window(whole, thr), d["ref"], name)
    for cut in (S - 1, S, S + 1):
        for split in ((cut, T - cut), (T - cut, cut)):
            for how in ("windows", "pieces"):
                same_result(fed_in_pieces(d["zones"], dev, split, how, kw), whole)


# ------------------------------------------------------------------ 5. the unit loop
def test_several_unit_loop_iterations(cuda):
    T, big = 4, 190000
    n = big + 10000
    cap = Zones.gauges(torch.zeros(20000, dtype=torch.int64), 1).launch(T)[0]     # the grid of a large launch
    chunks_big = Zones.from_lists([torch.zeros(big, dtype=torch.int64)], 1).launch(T)[0]
    assert 1 < chunks_big < cap
    gauges = 2 * cap + cap // 3 + 13 - chunks_big                                  # two full rounds and a ragged third
    gen = torch.Generator().manual_seed(12)
    zones = Zones.from_lists([torch.randperm(n, generator=gen)[:big]], n) + Zones.gauges(torch.randint(0, n, (gauges,), generator=gen), n)
    grid, per_wg, iters = zones.launch(T)
    units = gauges + chunks_big
    assert grid == cap and per_wg == 1 and iters >= 3 and units % grid != 0 and grid * (iters - 1) < units <= grid * iters
    assert n * 2 * T * 4 < 16 << 20
    host = make_pred(n, T, seed=9)
    area = make_area(n, 10)
    run_case(zones, host, host.to(cuda), area, THR4[:2], 0, T, label=f"units={units} grid={grid}")
    zones.close()


# ------------------------------------------------------------------ 6. ties to the existing kernels
def test_h_max_equals_flood_maps(cuda):
    host = torch.from_numpy(golden(str(FX["rollouts"][1]))["rollout"])
    n = host.shape[0]
    zones = fixture_zones(n, 13)
    dev = host.to(cuda)
    per_cell = flood_maps(dev, want=("h_max", "q_max"))
    res = zone_series(dev, zones, want=("h_max", "q_max"))
    for k in ("h_max", "q_max"):
        for z in range(zones.num_zones):
            rows = zones.rows[zones.ptr[z]:zones.ptr[z + 1]].long().to(cuda)
            assert rows.numel() and torch.equal(res[k][z].max(), per_cell[k][rows].max()), (k, z)


def test_volume_equals_rollout_metrics_stored_volume(cuda):
    gs = [wet_state(make_multiscale_mesh(**mesh_config("tiny"), T=12), seed=1),
          make_multiscale_mesh(n_coarse=3, num_scales=4, seed=5, T=12)]
    b = adapt_batch_training(collate(gs))
    n, T = b.x.shape[0], 12
    ranges = finest_ranges(b)
    host = make_pred(n, T, seed=14)
    area = make_area(n, 15)
    dev, area_dev = host.to(cuda), area.to(cuda)
    S = len(ranges)
    sums = torch.zeros(S, T, 10, dtype=torch.float64, device=cuda)
    counts = torch.zeros(S, T, 1, 4, dtype=torch.int64, device=cuda)
    rng = (C.c_int64 * (2 * S))(*[v for r in ranges for v in r])
    _lib.check(_lib.lib().msw_rollout_metrics(C.c_void_p(dev.data_ptr()), C.c_void_p(dev.data_ptr()), T, rng, S,
                                              (C.c_float * 1)(0.0), 0, C.c_void_p(area_dev.data_ptr()),
                                              C.c_void_p(sums.data_ptr()), C.c_void_p(counts.data_ptr()),
                                              C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    zones = Zones.finest(b)
    assert zones.num_zones == 2
    vol = zone_series(dev, zones, area=area_dev, want=("volume",))["volume"].cpu()
    want = expected(host, zones, area, ())
    bound = 2 * zones.sizes.double()[:, None] * 2.0 ** -53 * want["abs_volume"]
    assert bool(((vol - sums[:, :, 9].cpu()).abs() <= bound).all())
    check_series({"volume": vol}, want, zones, "finest")


# ------------------------------------------------------------------ 7. the engine, end to end
@pytest.fixture(scope="module")
def engine(cuda):
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    m.engine = "hip"
    return m


def _same(u, v):
    if isinstance(u, dict):
        return u.keys() == v.keys() and all(_same(u[k], v[k]) for k in u)
    if isinstance(u, list):
        return len(u) == len(v) and all(_same(a, b) for a, b in zip(u, v))
    if not isinstance(u, torch.Tensor):
        return u == v
    if torch.is_floating_point(u):  # h_mean of an empty zone
        u, v = torch.nan_to_num(u, nan=-7.0), torch.nan_to_num(v, nan=-7.0)
    return torch.equal(u, v)


def _products_case(m, g, T, chunk, cuda):
    n = g.x.shape[0]
    zones = Zones.finest(g) + fixture_zones(n, 17) + Zones.from_lists([[]], n)
    area = make_area(n, 18).to(cuda)
    whole = m.rollout(g, T)
    maps, series = rollout_products(m, g, maps=FloodMaps(n, device=cuda), series=ZoneSeries(zones, T, area=area, device=cuda),
                                    steps=T, chunk=chunk)
    assert _same(series, zone_series(whole, zones, area=area))
    assert _same(maps, rollout_flood_maps(m, g, T, chunk=chunk))
    want = expected(whole.cpu(), zones, area.cpu(), (0.05, 0.3))
    check_series({k: series[k] for k in ("volume", "h_max", "q_max")}, want, zones, f"chunk={chunk}")
    zones.close()


@pytest.mark.parametrize("chunk", [16, 7])
def test_engine_rollout_products(cuda, engine, chunk):
    g = wet_state(make_multiscale_mesh(**mesh_config("tiny"), T=20), seed=1).to(cuda)
    _products_case(engine, g, 20, chunk, cuda)


def test_engine_rollout_products_on_a_batch(cuda, engine):
    gs = [wet_state(make_multiscale_mesh(**mesh_config("tiny"), T=20), seed=1),
          make_multiscale_mesh(n_coarse=3, num_scales=4, seed=5, T=20)]
    b = adapt_batch_training(collate(gs)).to(cuda)
    _products_case(engine, b, 20, 16, cuda)


def test_update_behind_rollout_on_a_side_stream(cuda, engine):
    from mswegnn.engine import plan_for
    g = wet_state(make_multiscale_mesh(**mesh_config("tiny"), T=20), seed=1).to(cuda)
    whole = engine.rollout(g, 20)
    zones = fixture_zones(g.x.shape[0], 19, g)
    want = zone_series(whole, zones)
    plan = plan_for(engine, g)
    side = torch.cuda.Stream(cuda)
    zs = ZoneSeries(zones, 20, device=cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = plan.rollout(g.x, g.BC, g.node_BC, g.type_BC, 20)
        zs.update(out)       # enqueued directly behind the rollout: no synchronisation in between
    side.synchronize()
    assert torch.equal(out, whole)
    assert _same(zs.result(), want)
    zones.close()


def test_zones_create_rejects_a_row_past_the_end(cuda):
    lib = _lib.lib()
    ptr, rows, out = (C.c_int64 * 2)(0, 3), (C.c_int32 * 3)(0, 10, 4), C.c_void_p(1234)
    assert lib.msw_zones_create(ptr, rows, 1, 10, cuda.index, C.byref(out)) == -1   # MSW_ERR_INVALID: 10 == num_rows
    assert "row id" in lib.msw_last_error().decode() and not out.value              # nothing was allocated
    rows[1] = 9
    assert lib.msw_zones_create(ptr, rows, 1, 10, cuda.index, C.byref(out)) == _lib.MSW_OK and out.value
    assert lib.msw_zones_destroy(out) == _lib.MSW_OK
