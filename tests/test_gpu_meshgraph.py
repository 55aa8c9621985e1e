"""The mesh-graph kernels (k_locate_points, k_mesh_faces, k_mesh_edges) on the GPU against the
brute-force numpy restatements of tests/meshgraph_cases.py, against the rasterizer, against the
generator, and -- for graphs built from non-nested triangulations -- the engine on the built graph
against the oracle.  Indices are decided by fp64 predicates or vertex lists and the float64 arrays
are stated sequences of IEEE operations: everything but sqrt's results is compared bit for bit.
The rows that msw_locate_points writes sit between canary words; the dual graph's arrays are the
handle's own allocations and are copied out whole.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import meshgraph_cases as mc
import msgnn_torch as orc
import raster_cases as rc
from conftest import REL_TOL, build_msgnn, per_step_rel, state_dict_of
from mswegnn import _lib
from mswegnn.mesh import wet_state
from mswegnn.meshgraph import (DualGraph, PointLocator, _dual_numpy, graph_from_meshes, intra_edges, locate_launch,
                               mesh_dual_launch)
from mswegnn.raster import RasterGrid, Rasterizer
from mswegnn.series import Zones, rollout_zone_series
from test_gpu_raster import PADS, Out, stream_ptr
from test_meshgraph import GENERATOR, REFUSALS, assert_generator_equal, bits_equal, generator_case

pytestmark = pytest.mark.gpu

INVALID = -1


def raw_locator(xy, faces, rows, cuda):
    xy = np.ascontiguousarray(xy, np.float64)
    faces = np.ascontiguousarray(faces, np.int32)
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    h = C.c_void_p()
    _lib.check(_lib.lib().msw_locator_create(xy.ctypes.data_as(C.POINTER(C.c_double)), xy.shape[0],
                                             faces.ctypes.data_as(_lib.c_int32_p),
                                             None if rows is None else rows.ctypes.data_as(_lib.c_int32_p),
                                             faces.shape[0], cuda.index or 0, C.byref(h)))
    return h


def raw_locate(h, pts, cuda, pad=37):
    """msw_locate_points through ctypes into a canary-padded array -> (return code, Out)."""
    d = torch.from_numpy(np.ascontiguousarray(pts, np.float64)).to(cuda)
    out = Out((d.shape[0],), cuda, pad)
    code = _lib.lib().msw_locate_points(h, C.c_void_p(d.data_ptr()), d.shape[0], out.ptr, stream_ptr())
    torch.cuda.synchronize()
    return code, out


# ----------------------------------------------------------------------------- locate
@pytest.mark.parametrize("name", list(mc.LOCATE_CASES))
def test_locate_points(cuda, name):
    """Vertices, midpoints, centroids, their float64 neighbours, points outside the hull and the
    bucket grid, NaN, +-inf, -0.0; in planted order and shuffled (lanes diverge)."""
    xy, faces, rows = mc.LOCATE_CASES[name]
    pts = mc.probe_points(xy, faces)
    want = mc.locate_ref(xy, faces, rows, pts)
    assert (want >= 0).any() and (want < 0).any()
    h = raw_locator(xy, faces, rows, cuda)
    try:
        for pad in PADS:
            code, out = raw_locate(h, pts, cuda, pad)
            assert code == 0
            out.check(want, name)
        perm = np.random.default_rng(5).permutation(len(pts))
        code, out = raw_locate(h, pts[perm], cuda)
        assert code == 0
        out.check(want[perm], name + " shuffled")
    finally:
        _lib.lib().msw_locator_destroy(h)


def test_locate_counts(cuda):
    """n = 0, 1, 63, 64, 65, 129 and two and three grid-stride rounds (sizes from msw_locate_launch)."""
    xy, faces = rc.hex_fan()
    rows = np.array([5, -1, 3, 2, 1, 0], np.int32)
    base = mc.probe_points(xy, faces)
    base_want = mc.locate_ref(xy, faces, rows, base)
    grid, per_wg, _ = locate_launch(10 ** 9)
    sizes = [0, 1, 63, 64, 65, 129, grid * per_wg + 1, 2 * grid * per_wg + 7]
    assert [locate_launch(n)[2] for n in sizes[-2:]] == [2, 3]
    h = raw_locator(xy, faces, rows, cuda)
    try:
        none = Out((1,), cuda)                         # n = 0: nothing is launched, nothing written
        d = torch.zeros(1, 2, dtype=torch.float64, device=cuda)
        assert _lib.lib().msw_locate_points(h, C.c_void_p(d.data_ptr()), 0, none.ptr, stream_ptr()) == 0
        assert PointLocator(xy, faces, rows, device=cuda).locate(np.zeros((0, 2))).shape == (0,)
        torch.cuda.synchronize()
        assert none.untouched()
        for n in sizes[1:]:
            idx = (np.arange(n) * 7 + 3) % len(base)
            code, out = raw_locate(h, base[idx].reshape(-1, 2), cuda)
            assert code == 0
            out.check(base_want[idx], f"n = {n}")
    finally:
        _lib.lib().msw_locator_destroy(h)


@pytest.mark.parametrize("name", rc.NAMES)
def test_locate_equals_rasterizer(cuda, name):
    xy, faces, rows, grid = rc.CASES[name]
    g = RasterGrid(*grid)
    px, py = g.centres()
    pts = np.ascontiguousarray(np.stack(np.broadcast_arrays(px[None, :], py[:, None]), -1).reshape(-1, 2))
    got = PointLocator(xy, faces, rows, device=cuda).locate(pts)
    want = Rasterizer(xy, faces, g, rows, device=cuda).pixel_rows
    assert got.dtype == torch.int32 and torch.equal(got.reshape(g.shape), want)
    bits_equal(got.cpu().numpy().reshape(g.shape), rc.reference(name), name)


def test_locate_refusals(cuda):
    xy, faces = rc.hex_fan()
    h = raw_locator(xy, faces, None, cuda)
    lib = _lib.lib()
    try:
        d = torch.zeros(9, 2, dtype=torch.float64, device=cuda)
        out = Out((8,), cuda)
        p = C.c_void_p(d.data_ptr())
        assert lib.msw_locate_points(None, p, 8, out.ptr, stream_ptr()) == INVALID
        assert lib.msw_locate_points(h, None, 8, out.ptr, stream_ptr()) == INVALID
        assert lib.msw_locate_points(h, p, 8, None, stream_ptr()) == INVALID
        assert lib.msw_locate_points(h, p, -1, out.ptr, stream_ptr()) == INVALID
        assert lib.msw_locate_points(h, C.c_void_p(d.data_ptr() + 4), 8, out.ptr, stream_ptr()) == INVALID
        assert lib.msw_locate_points(h, p, 0, out.ptr, stream_ptr()) == 0
        torch.cuda.synchronize()
        assert out.untouched()
    finally:
        lib.msw_locator_destroy(h)
    bad = xy.copy()
    bad[2, 0] = np.nan
    with pytest.raises(ValueError):
        PointLocator(bad, faces, device=cuda)
    g = C.c_void_p()
    f32 = np.ascontiguousarray(faces, np.int32)
    assert lib.msw_locator_create(bad.ctypes.data_as(C.POINTER(C.c_double)), len(bad), f32.ctypes.data_as(_lib.c_int32_p),
                                  None, len(f32), 0, C.byref(g)) == INVALID and not g.value


def test_locator_stats_and_empty(cuda):
    xy, faces = rc.huge_and_tiny()
    loc = PointLocator(xy, faces, device=cuda)
    s = loc.stats()
    assert s["buckets"] == s["buckets_x"] * s["buckets_y"] >= 1 and s["list_entries"] >= len(faces)
    assert s["device_bytes"] >= 64 * len(faces) and s["longest_list"] >= 1
    loc.close()
    empty = PointLocator(np.zeros((3, 2)), np.zeros((0, 3), np.int32), device=cuda)
    assert empty.locate(np.array([[0.0, 0.0], [np.nan, 1.0]])).tolist() == [-1, -1]
    flat = PointLocator(np.array([[0.0, 0], [1, 1], [2, 2]]), np.array([[0, 1, 2]], np.int32), device=cuda)
    assert flat.locate(np.array([[1.0, 1.0]])).tolist() == [-1]


# ----------------------------------------------------------------------------- dual graph
@pytest.mark.parametrize("name", list(mc.DUAL_CASES))
def test_dual_graph(cuda, name):
    xy, faces = mc.DUAL_CASES[name]
    d, ref = DualGraph(xy, faces, device=cuda), mc.dual_ref(xy, faces)
    got, want = d.edge_length.cpu().numpy(), ref["edge_length"]
    if got.shape == want.shape and got.size:
        print(f"{name}: edge_length, worst |got - want| in ulps {(np.abs(got - want) / np.spacing(want)).max():.1f}")
    for k in ref:
        bits_equal(getattr(d, k).cpu().numpy(), ref[k], k)
    s = d.stats()
    assert s["num_faces"] == len(faces) and s["num_edges"] == d.num_edges and s["num_boundary"] == len(ref["boundary"])


def test_dual_graph_past_one_grid_round(cuda):
    grid, per_wg, _ = mesh_dual_launch(10 ** 9)
    n = int(np.ceil(np.sqrt((grid * per_wg + 1) / 2)))
    xy, faces = rc.squares(n)
    assert mesh_dual_launch(len(faces))[2] == 2
    d = DualGraph(xy, faces, device=cuda)
    # the numpy restatement, pinned to the dict-based one at small sizes by tests/test_meshgraph.py
    ref = dict(zip(DualGraph._NAMES, _dual_numpy(xy, faces)))
    for k in ref:
        bits_equal(getattr(d, k).cpu().numpy(), ref[k], k)


def test_dual_graph_empty(cuda):
    d = DualGraph(np.zeros((4, 2)), np.zeros((0, 3), np.int32), device=cuda)
    assert d.num_faces == 0 and d.num_edges == 0 and d.boundary.shape == (0, 2) and d.centroid.shape == (0, 2)
    assert d.edge_index.dtype == torch.int64 and d.edge_index.shape == (2, 0)


@pytest.mark.parametrize("name", list(REFUSALS))
def test_dual_graph_refusals(cuda, name):
    xy, faces, face, word = REFUSALS[name]
    with pytest.raises(ValueError, match=rf"face {face}: .*{word}"):
        DualGraph(xy, faces, device=cuda)


def test_dual_graph_unused_vertex_must_be_finite(cuda):
    xy, faces = rc.squares(2)
    with pytest.raises(ValueError, match="not finite"):
        DualGraph(np.concatenate([xy, [[np.nan, 0.0]]]), faces, device=cuda)


def test_intra_edges(cuda):
    scales = mc.GRAPH_CASES["overhang"][0]
    (fxy, ffn), (cxy, cfn) = scales[0], scales[1]
    fine = DualGraph(fxy, ffn, device=cuda)
    got = intra_edges(fine, PointLocator(cxy, cfn, device=cuda))
    bits_equal(got.cpu().numpy(), mc.intra_ref(fine.centroid.cpu().numpy(), cxy, cfn))


# ----------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name,shape", GENERATOR)
def test_generator_equality(cuda, name, shape, seed):
    g, scales, bc_xy, dem = generator_case(name, shape, seed)
    m = graph_from_meshes(scales, bc_xy, dem, T=6, BC=g.BC, device=cuda)
    assert_generator_equal(m.graph, g, m.centroids, scales)
    assert m.orphans == [0] * len(scales) and m.childless == [0] * len(scales)


@pytest.mark.parametrize("name", list(mc.GRAPH_CASES))
def test_graph_equals_restatement(cuda, name):
    scales, bc_xy, dem = mc.GRAPH_CASES[name]
    m = graph_from_meshes(scales, bc_xy, dem, T=6, device=cuda)
    ref = mc.graph_ref(scales, bc_xy, dem, T=6)
    for k in mc.GRAPH_ARRAYS:
        if k != "edge_attr":
            bits_equal(getattr(m.graph, k).numpy(), ref[k], k)
    got, want = m.graph.edge_attr.numpy(), ref["edge_attr"]
    assert got.shape == want.shape and (np.abs(got - want) <= np.spacing(np.maximum(np.abs(got), np.abs(want)))).all()
    assert m.bc_face == ref["bc_face"] and m.orphans == ref["orphans"] and m.childless == ref["childless"]


# ----------------------------------------------------------------------------- the engine on built graphs
def _rollout_against_oracle(cuda, case):
    scales, bc_xy, dem = mc.GRAPH_CASES[case]
    m = graph_from_meshes(scales, bc_xy, dem, T=6, device=cuda)
    g = m.graph
    children = np.bincount(g.intra_mesh_edge_index[0].numpy(), minlength=g.num_nodes)
    indeg = np.bincount(g.edge_index[1].numpy(), minlength=g.num_nodes)
    assert children.max() <= 16 and indeg.max() <= 3
    g = wet_state(g, seed=3)
    model = build_msgnn(3, 16, 2, seed=11)
    P, cfg = state_dict_of(model), orc.msgnn_config(num_scales=3, hid_features=16, K=2)
    ref = orc.rollout(P, cfg, g, 6)
    assert ref.abs().max() > 0.1
    model = model.to(cuda)
    model.engine = "hip"
    e = per_step_rel(model.rollout(g.to(cuda), 6).cpu(), ref)
    print(f"{case}: HIP on the built graph vs the oracle, worst per-step rel {e:.2e}")
    assert e <= REL_TOL, (case, e)
    return m, model


def test_non_nested_rollout(cuda):
    m, _ = _rollout_against_oracle(cuda, "non_nested")
    assert m.orphans == [0, 0, 0]
    children = np.bincount(m.graph.intra_mesh_edge_index[0].numpy())
    assert len(set(children[children > 0].tolist())) > 2


def test_overhang_rollout(cuda):
    m, _ = _rollout_against_oracle(cuda, "overhang")
    assert m.orphans[0] > 0


def test_gauges_feed_zone_series(cuda):
    scales, bc_xy, dem = mc.GRAPH_CASES["non_nested"]
    m = graph_from_meshes(scales, bc_xy, dem, T=6, device=cuda)
    g = wet_state(m.graph, seed=3)
    pts = np.array([[10.0, 10.0], [500.0, 480.0], [999.0, 3.0], [250.0, 750.0], [40.0, 520.0]])
    rows = mc.locate_ref(*scales[0], None, pts).astype(np.int64)
    assert (rows >= 0).all() and len(set(rows.tolist())) == len(pts)
    model = build_msgnn(3, 16, 2, seed=11).to(cuda)
    model.engine = "hip"
    gd = g.to(cuda)
    got = rollout_zone_series(model, gd, m.gauges(pts), 6, area=g.area)
    want = rollout_zone_series(model, gd, Zones.gauges(rows, g.num_nodes), 6, area=g.area)
    def same(u, v):
        if isinstance(u, dict):
            return u.keys() == v.keys() and all(same(u[k], v[k]) for k in u)
        return torch.equal(u, v) if torch.is_tensor(u) else u == v

    assert same(got, want) and float(got["h_max"].max()) > 0
    with pytest.raises(ValueError, match="lie in no cell"):
        m.gauges(np.array([[-5.0, 10.0]]))
