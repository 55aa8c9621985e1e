"""mswegnn.meshgraph on the CPU (the numpy restatements behind PointLocator, DualGraph and
graph_from_meshes) against the brute-force restatements of tests/meshgraph_cases.py, against
mswegnn.mesh's own ``_dual_graph`` and against the generator: on the geometry that
``multiscale_geometry`` returns, ``graph_from_meshes`` must reproduce ``make_multiscale_mesh``'s
graph from the coordinates and vertex lists alone.  tests/test_gpu_meshgraph.py runs the same
comparisons through the HIP kernels.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import meshgraph_cases as mc
import raster_cases as rc
from mswegnn import _lib
from mswegnn.mesh import _dual_graph, make_multiscale_mesh, mesh_config
from mswegnn.meshgraph import (DualGraph, PointLocator, graph_from_meshes, intra_edges, locate_launch,
                               mesh_dual_launch)

GENERATOR = [("tiny", None), ("small", None), ("small3", None), ("S1", (4, 1)), ("S2", (5, 2))]


def bits_equal(got, want, label=""):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), label


def within_one_ulp(got, want):
    """fp32 arrays: |got - want| <= the spacing of the larger magnitude."""
    got, want = got.numpy().astype(np.float32), want.numpy().astype(np.float32)
    return bool((np.abs(got.astype(np.float64) - want.astype(np.float64))
                 <= np.spacing(np.maximum(np.abs(got), np.abs(want))).astype(np.float64)).all())


def assert_generator_equal(h, g, centroids, scales):
    """h: graph_from_meshes(...).graph, g: make_multiscale_mesh's."""
    assert sorted(h.keys()) == sorted(g.keys())
    for k in ("edge_index", "edge_ptr", "node_ptr", "intra_mesh_edge_index", "intra_edge_ptr", "node_BC", "type_BC",
              "temporal_res", "previous_t", "BC", "y"):
        a, b = getattr(h, k), getattr(g, k)
        assert a.dtype == b.dtype and torch.equal(a, b), k
    # only IEEE basic operations in a stated order: exact
    assert torch.equal(h.area, g.area) and torch.equal(h.x[:, 0], g.x[:, 0]), "area"
    assert torch.equal(h.x[:, 1], g.x[:, 1]), "DEM"
    assert torch.equal(h.x[:, 2:], g.x[:, 2:])
    assert torch.equal(h.edge_BC_length, g.edge_BC_length)
    for c, (xy, fn) in zip(centroids, scales):
        bits_equal(c.numpy(), xy[fn].mean(1), "centroid")
    # through sqrt, the one operation not guaranteed correctly rounded on both sides: 1 fp32 ulp
    assert h.edge_attr.shape == g.edge_attr.shape and within_one_ulp(h.edge_attr, g.edge_attr), "edge_attr"


def generator_case(name, shape, seed):
    cfg = mesh_config(name) if shape is None else dict(n_coarse=shape[0], num_scales=shape[1])
    g = make_multiscale_mesh(**cfg, seed=seed, T=6)
    scales, bc_xy, dem = mc.generator_inputs(cfg["n_coarse"], cfg["num_scales"], seed)
    return g, scales, bc_xy, dem


# ----------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("name", list(mc.DUAL_CASES))
def test_restatement_agrees_with_dual_graph(name):
    xy, faces = mc.DUAL_CASES[name]
    ref = mc.dual_ref(xy, faces)
    pairs, boundary = _dual_graph(faces.astype(np.int64))
    bits_equal(ref["edge_index"], pairs.reshape(2, -1).astype(np.int64))
    got = {(min(int(faces[f, k]), int(faces[f, (k + 1) % 3])), max(int(faces[f, k]), int(faces[f, (k + 1) % 3]))): f
           for f, k in ref["boundary"].tolist()}
    assert got == {k: int(v) for k, v in boundary.items()}
    assert ref["edge_index"].shape[1] + ref["boundary"].shape[0] == 3 * len(faces)


def test_restatement_agrees_with_generator():
    g, scales, bc_xy, dem = generator_case("tiny", None, 1)
    ref = mc.graph_ref(scales, bc_xy, dem, T=6, BC=g.BC.numpy())
    for k in mc.GRAPH_ARRAYS:
        bits_equal(ref[k], getattr(g, k).numpy(), k)


# ----------------------------------------------------------------------------- the CPU classes
@pytest.mark.parametrize("name", list(mc.DUAL_CASES))
def test_dual_graph_cpu(name):
    xy, faces = mc.DUAL_CASES[name]
    d, ref = DualGraph(xy, faces), mc.dual_ref(xy, faces)
    for k, v in ref.items():
        bits_equal(getattr(d, k).numpy(), v, k)


def test_dual_graph_empty_cpu():
    d = DualGraph(np.zeros((4, 2)), np.zeros((0, 3), np.int32))
    assert d.num_faces == 0 and d.num_edges == 0 and d.boundary.shape == (0, 2) and d.centroid.shape == (0, 2)


def refusals():
    """name -> (xy, faces, the face the message must name, a word of the message)."""
    xy, faces = rc.squares(3)
    out = {}
    f = faces.copy(); f[7, 2] = f[7, 0]
    out["repeated_vertex"] = (xy, f, 7, "repeats")
    out["zero_area"] = (xy, np.concatenate([faces, [[0, 1, 2]]]).astype(np.int32), len(faces), "area2")  # collinear
    f = faces.copy(); f[9, 1] = len(xy)
    out["index_out_of_range"] = (xy, f, 9, "vertex index")
    f = faces.copy(); f[2, 0] = -1
    out["index_negative"] = (xy, f, 2, "vertex index")
    p = xy.copy(); p[faces[11, 1], 0] = np.nan
    out["nan_coordinate"] = (p, faces, int(np.nonzero((faces == faces[11, 1]).any(1))[0][0]), "not finite")
    p = xy.copy(); p[faces[4, 0], 1] = np.inf
    out["inf_coordinate"] = (p, faces, int(np.nonzero((faces == faces[4, 0]).any(1))[0][0]), "not finite")
    third = np.array([[faces[6, 1], faces[6, 2], len(xy)]], np.int32)   # a third face on an interior edge
    shared = np.nonzero([(len({*faces[6, 1:]} & {*g}) == 2) for g in faces])[0]
    assert len(shared) == 2
    out["edge_three_faces"] = (np.concatenate([xy, [[0.4, 7.0]]]), np.concatenate([faces, third]), int(shared[0]), "more than two")
    txy, tf = rc.tri((0, 1, 2))                                          # a triangle and its mirror image
    out["two_shared_edges"] = (txy, np.concatenate([tf, tf[:, [0, 2, 1]]]), 0, "more than one edge")
    return out


REFUSALS = refusals()


@pytest.mark.parametrize("name", list(REFUSALS))
def test_dual_graph_refusals_cpu(name):
    xy, faces, face, word = REFUSALS[name]
    with pytest.raises(ValueError, match=rf"face {face}: .*{word}"):
        DualGraph(xy, faces)


def test_unused_vertex_must_be_finite_cpu():
    xy, faces = rc.squares(2)
    with pytest.raises(ValueError, match="not finite"):
        DualGraph(np.concatenate([xy, [[np.nan, 0.0]]]), faces)


@pytest.mark.parametrize("name", list(mc.LOCATE_CASES))
def test_locate_cpu(name):
    xy, faces, rows = mc.LOCATE_CASES[name]
    pts = mc.probe_points(xy, faces)
    got = PointLocator(xy, faces, rows).locate(pts)
    assert got.dtype == torch.int32
    bits_equal(got.numpy(), mc.locate_ref(xy, faces, rows, pts), name)


@pytest.mark.parametrize("name", rc.NAMES)
def test_locate_equals_pixel_rows_cpu(name):
    xy, faces, rows, grid = rc.CASES[name]
    px, py = rc.centres(grid)
    pts = np.ascontiguousarray(np.stack([px.ravel(), py.ravel()], 1))
    got = PointLocator(xy, faces, rows).locate(pts).numpy().reshape(px.shape)
    bits_equal(got, rc.reference(name), name)


def test_intra_edges_cpu():
    for name in ("non_nested", "overhang", "childless"):
        scales = mc.GRAPH_CASES[name][0]
        for (fxy, ffn), (cxy, cfn) in zip(scales[:-1], scales[1:]):
            fine = DualGraph(fxy, ffn)
            got = intra_edges(fine, PointLocator(cxy, cfn))
            bits_equal(got.numpy(), mc.intra_ref(fine.centroid.numpy(), cxy, cfn), name)
    g, scales, _, _ = generator_case("small3", None, 0)
    (fxy, ffn), (cxy, cfn) = scales[0], scales[1]
    got = intra_edges(DualGraph(fxy, ffn), PointLocator(cxy, cfn)) + torch.tensor([[int(g.node_ptr[1])], [0]])
    assert torch.equal(got, g.intra_mesh_edge_index[:, :int(g.intra_edge_ptr[1]) - 1])


@pytest.mark.parametrize("name", list(mc.GRAPH_CASES))
def test_graph_cpu_equals_restatement(name):
    scales, bc_xy, dem = mc.GRAPH_CASES[name]
    m = graph_from_meshes(scales, bc_xy, dem, T=6)
    ref = mc.graph_ref(scales, bc_xy, dem, T=6)
    for k in mc.GRAPH_ARRAYS:
        bits_equal(getattr(m.graph, k).numpy(), ref[k], k)
    assert m.bc_face == ref["bc_face"] and m.orphans == ref["orphans"] and m.childless == ref["childless"]
    assert int(m.graph.type_BC) == 2 and m.graph.y.shape == (m.graph.num_nodes, 2, 6)
    E = m.graph.edge_index.shape[1]
    assert m.face_relative_distance.shape == (E, 2) and m.edge_slope.shape == (E,)
    assert bool(torch.isfinite(m.edge_slope).all())


def test_graph_case_properties():
    """What the named cases are there for."""
    m = graph_from_meshes(*mc.GRAPH_CASES["overhang"], T=6)
    assert m.orphans[0] > 0 and m.orphans[-1] == 0
    m = graph_from_meshes(*mc.GRAPH_CASES["childless"], T=6)
    assert m.childless[1] > 0 and m.childless[0] == 0
    m = graph_from_meshes(*mc.GRAPH_CASES["non_nested"], T=6)
    assert m.orphans == [0, 0, 0]
    g = m.graph
    children = np.bincount(g.intra_mesh_edge_index[0].numpy())
    assert len(set(children[children > 0].tolist())) > 2, "children per coarse face vary"


def test_per_scale_dem_and_errors():
    scales, bc_xy, dem = mc.GRAPH_CASES["non_nested"]
    m = graph_from_meshes(scales, bc_xy, dem, T=6)
    per_scale = [mc.dem_of(s, 1) for s in scales]
    h = graph_from_meshes(scales, bc_xy, per_scale, T=6).graph
    lo = min(d.min() for d in per_scale)
    ptr = h.node_ptr.tolist()
    for s, d in enumerate(per_scale):
        bits_equal(h.x[ptr[s]:ptr[s + 1] - 1, 1].numpy(), (d - lo).astype(np.float32))
    assert torch.equal(h.edge_index, m.graph.edge_index)
    with pytest.raises(ValueError, match="one value per finest face"):
        graph_from_meshes(scales, bc_xy, dem[:-1], T=6)
    # a coarse mesh that overhangs the fine one: a childless face with no finer face under its centroid
    s = mc.independent_scales((3, 6), 8)
    big = (s[1][0] * 3.0, s[1][1])
    with pytest.raises(ValueError, match=r"\d+ childless face"):
        graph_from_meshes([s[0], big], (0.0, 520.0), mc.dem_of(s[0], 8), T=6)


def test_gauges_cpu():
    scales, bc_xy, dem = mc.GRAPH_CASES["non_nested"]
    m = graph_from_meshes(scales, bc_xy, dem, T=6)
    pts = np.array([[10.0, 10.0], [500.0, 480.0], [999.0, 3.0]])
    for s in (0, 1):
        z = m.gauges(pts, scale=s)
        want = mc.locate_ref(*scales[s], None, pts).astype(np.int64) + int(m.graph.node_ptr[s])
        assert z.rows.tolist() == want.tolist() and z.ptr.tolist() == [0, 1, 2, 3] and z.num_rows == m.graph.num_nodes
    with pytest.raises(ValueError, match="lie in no cell"):
        m.gauges(np.array([[10.0, 10.0], [-5.0, 10.0]]))


# ----------------------------------------------------------------------------- sensitivity
def test_sensitivity():
    """Every wrong variant of a restatement changes an asserted array on a named case."""
    for v in mc.LOCATE_VARIANTS:
        assert any((mc.locate_ref(xy, f, r, mc.probe_points(xy, f), v) != mc.locate_ref(xy, f, r, mc.probe_points(xy, f))).any()
                   for xy, f, r in (mc.LOCATE_CASES[n] for n in ("hex_fan", "squares5"))), v
    for v in mc.DUAL_VARIANTS:
        a, b = mc.dual_ref(*mc.DUAL_CASES["squares3"], v), mc.dual_ref(*mc.DUAL_CASES["squares3"])
        assert any(a[k].tobytes() != b[k].tobytes() for k in b), v
    scales = mc.GRAPH_CASES["non_nested"][0]
    fine = mc.dual_ref(*scales[0])["centroid"]
    for v in mc.INTRA_VARIANTS:
        assert mc.intra_ref(fine, *scales[1], v).tobytes() != mc.intra_ref(fine, *scales[1]).tobytes(), v
    where = {"bc_not_overridden": "bc_drift"}
    for v in mc.GRAPH_VARIANTS:
        case = mc.GRAPH_CASES[where.get(v, "non_nested")]
        a, b = mc.graph_ref(*case, T=6, variant=v), mc.graph_ref(*case, T=6)
        changed = [k for k in mc.GRAPH_ARRAYS if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
        assert changed, v
    a, b = mc.graph_ref(*mc.GRAPH_CASES["bc_drift"], T=6, variant="bc_not_overridden"), mc.graph_ref(*mc.GRAPH_CASES["bc_drift"], T=6)
    assert a["bc_face"][0] == b["bc_face"][0] and a["bc_face"][1] != b["bc_face"][1]


# ----------------------------------------------------------------------------- the generator
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("name,shape", GENERATOR)
def test_generator_equality_cpu(name, shape, seed):
    g, scales, bc_xy, dem = generator_case(name, shape, seed)
    m = graph_from_meshes(scales, bc_xy, dem, T=6, BC=g.BC)
    assert_generator_equal(m.graph, g, m.centroids, scales)
    assert m.orphans == [0] * len(scales) and m.childless == [0] * len(scales)


# ----------------------------------------------------------------------------- the ABI (host only)
def test_abi_host_side():
    lib = _lib.lib()
    assert lib.msw_struct_size(b"msw_locator_stats") == C.sizeof(_lib.MswLocatorStats) == 48
    assert lib.msw_struct_size(b"msw_mesh_dual_stats") == C.sizeof(_lib.MswMeshDualStats) == 72
    for fn in (locate_launch, mesh_dual_launch):
        assert fn(0) == (0, 64, 0) and fn(1) == (1, 64, 1) and fn(64) == (1, 64, 1) and fn(65) == (2, 64, 1)
        assert fn(4096 * 64) == (4096, 64, 1) and fn(4096 * 64 + 1) == (4096, 64, 2)
        with pytest.raises(_lib.EngineError):
            fn(-1)
    h = C.c_void_p()
    assert lib.msw_locator_create(None, 3, None, None, 1, 0, C.byref(h)) == -1 and not h.value
    assert lib.msw_mesh_dual_create(None, 3, None, 1, 0, None, C.byref(h)) == -1 and not h.value
    assert lib.msw_locate_points(None, None, 1, None, None) == -1
