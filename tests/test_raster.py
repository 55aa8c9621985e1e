"""The raster products on the CPU: mswegnn.raster's numpy / torch path against the brute-force
restatement of tests/raster_cases.py, bit for bit; the generator's geometry; coverage along shared
edges; the sensitivity of the restatement; admission errors through the wrapper.  No GPU.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import raster_cases as rc
from mswegnn import _lib
from mswegnn.mesh import make_multiscale_mesh, multiscale_geometry
from mswegnn.raster import RasterGrid, Rasterizer, raster_launch


def rasterizer(name):
    xy, faces, rows, grid = rc.CASES[name]
    return Rasterizer(xy, faces, RasterGrid(*grid), face_row=rows)


def words(t):
    return t.contiguous().view(torch.int32).numpy().view(np.uint32)


@pytest.mark.parametrize("name", rc.NAMES)
def test_torch_path_matches_brute_force(name):
    r = rasterizer(name)
    want = rc.reference(name)
    got = r.pixel_rows
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
    assert np.array_equal(got.numpy(), want), name
    if r.max_row < 0:
        return
    n, off = r.max_row + 1, 5
    for ints in (False, True):
        layers = rc.make_layers(3, n + off, seed=len(name), ints=ints)
        out = r.sample(torch.from_numpy(layers), row_offset=off)
        assert out.dtype == (torch.int32 if ints else torch.float32)
        assert np.array_equal(words(out), rc.sample_ref(want, layers, off, rc.NODATA_I if ints else rc.NODATA_F)), name
    one = r.sample(torch.from_numpy(layers[1]), row_offset=off)
    assert tuple(one.shape) == want.shape and np.array_equal(words(one), rc.sample_ref(want, layers[1:2], off, rc.NODATA_I)[0])
    pred = rc.make_pred(n + off, 7, seed=3)
    fr = r.frames(torch.from_numpy(pred), var=1, t_begin=2, t_count=4, row_offset=off)
    assert np.array_equal(words(fr), rc.frames_ref(want, pred, 1, 2, 4, off)), name


def test_named_cases_hold_what_they_name():
    """The planted ties are there: the restatement's own counts on the named cases."""
    xy, faces, rows, grid = rc.CASES["hex_vertex_edges"]
    got, n = rc.locate_ref(xy, faces, rows, grid, count=True)
    assert n[4, 4] == 6 and got[4, 4] == 0                        # the vertex of 6 faces: the lowest
    assert list(n[4, 5:8]) == [2, 2, 2] and list(got[4, 5:8]) == [0, 0, 0]   # the edge shared by faces 0 and 5
    assert n[6, 7] == 1 and got[6, 7] == 0                        # the boundary edge (8, 4) - (6, 8)
    assert list(n[8, 3:6]) == [1, 1, 1] and n[8, 6] == 2          # the boundary edge y = 8 and its end
    # (0.5, 0.5) lies in face 1 alone, (2, 2) in both: face 0 wins
    assert rc.reference("overlap")[1, 1] == 3 and rc.reference("overlap")[4, 4] == 7
    assert rc.reference("tri_ccw").max() == 0 and np.array_equal(rc.reference("tri_ccw"), rc.reference("tri_cw"))
    assert (rc.reference("outside") == -1).all() and (rc.reference("window_inside") >= 0).all()
    lid = rc.reference("novalue_covers")[3:12, 3:12]             # pixels (x, y) = 0..8: the lid holds x + y <= 12
    x, y = np.meshgrid(np.arange(9), np.arange(9))
    assert (lid[x + y <= 12] == -1).all() and lid[8, 6] == 0 and (lid[x + y > 12] >= 0).sum() == 4
    xy, faces, rows, grid = rc.CASES["sliver"]
    got, n = rc.locate_ref(xy, faces, rows, grid, count=True)
    # rows at y = 0 (the base), 1/4, 1/2, 3/4 of the height and the apex: 1 + 64 (1 - y / height) pixels each
    assert n.sum(1).tolist() == [0, 0, 65, 49, 33, 17, 1, 0, 0] and n.max() == 1
    assert got[2, 1:66].tolist() == [0] * 65 and got[6, 33] == 0


@pytest.mark.parametrize("n_coarse,num_scales,seed", [(3, 4, 0), (2, 3, 5), (5, 2, 11)])
def test_multiscale_geometry_is_the_generators(n_coarse, num_scales, seed):
    g = make_multiscale_mesh(n_coarse, num_scales, seed, T=2)
    geo = multiscale_geometry(n_coarse, num_scales, seed)
    assert len(geo) == num_scales
    ptr = g.node_ptr.tolist()
    for s, (xy, faces) in enumerate(geo):
        assert xy.dtype == np.float64 and faces.dtype == np.int32 and faces.shape[1] == 3
        nf = faces.shape[0]
        assert nf == 2 * n_coarse ** 2 * 4 ** (num_scales - 1 - s) and ptr[s + 1] - ptr[s] == nf + 1
        p0, p1, p2 = xy[faces[:, 0]], xy[faces[:, 1]], xy[faces[:, 2]]
        area = 0.5 * np.abs((p1[:, 0] - p0[:, 0]) * (p2[:, 1] - p0[:, 1]) - (p2[:, 0] - p0[:, 0]) * (p1[:, 1] - p0[:, 1]))
        assert np.array_equal(area.astype(np.float32), g.area[ptr[s]:ptr[s] + nf].numpy()), f"scale {s}"


def test_no_hole_along_interior_edges():
    """Both faces of a shared edge evaluate it from the same end, so no pixel inside the mesh is
    rejected by all faces: 40 seeded grids of 160 x 160 inside the jittered (3, 4, 0) mesh."""
    xy, faces = multiscale_geometry(3, 4, 0)[0]
    uncovered = 0
    for k in range(40):
        rng = np.random.default_rng(k)
        pixel = rng.uniform(0.01, 6.0)
        x0, y0 = rng.uniform(0.0, 1000.0 - 160 * pixel, 2)
        r = Rasterizer(xy, faces, RasterGrid(x0, y0 + 159 * pixel, pixel, -pixel, 160, 160))
        uncovered += int((r.pixel_rows < 0).sum())
    assert uncovered == 0


def test_boundary_aligned_grid_ties():
    """x0 = 0, y0 = 1000, 7.8125 = 1000 / 128: centres on the undeformed rim and on the vertices
    and edges that the jitter leaves in place."""
    xy, faces = multiscale_geometry(3, 4, 0)[0]
    grid = (0.0, 1000.0, 7.8125, -7.8125, 129, 129)
    got, n = rc.locate_ref(xy, faces, None, grid, count=True)
    assert (n >= 1).all()
    assert int((n > 1).sum()) == 172 and int(n.max()) == 6
    px, py = rc.centres(grid)
    tie = n > 1
    holds = np.stack([rc.contains(xy, f, px[tie], py[tie]) for f in faces])   # [nf, 172]
    assert np.array_equal(holds.sum(0), n[tie]) and np.array_equal(holds.argmax(0), got[tie])
    assert np.array_equal(Rasterizer(xy, faces, RasterGrid(*grid)).pixel_rows.numpy(), got)


def test_sensitivity():
    """Each wrong variant of the restatement changes an asserted value on a named case."""
    hit = {"strict": "hex_vertex_edges", "highest": "hex_vertex_edges", "keep_zero": "zero_area_first",
           "corner": "tri_ccw", "swap_xy": "negative_dx", "abs_dy": "negative_dy", "no_face_row": "permuted_rows"}
    assert set(hit) == set(rc.LOCATE_VARIANTS)
    for variant, name in hit.items():
        assert not np.array_equal(rc.locate_ref(*rc.CASES[name], variant=variant), rc.reference(name)), variant
    rows = rc.reference("permuted_rows")
    layers, pred = rc.make_layers(2, 40, seed=1), rc.make_pred(40, 9, seed=2)
    good = rc.sample_ref(rows, layers, 11)
    for variant in rc.SAMPLE_VARIANTS:
        assert not np.array_equal(rc.sample_ref(rows, layers, 11, variant=variant), good), variant
    good = rc.frames_ref(rows, pred, 1, 3, 4, 11)
    for variant in rc.FRAME_VARIANTS:
        assert not np.array_equal(rc.frames_ref(rows, pred, 1, 3, 4, 11, variant=variant), good), variant
    assert not np.array_equal(rc.frames_ref(rows, pred, 1, 3, 4, 0), good)  # row_offset ignored


def test_grid_cover():
    xy = rc.CASES["hex_vertex_edges"][0]
    g = RasterGrid.cover(xy, 0.75)
    px, py = g.centres()
    assert (g.dx, g.dy) == (0.75, -0.75) and px[0] == 0.0 and py[0] == 8.0
    assert px[-1] >= 8.0 > px[-2] and py[-1] <= 0.0 < py[-2]
    g = RasterGrid.cover(xy, 2.0, north_up=False)
    assert (g.x0, g.y0, g.dx, g.dy, g.width, g.height) == (0.0, 0.0, 2.0, 2.0, 5, 5)


def test_admission_errors():
    xy, faces = rc.hex_fan()
    ok = RasterGrid(0.0, 0.0, 1.0, 1.0, 9, 9)
    for bad in ((0, 0, 0.0, 1, 4, 4), (0, 0, 1, 0.0, 4, 4), (0, 0, 1, 1, 0, 4), (0, 0, 1, 1, 4, -1),
                (0, 0, 1, 1, 65536, 32768), (float("nan"), 0, 1, 1, 4, 4), (0, 0, float("inf"), 1, 4, 4)):
        with pytest.raises(ValueError):
            RasterGrid(*bad)
    RasterGrid(0, 0, 1, 1, 65535, 32768)  # 2^31 - 32768 pixels: admitted
    with pytest.raises(ValueError, match="triangles"):
        Rasterizer(xy, np.zeros((2, 4), np.int32), ok)
    for f in (np.array([[0, 1, 7]]), np.array([[0, -1, 2]])):
        with pytest.raises(ValueError, match="vertex index"):
            Rasterizer(xy, f, ok)
    with pytest.raises(ValueError):
        Rasterizer(xy, faces, ok, face_row=np.array([0, 1, 2, 3, 4, -2]))
    with pytest.raises(ValueError):
        Rasterizer(xy, faces, ok, face_row=np.array([0, 1, 2]))
    r = Rasterizer(xy, faces, ok, face_row=np.array([2, 3, 4, 5, 6, 7]))
    layers, pred = torch.zeros(2, 8), torch.zeros(8, 2, 6)
    assert r.sample(layers).shape == (2, 9, 9) and r.sample(layers[:, :6], row_offset=-2).shape == (2, 9, 9)
    for off in (1, -3):
        with pytest.raises(ValueError, match="row_offset"):
            r.sample(layers, row_offset=off)
        with pytest.raises(ValueError, match="row_offset"):
            r.frames(pred, row_offset=off)
    for kw in (dict(var=2), dict(t_begin=-1), dict(t_begin=4, t_count=3), dict(t_count=7)):
        with pytest.raises(ValueError):
            r.frames(pred, **kw)
    with pytest.raises(ValueError):
        r.frames(torch.zeros(8, 3, 6))
    assert r.frames(pred, t_begin=6).shape == (0, 9, 9) and r.sample(torch.zeros(0, 8)).shape == (0, 9, 9)


def test_sample_walks_result_dicts():
    r = rasterizer("permuted_rows")
    n = r.max_row + 1
    maps = {"h_max": torch.arange(n, dtype=torch.float32), "steps": 5,
            "first_wet": {0.05: torch.arange(n, dtype=torch.int32), 0.3: -torch.ones(n, dtype=torch.int64)}}
    out = r.sample(maps, nodata=-9999.0)
    rows = torch.from_numpy(rc.reference("permuted_rows").copy())
    assert set(out) == {"h_max", "first_wet"} and set(out["first_wet"]) == {0.05, 0.3}
    assert torch.equal(out["h_max"], torch.where(rows >= 0, rows.float(), torch.tensor(-9999.0)))
    assert out["first_wet"][0.05].dtype == torch.int32 and torch.equal(out["first_wet"][0.05], rows)
    assert torch.equal(out["first_wet"][0.3], torch.full_like(rows, -1))


def test_abi_structs_and_launch():
    lib = _lib.lib()
    assert lib.msw_struct_size(b"msw_raster_grid") == C.sizeof(_lib.MswRasterGrid) == 40
    assert lib.msw_struct_size(b"msw_raster_stats") == C.sizeof(_lib.MswRasterStats) == 56
    assert lib.msw_abi_version() == 1
    assert raster_launch(1, 1) == (1, 64, 1) and raster_launch(9, 8) == (2, 64, 1)
    assert raster_launch(8 * 4096, 8) == (4096, 64, 1) and raster_launch(8 * 4096 + 1, 8) == (4096, 64, 2)
    for name in ("ragged2", "ragged3"):
        grid = rc.ragged_case(4096, int(name[-1]))[3]
        assert raster_launch(grid[4], grid[5]) == (4096, 64, int(name[-1]))
    g, p, it = C.c_int32(7), C.c_int32(7), C.c_int32(7)
    for w, h in ((0, 4), (4, 0), (-1, 4), (65536, 32768)):
        assert lib.msw_raster_launch(w, h, C.byref(g), C.byref(p), C.byref(it)) == -1
    assert lib.msw_raster_launch(4, 4, None, C.byref(p), C.byref(it)) == -1
    assert (g.value, p.value, it.value) == (7, 7, 7) and b"null" in lib.msw_last_error()
