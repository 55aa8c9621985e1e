"""The zonal statistics on the CPU: mswegnn.raster.CellPixels' numpy / torch path against the
restatement of tests/zonal_cases.py; the named cases' own counts; the sensitivity of the
restatement; the round trip through Rasterizer.sample; admission errors.  No GPU.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import zonal_cases as zc
from mswegnn import _lib
from mswegnn.raster import CellPixels, RasterGrid, Rasterizer, zonal_launch


def rasterizer(case):
    xy, faces, rows, grid = case
    return Rasterizer(xy, faces, RasterGrid(*grid), face_row=rows)


def words(t):
    return t.contiguous().view(torch.int32).numpy().view(np.uint32)


_CELLS = {}


def cells(name):
    """The CPU CellPixels of a named case, made once."""
    if name not in _CELLS:
        r = rasterizer(zc.CASES[name])
        assert np.array_equal(r.pixel_rows.numpy(), zc.reference(name)[0]), name
        _CELLS[name] = (r, r.cells())
    return _CELLS[name]


def test_named_cases_hold_what_they_name():
    """The counts the cases are named for, so that a fill test cannot pass without empty cells and
    a no-fill test cannot pass with them."""
    for name, (shape, shortest, longest, empty, outside) in zc.COUNTS.items():
        rows, fptr, pix, centre = zc.reference(name)
        n = np.diff(fptr)
        assert rows.shape == shape and (n.min(), n.max()) == (shortest, longest), (name, rows.shape, n.min(), n.max())
        assert int((n == 0).sum()) == empty, (name, int((n == 0).sum()))
        if outside is not None:
            assert int((rows < 0).sum()) == outside, name
        assert (centre >= 0).all(), name      # every centroid of the mesh lies on the covering grid
    assert len(zc.CASES["long"][1]) == 8 and len(zc.CASES["coarse60"][1]) == 512
    n = np.diff(zc.reference("unvalued")[1])
    assert (n[zc.face_rows("unvalued") < 0] == 0).all() and (zc.face_rows("unvalued") < 0).sum() == 73
    assert zc.reference("outside")[2].size == 0 and zc.reference("zero_faces")[1].tolist() == [0]
    assert np.diff(zc.reference("zero_area_first")[1])[0] == 0            # the zero-area face lists nothing
    assert (zc.reference("outside")[3] == -1).all()                       # centroids off the grid


@pytest.mark.parametrize("name", zc.NAMES)
def test_partition(name):
    """The lists together are a permutation of the located pixels; every list ascends strictly."""
    rows, fptr, pix, _ = zc.reference(name)
    assert np.array_equal(np.sort(pix), np.nonzero(rows.reshape(-1) >= 0)[0]), name
    inner = np.ones(len(pix), bool)
    inner[fptr[:-1][fptr[:-1] < len(pix)]] = False                        # a list's first entry
    assert (np.diff(pix.astype(np.int64), prepend=-1)[inner] > 0).all(), name
    frow = zc.face_rows(name)
    for f in range(len(frow)):
        assert (rows.reshape(-1)[pix[fptr[f]:fptr[f + 1]]] == frow[f]).all(), (name, f)


@pytest.mark.parametrize("name", zc.NAMES)
def test_torch_path_matches_the_restatement(name):
    """Fails on the parent commit: Rasterizer has no cells()."""
    r, cp = cells(name)
    rows, fptr, pix, centre = zc.reference(name)
    assert np.array_equal(cp.face_ptr.numpy(), fptr) and np.array_equal(cp.pixels.numpy(), pix), name
    assert np.array_equal(cp.centre_pixel.numpy(), centre) and cp.face_ptr.dtype == torch.int32, name
    s = cp.stats()
    n = np.diff(fptr)
    frow = zc.face_rows(name)
    assert (s["num_faces"], s["listed_pixels"], s["longest_list"]) == (len(frow), len(pix), int(n.max(initial=0)))
    assert s["empty_faces"] == int(((n == 0) & (frow >= 0)).sum()) and s["wave_faces"] == int((n > zc.SERIAL).sum())
    off = zc.ROW_OFFSET.get(name, 0)
    P = rows.size
    num_rows = off + int(frow.max(initial=-1)) + 1 + 3
    layers, _ = zc.plant(zc.lattice_layers(3, P, seed=len(name)), fptr, pix)
    for fill, nodata in ((True, zc.NODATA), (False, np.uint32(0xC61C3C00))):           # NaN, or -9999.0
        want = zc.reduce_ref(fptr, pix, centre, frow, layers, off, num_rows, fill, nodata,
                             sums="exact" if name == "long" else "fsum")
        init = {k: torch.from_numpy(np.full((3, num_rows), zc.CANARY).view(np.int32).copy()) for k in want}
        out = {k: (v if k == "count" else v.view(torch.float32)) for k, v in init.items()}
        got = cp.reduce(torch.from_numpy(layers).view(3, *rows.shape), off, fill_centre=fill,
                        nodata=float(np.array(nodata).view(np.float32)), out=out)
        for k in want:
            assert np.array_equal(words(got[k]), want[k].view(np.uint32)), (name, k, fill)
    fresh = cp.reduce(torch.from_numpy(layers[1]).view(*rows.shape), off, nodata=-1.0)    # [H, W], fresh outputs
    want = zc.reduce_ref(fptr, pix, centre, frow, layers[1:2], off, None, True, np.uint32(0xBF800000),
                         init={k: np.full((1, off + int(frow.max(initial=-1)) + 1), 0 if k == "count" else 0xBF800000,
                                          np.uint32) for k in ("mean", "count", "min", "max")},
                         sums="exact" if name == "long" else "fsum")
    for k in want:
        assert fresh[k].dim() == 1 and np.array_equal(words(fresh[k]), want[k][0].view(np.uint32)), (name, k)
    if frow.max(initial=-1) < 0:
        return
    pred = zc.rc.make_pred(num_rows, 7, seed=3)
    frames = layers[[2, 0]]
    t = torch.from_numpy(pred.copy())
    assert cp.frames_to_rows(torch.from_numpy(frames).view(2, *rows.shape), t, var=1, t_begin=3, row_offset=off) is t
    want = zc.frames_ref(fptr, pix, centre, frow, frames, pred, 1, 3, off, sums="exact" if name == "long" else "fsum")
    assert np.array_equal(words(t), want), name
    mean = cp.mean(torch.from_numpy(frames).view(2, *rows.shape), off, num_rows)
    valued = frow[frow >= 0].astype(np.int64) + off
    assert np.array_equal(words(mean)[:, valued], want[valued, 1, 3:5].T), name       # frames == reduce's mean


def test_planted_cells_are_there():
    """The data holds what the cases name: a cell of all NaN (filled, count 0), of all -0.0 (mean
    +0.0, min = max = -0.0) and of both zeros (min -0.0, max +0.0), and NaN pixels elsewhere."""
    rows, fptr, pix, centre = zc.reference("straddle64")
    layers, (f_nan, f_neg, f_mix) = zc.plant(zc.lattice_layers(2, rows.size, seed=1), fptr, pix)
    got = zc.reduce_ref(fptr, pix, centre, zc.face_rows("straddle64"), layers)
    w = layers.view(np.uint32)
    assert got["count"][0, f_nan] == 0 and got["mean"][0, f_nan] == w[0, centre[f_nan]] == 0x7FC00001
    assert got["mean"][0, f_neg] == 0 and got["min"][0, f_neg] == got["max"][0, f_neg] == zc.NEG_ZERO
    assert got["min"][0, f_mix] == zc.NEG_ZERO and got["max"][0, f_mix] == 0 and got["mean"][0, f_mix] == 0
    n = np.diff(fptr)
    assert ((got["count"][1] < n) & (got["count"][1] > 0)).any()        # NaN pixels skipped in ordinary cells
    nofill = zc.reduce_ref(fptr, pix, centre, zc.face_rows("straddle64"), layers, fill_centre=False)
    assert nofill["mean"][0, f_nan] == nofill["min"][0, f_nan] == zc.NODATA and nofill["count"][0, f_nan] == 0


def test_sensitivity():
    """Each wrong variant of the restatement changes an asserted value on a named case."""
    def outputs(name, variant, fill=True, L=2):
        rows = zc.reference(name)[0]
        case, frow, off = zc.CASES[name], zc.face_rows(name), zc.ROW_OFFSET.get(name, 0)
        fptr, pix = zc.cells_ref(rows, frow, variant)
        centre = zc.centre_ref(case[0], case[1], case[3], variant)
        layers, _ = zc.plant(zc.lattice_layers(L, rows.size, seed=5), *zc.reference(name)[1:3])
        red = zc.reduce_ref(fptr, pix, centre, frow, layers, off, off + int(frow.max()) + 2, fill, variant=variant,
                            sums="exact")
        return [fptr, pix, centre] + [red[k] for k in ("mean", "count", "min", "max")]

    def differs(name, variant, **kw):
        return any(not np.array_equal(a, b) for a, b in zip(outputs(name, variant, **kw), outputs(name, None, **kw)))
    hit = {"drop_last": ("fine20", {}), "mult64": ("straddle64", {}), "first64": ("straddle64", {}),
           "floor": ("fine20", {}), "swap_xy": ("fine20", {}), "abs_dy": ("fine20", {}),
           "nan_counted": ("fine20", {}), "no_offset": ("unvalued", {}), "unvalued_written": ("unvalued", {}),
           "fill_never": ("coarse60", {}), "fill_always": ("coarse60", dict(fill=False)),
           "minmax_swapped": ("fine20", {}), "zero_tied": ("straddle64", {}), "float32": ("long", {})}
    assert set(hit) == set(zc.LIST_VARIANTS + zc.CENTRE_VARIANTS + zc.REDUCE_VARIANTS)
    for variant, (name, kw) in hit.items():
        assert differs(name, variant, **kw), variant
    rows, fptr, pix, centre = zc.reference("unvalued")
    frow = zc.face_rows("unvalued")
    frames, pred = zc.lattice_layers(3, rows.size, seed=2), zc.rc.make_pred(520, 9, seed=2)
    good = zc.frames_ref(fptr, pix, centre, frow, frames, pred, 1, 4, 5)
    for variant in zc.FRAME_VARIANTS:
        assert not np.array_equal(zc.frames_ref(fptr, pix, centre, frow, frames, pred, 1, 4, 5, variant=variant), good)


@pytest.mark.parametrize("name", ["fine20", "straddle64", "long", "coarse60", "unvalued"])
def test_round_trip_through_sample(name):
    """cells.mean(r.sample(v)) == v bit for bit on every cell with count > 0, for arbitrary float32
    v without NaN or -0.0: n copies of a float32 sum exactly in float64, and (n v) / n = v."""
    r, cp = cells(name)
    frow = zc.face_rows(name)
    off = zc.ROW_OFFSET.get(name, 0)
    n = off + int(frow.max()) + 1
    v = torch.from_numpy(zc.full_layers(2, n, seed=11) * np.float32(1e3))
    assert not (v == 0).any()
    got = cp.reduce(r.sample(v, row_offset=off), off, n, fill_centre=False)
    have = got["count"] > 0
    assert torch.equal(got["mean"].view(torch.int32)[have], v.view(torch.int32)[have]), name
    assert torch.equal(got["min"].view(torch.int32)[have], v.view(torch.int32)[have])
    listed = np.diff(zc.reference(name)[1]) > 0
    assert int(have[0].sum()) == int(listed.sum())
    if name in ("fine20", "straddle64", "long"):
        assert bool(have.all()), name


def test_full_precision_within_the_bound():
    """fsum against the documented order of the kernel: |S - fsum| <= (n - 1) 2^-53 sum|v|, and the
    float32 means at most 1 ulp apart; the torch path likewise."""
    worst = 0.0
    for name in ("fine20", "straddle64", "long"):
        rows, fptr, pix, centre = zc.reference(name)
        layers = zc.full_layers(1, rows.size, seed=3)
        for f in range(len(fptr) - 1):
            v = layers[0, pix[fptr[f]:fptr[f + 1]]].astype(np.float64)
            bound = (len(v) - 1) * 2.0 ** -53 * np.abs(v).sum()
            err = abs(zc.kernel_order_sum(v) - math.fsum(v))
            assert err <= bound, (name, f, err, bound)
            worst = max(worst, err / bound)
        exact = zc.reduce_ref(fptr, pix, centre, zc.face_rows(name), layers)["mean"].view(np.int32).astype(np.int64)
        for other in (zc.reduce_ref(fptr, pix, centre, zc.face_rows(name), layers, sums="kernel")["mean"],
                      words(cells(name)[1].mean(torch.from_numpy(layers).view(1, *rows.shape)))):
            assert np.abs(other.view(np.int32).astype(np.int64) - exact).max() <= 1, name
    print(f"worst share of the summation bound: {worst:.3f}")
    assert 0 < worst <= 1


def test_strip_case_is_what_it_says():
    case, rows = zc.strip_case(2 * 4100)
    assert np.array_equal(zc.rc.locate_ref(case[0][:, :], case[1], case[2], case[3])[:, :400], rows[:, :400])
    assert np.array_equal(Rasterizer(case[0], case[1][-400:], RasterGrid(*case[3]), face_row=case[2][-400:])
                          .pixel_rows.numpy()[:, -300:], rows[:, -300:])
    n = np.diff(zc.cells_ref(rows, case[2])[0])
    assert sorted(set(n.tolist())) == [1, 3, 128] and (n == 128).sum() == 4 and (rows >= 0).all()
    for rounds in (2, 3):
        nf = zc.ragged_faces(4096, 64, rounds)
        assert zonal_launch(nf) == (4096, 64, rounds) and nf % 64 and (-(-nf // 64)) % 4096


def test_admission_errors():
    with pytest.raises(ValueError, match="share"):
        rasterizer(zc.SHARED_ROW).cells()
    r, cp = cells("permuted_rows")                        # face rows 0 .. 21
    H, W = r.grid.shape
    layers = torch.zeros(2, H, W)
    assert cp.reduce(layers)["mean"].shape == (2, 22) and cp.mean(layers[0], 2, 30).shape == (30,)
    for off in (-1, 9):
        with pytest.raises(ValueError, match="row_offset"):
            cp.reduce(layers, off, 30)
        with pytest.raises(ValueError, match="row_offset"):
            cp.frames_to_rows(layers, torch.zeros(30, 2, 4), row_offset=off)
    for bad in (torch.zeros(2, H, W + 1), torch.zeros(H * W), "x"):
        with pytest.raises(ValueError):
            cp.reduce(bad)
    for out in ({}, {"median": torch.zeros(2, 22)}, {"mean": torch.zeros(2, 22, dtype=torch.float64)},
                {"count": torch.zeros(2, 22)}, {"mean": torch.zeros(3, 22)}, {"mean": torch.zeros(22)},
                {"mean": torch.zeros(2, 22), "min": torch.zeros(2, 23)}, {"mean": torch.zeros(2, 44)[:, ::2]}):
        with pytest.raises(ValueError):
            cp.reduce(layers, out=out)
    pred = torch.zeros(30, 2, 4)
    for kw in (dict(var=2), dict(t_begin=3), dict(t_begin=-1)):
        with pytest.raises(ValueError):
            cp.frames_to_rows(layers, pred, **kw)
    for bad in (torch.zeros(30, 3, 4), torch.zeros(30, 2, 4, dtype=torch.float64), torch.zeros(30, 2, 8)[:, :, ::2]):
        with pytest.raises(ValueError):
            cp.frames_to_rows(layers, bad)
    assert cp.frames_to_rows(layers[:0], pred) is pred and cp.reduce(layers[:0])["count"].shape == (0, 22)
    assert isinstance(cp, CellPixels)


def test_abi_struct_and_launch():
    lib = _lib.lib()
    assert lib.msw_struct_size(b"msw_zonal_stats") == C.sizeof(_lib.MswZonalStats) == 56
    assert lib.msw_abi_version() == 1
    assert zonal_launch(0) == (0, 64, 0) and zonal_launch(1) == (1, 64, 1) and zonal_launch(65) == (2, 64, 1)
    assert zonal_launch(64 * 4096) == (4096, 64, 1) and zonal_launch(64 * 4096 + 1) == (4096, 64, 2)
    g, p, it = C.c_int32(7), C.c_int32(7), C.c_int32(7)
    assert lib.msw_zonal_launch(-1, C.byref(g), C.byref(p), C.byref(it)) == -1
    assert lib.msw_zonal_launch(4, None, C.byref(p), C.byref(it)) == -1
    assert (g.value, p.value, it.value) == (7, 7, 7) and b"null" in lib.msw_last_error()
    # refusals that need no device: they come before any HIP call
    h = C.c_void_p(1)
    assert lib.msw_zonal_create(None, None, C.byref(h)) == -1 and not h.value
    assert lib.msw_zonal_create(None, None, None) == -1 and lib.msw_zonal_destroy(None) == 0
    assert lib.msw_zonal_reduce(None, None, 1, 0, 0, 0, 0, 1, 0, None, None, None, None, None) == -1
    assert lib.msw_zonal_frames(None, None, 0, None, 0, 0, 0, 0, 0, 0, 1, 0, None) == -1
    assert lib.msw_zonal_lists(None, None, None, None) == -1 and lib.msw_zonal_get_stats(None, None) == -1
