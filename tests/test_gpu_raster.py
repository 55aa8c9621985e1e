"""The raster kernels (msw_raster_create / _sample / _frames) on the GPU against the brute-force
numpy restatement of tests/raster_cases.py -- the reference has no counterpart.  Every output is an
index decided by fp64 predicates in a written order or a 32-bit word copied unchanged, so
everything is compared with ``torch.equal`` on int32 views.  Every output array sits between canary
words, at bases that are and are not 16-byte aligned.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import raster_cases as rc
from conftest import build_msgnn, weights
from mswegnn import _lib
from mswegnn.ensemble import make_ensemble, member_ranges
from mswegnn.floodmaps import flood_maps
from mswegnn.mesh import hydrograph_bc, make_multiscale_mesh, mesh_config, multiscale_geometry
from mswegnn.raster import RasterGrid, Rasterizer, raster_launch

pytestmark = pytest.mark.gpu

PADS = (37, 40)  # canary words on each side: the array's base is not / is 16-byte aligned
INVALID = -1


class Out:
    """An output array of 32-bit words inside a canary-filled allocation."""

    def __init__(self, shape, dev, pad=37):
        size = int(np.prod(shape))
        self.pad = pad
        self.full = torch.full((size + 2 * pad,), int(rc.CANARY_I), device=dev, dtype=torch.int32)
        self.view = self.full[pad:pad + size].view(shape)
        assert self.view.data_ptr() % 16 == (4 * pad) % 16

    @property
    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def check(self, want, label=""):
        c = int(rc.CANARY_I)
        assert bool((self.full[:self.pad] == c).all()) and bool((self.full[self.full.numel() - self.pad:] == c).all()), \
            f"{label}: canary overwritten"
        w = torch.from_numpy(np.ascontiguousarray(want).view(np.int32))
        assert tuple(w.shape) == tuple(self.view.shape) and torch.equal(self.view.cpu(), w), label

    def untouched(self):
        return bool((self.full == int(rc.CANARY_I)).all())


def stream_ptr(stream=None):
    return C.c_void_p(stream if stream is not None else torch.cuda.current_stream().cuda_stream)


def create(case, cuda, **over):
    """msw_raster_create through ctypes -> (return code, handle)."""
    xy, faces, rows, grid = case
    xy = np.ascontiguousarray(xy, np.float64)
    faces = np.ascontiguousarray(faces, np.int32)
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    a = dict(xy=xy.ctypes.data_as(C.POINTER(C.c_double)), V=xy.shape[0], faces=faces.ctypes.data_as(_lib.c_int32_p),
             rows=None if rows is None else rows.ctypes.data_as(_lib.c_int32_p), nf=faces.shape[0],
             grid=C.byref(_lib.MswRasterGrid(*[float(v) for v in grid[:4]], int(grid[4]), int(grid[5]))),
             device=cuda.index or 0, out=True)
    a.update(over)
    h = C.c_void_p()
    code = _lib.lib().msw_raster_create(a["xy"], a["V"], a["faces"], a["rows"], a["nf"], a["grid"], a["device"],
                                        stream_ptr(), C.byref(h) if a["out"] else None)
    return code, h


@contextlib.contextmanager
def handle(case, cuda):
    code, h = create(case, cuda)
    _lib.check(code)
    try:
        yield h
    finally:
        _lib.lib().msw_raster_destroy(h)


def raw_rows(h, grid, cuda):
    """The handle's own pixel_rows array, copied out with the HIP runtime the library links."""
    p = C.c_void_p()
    _lib.check(_lib.lib().msw_raster_pixel_rows(h, C.byref(p)))
    assert p.value
    out = torch.empty((grid[5], grid[4]), dtype=torch.int32, device=cuda)
    copy = _lib.lib().hipMemcpy
    copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert copy(out.data_ptr(), p, out.numel() * 4, 3) == 0   # hipMemcpyDeviceToDevice
    return out.cpu().numpy()


def sample(h, layers, out, row_offset=0, nodata=rc.NODATA_F, L=None, stride=None, num_rows=None, lp=True, op=True, hp=True):
    return _lib.lib().msw_raster_sample(h if hp else None, C.c_void_p(layers.data_ptr()) if lp else None,
                                        layers.shape[0] if L is None else L,
                                        layers.stride(0) if stride is None else stride, row_offset,
                                        layers.shape[1] if num_rows is None else num_rows, nodata,
                                        out.ptr if op else None, stream_ptr())


def frames(h, pred, out, var, t_begin, t_count, row_offset=0, nodata=rc.NODATA_F, N=None, T=None, pp=True, op=True, hp=True):
    return _lib.lib().msw_raster_frames(h if hp else None, C.c_void_p(pred.data_ptr()) if pp else None,
                                        pred.shape[0] if N is None else N, pred.shape[2] if T is None else T, var,
                                        t_begin, t_count, row_offset, nodata, out.ptr if op else None, stream_ptr())


def on_device(host, cuda, shift=0):
    """``host`` on the GPU, its base ``shift`` words past a 16-byte boundary."""
    store = torch.zeros(host.size + 8, device=cuda, dtype=torch.int32)
    dev = store[shift:shift + host.size].view(host.shape)
    dev.copy_(torch.from_numpy(np.ascontiguousarray(host).view(np.int32)))
    assert dev.data_ptr() % 16 == (4 * shift) % 16
    return dev


# ------------------------------------------------------------------ 1. locate
@pytest.mark.parametrize("name", rc.NAMES)
def test_locate_matches_brute_force(cuda, name):
    """Fails on the parent commit: there is no such symbol and no such module."""
    case = rc.CASES[name]
    want = rc.reference(name)
    with handle(case, cuda) as h:
        assert np.array_equal(raw_rows(h, case[3], cuda), want), name
        s = _lib.MswRasterStats()
        _lib.check(_lib.lib().msw_raster_get_stats(h, C.byref(s)))
        assert s.buckets == s.buckets_x * s.buckets_y >= 1 and s.device_bytes >= 4 * want.size
        assert 0 <= s.longest_list <= s.list_entries and s.host_build_seconds >= 0
    r = Rasterizer(case[0], case[1], RasterGrid(*case[3]), face_row=case[2], device=cuda)
    got = r.pixel_rows
    assert got.dtype == torch.int32 and got.device.type == "cuda" and np.array_equal(got.cpu().numpy(), want), name
    r.close()


@pytest.mark.parametrize("rounds", [2, 3])
def test_locate_several_ragged_rounds(cuda, rounds):
    cap, per, one = raster_launch(1 << 20, 8)   # more blocks than the cap: the cap itself
    assert per == 64 and one * cap == (1 << 20) // 8
    case = rc.ragged_case(cap, rounds)
    g, per, it = raster_launch(case[3][4], case[3][5])
    blocks = -(-case[3][4] // 8) * -(-case[3][5] // 8)
    assert (g, it) == (cap, rounds) and blocks % cap != 0 and case[3][4] % 8 and case[3][5] % 8
    want = rc.locate_ref(*case)
    assert (want >= 0).any() and (want < 0).any()
    with handle(case, cuda) as h:
        assert np.array_equal(raw_rows(h, case[3], cuda), want)


# ------------------------------------------------------------------ 2. sample
@pytest.mark.parametrize("name", ["generator_seed0_scale1", "permuted_rows", "novalue_covers"])
def test_sample_layers(cuda, name):
    case = rc.CASES[name]
    rows = rc.reference(name)
    off = 5
    n = int(max(case[2].max() if case[2] is not None else len(case[1]) - 1, 0)) + 1 + off
    with handle(case, cuda) as h:
        for k, (L, ints) in enumerate([(L, ints) for L in (1, 2, 9) for ints in (False, True)]):
            layers = rc.make_layers(L, n, seed=L, ints=ints)
            nodata = rc.NODATA_I if ints else (rc.NODATA_F, 0xC61C3C00)[L == 2]   # NaN, or -9999.0
            want = rc.sample_ref(rows, layers, off, nodata)
            if not ints and name.startswith("generator"):
                assert (want == 0x7FC12345).any() and (want == 0x80000000).any()    # a NaN payload and -0.0 arrive
            out = Out(want.shape, cuda, PADS[k % 2])
            _lib.check(sample(h, on_device(layers, cuda, k % 3), out, off, nodata))
            out.check(want, f"{name} L={L} ints={ints}")


def test_sample_stride_and_ensemble_members(cuda, ensemble):
    """A layer stride larger than the rows addressed, and one handle serving members 0 and 3 of a
    4-member batch through ``row_offset``."""
    xy, faces = multiscale_geometry(**mesh_config("small"))[0]
    case = (xy, faces, None, rc.cover(xy, 61, 47))
    rows = rc.locate_ref(*case)
    ranges = [(int(s), int(e)) for s, e in member_ranges(ensemble)]
    N = int(ensemble.x.shape[0])
    assert len(ranges) == 4 and ranges[0][1] - ranges[0][0] == len(faces) + 1
    with handle(case, cuda) as h:
        wide = rc.make_layers(3, len(faces) + 13, seed=2)
        dev = on_device(wide, cuda)
        out = Out((3,) + rows.shape, cuda, 40)
        _lib.check(sample(h, dev, out, 0, stride=len(faces) + 13, num_rows=len(faces)))
        out.check(rc.sample_ref(rows, wide, 0))
        batch = rc.make_layers(2, N, seed=3)
        dev = on_device(batch, cuda, 1)
        for m in (0, 3):
            out = Out((2,) + rows.shape, cuda)
            _lib.check(sample(h, dev, out, ranges[m][0]))
            out.check(rc.sample_ref(rows, batch, ranges[m][0]), f"member {m}")
        assert not np.array_equal(rc.sample_ref(rows, batch, ranges[0][0]), rc.sample_ref(rows, batch, ranges[3][0]))


# ------------------------------------------------------------------ 3. frames
@pytest.mark.parametrize("T", [1, 5, 16, 17, 48])
def test_frames_windows(cuda, T):
    """T = 16 and 48 from an aligned base with t_begin 0 or 4 take the 16-byte loader, every other
    T, t_begin = 1 and every base shifted by one float the scalar one."""
    name = "generator_seed0_scale2"
    case, rows = rc.CASES[name], rc.reference(name)
    off = 3
    pred = rc.make_pred(len(case[1]) + off, T, seed=T)
    devs = [on_device(pred, cuda, 0), on_device(pred, cuda, 1)]
    k = 0
    with handle(case, cuda) as h:
        for tb in (0, 1, 4):
            for tc in (1, 3, 4, 5, 16, 17):
                if tb + tc > T:
                    continue
                for var, shift in ((0, 0), (1, 0), (k % 2, 1)):
                    want = rc.frames_ref(rows, pred, var, tb, tc, off)
                    out = Out(want.shape, cuda, PADS[k % 2])
                    _lib.check(frames(h, devs[shift], out, var, tb, tc, off))
                    out.check(want, f"T={T} window=({tb}, {tc}) var={var} shift={shift}")
                    k += 1
        if T == 1:
            out = Out((1,) + rows.shape, cuda)
            _lib.check(frames(h, devs[0], out, 1, 0, 1, off, nodata=0x80000000))
            out.check(rc.frames_ref(rows, pred, 1, 0, 1, off, nodata=0x80000000))
    assert k >= 3


# ------------------------------------------------------------------ 4. refusals leave the outputs alone
def test_abi_refusals_keep_the_canaries(cuda):
    lib = _lib.lib()
    case = rc.CASES["permuted_rows"]                      # face rows 0 .. 21
    xy, faces, frow, grid = case
    G = lambda *g: C.byref(_lib.MswRasterGrid(*g))  # noqa: E731
    bad_faces = [np.array([[0, 1, 7]], np.int32), np.array([[0, -1, 2]], np.int32)]
    nan_xy = xy.copy()
    nan_xy[3, 1] = np.nan
    refused = [dict(out=False), dict(xy=None), dict(faces=None), dict(grid=None), dict(V=-1), dict(nf=-1), dict(device=-1),
               dict(grid=G(0, 0, 0.0, 1, 4, 4)), dict(grid=G(0, 0, 1, 0.0, 4, 4)), dict(grid=G(0, 0, 1, 1, 0, 4)),
               dict(grid=G(0, 0, 1, 1, 4, -3)), dict(grid=G(0, 0, 1, 1, 65536, 32768)), dict(grid=G(np.nan, 0, 1, 1, 4, 4)),
               dict(grid=G(0, 0, np.inf, 1, 4, 4)), dict(V=6),
               dict(rows=np.array([0, 1, 2, 3, 4, -2], np.int32).ctypes.data_as(_lib.c_int32_p)),
               dict(xy=nan_xy.ctypes.data_as(C.POINTER(C.c_double)))]
    refused += [dict(faces=f.ctypes.data_as(_lib.c_int32_p), nf=1) for f in bad_faces]
    for kw in refused:
        code, h = create(case, cuda, **kw)
        assert code == INVALID and not h.value and lib.msw_last_error(), kw
    with handle(case, cuda) as h:
        rows = rc.reference("permuted_rows")
        layers, pred = rc.make_layers(2, 30, seed=1), rc.make_pred(30, 8, seed=1)
        dl, dp = on_device(layers, cuda), on_device(pred, cuda)
        out = Out((2,) + rows.shape, cuda)
        for kw in (dict(hp=False), dict(lp=False), dict(op=False), dict(L=-1), dict(stride=-1), dict(num_rows=-1),
                   dict(num_rows=29, row_offset=8), dict(row_offset=9), dict(row_offset=-1), dict(num_rows=21),
                   dict(row_offset=2 ** 62), dict(row_offset=-2 ** 62)):
            assert sample(h, dl, out, **kw) == INVALID and out.untouched(), kw
        assert sample(h, dl, out, L=0) == _lib.MSW_OK and out.untouched()           # no layers: a no-op
        fo = Out((4,) + rows.shape, cuda, 40)
        ok = dict(var=1, t_begin=2, t_count=4)
        for kw in (dict(hp=False), dict(pp=False), dict(op=False), dict(var=2), dict(var=-1), dict(t_begin=-1), dict(t_count=-1),
                   dict(t_begin=5), dict(t_count=7), dict(T=5), dict(T=-1), dict(N=-1), dict(N=21), dict(row_offset=9),
                   dict(row_offset=-1), dict(row_offset=2 ** 62)):
            assert frames(h, dp, fo, **{**ok, **kw}) == INVALID and fo.untouched(), kw
        assert frames(h, dp, fo, **{**ok, "t_count": 0}) == _lib.MSW_OK and fo.untouched()   # an empty window
        assert lib.msw_raster_pixel_rows(None, C.byref(C.c_void_p())) == INVALID
        assert lib.msw_raster_pixel_rows(h, None) == INVALID and lib.msw_raster_get_stats(h, None) == INVALID
        _lib.check(sample(h, dl, out, 8))                                            # the good calls still work
        out.check(rc.sample_ref(rows, layers, 8))
        _lib.check(frames(h, dp, fo, **ok, row_offset=8))
        fo.check(rc.frames_ref(rows, pred, 1, 2, 4, 8))
    assert lib.msw_raster_destroy(None) == _lib.MSW_OK


def test_create_and_destroy_fifty_handles(cuda):
    case = rc.CASES["generator_seed0_scale0"]
    want = rc.reference("generator_seed0_scale0")
    first = None
    for k in range(50):
        r = Rasterizer(case[0], case[1], RasterGrid(*case[3]), device=cuda)
        s = r.stats()
        first = first or s
        assert s["device_bytes"] == first["device_bytes"] > 0 and s["buckets"] == first["buckets"]
        if k in (0, 49):
            assert np.array_equal(r.pixel_rows.cpu().numpy(), want)
        r.close()
        r.close()


# ------------------------------------------------------------------ 5. the engine, end to end
@pytest.fixture(scope="module")
def engine(cuda):
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    m.engine = "hip"
    return m


@pytest.fixture(scope="module")
def ensemble(cuda):
    g = make_multiscale_mesh(**mesh_config("small"), T=48)
    bcs = [hydrograph_bc(48, peak=p, seed=s) for p, s in ((1.0, 1), (3.0, 2), (4.5, 3), (7.0, 4))]
    return make_ensemble(g, bcs).to(cuda)


def _check_maps(got, maps, rows, label):
    """``got`` = Rasterizer.sample(maps) against the restatement applied to the same maps."""
    tensors = {k: v for k, v in maps.items() if isinstance(v, (dict, torch.Tensor))}
    assert got.keys() == tensors.keys(), label
    for k, v in tensors.items():
        if isinstance(v, dict):
            _check_maps(got[k], v, rows, f"{label}.{k}")
            continue
        host = v.cpu().numpy()
        ints = host.dtype.kind == "i"
        host = host.astype(np.int32 if ints else np.float32)
        want = rc.sample_ref(rows, host[None], 0, rc.NODATA_I if ints else rc.NODATA_F)[0]
        assert got[k].dtype == (torch.int32 if ints else torch.float32), f"{label}.{k}"
        assert torch.equal(got[k].view(torch.int32).cpu(), torch.from_numpy(want.view(np.int32))), f"{label}.{k}"


def test_rollout_to_rasters(cuda, engine, ensemble):
    """rollout -> flood_maps -> Rasterizer.sample(result), and one frame window, on the small mesh;
    the raster calls run on a side stream directly behind the rollout, without synchronisation."""
    from mswegnn.engine import plan_for
    xy, faces = multiscale_geometry(**mesh_config("small"))[0]
    grid = RasterGrid.cover(xy, 12.5)
    rows = rc.locate_ref(xy, faces, None, (grid.x0, grid.y0, grid.dx, grid.dy, grid.width, grid.height))
    ranges = [(int(s), int(e)) for s, e in member_ranges(ensemble)]
    plan = plan_for(engine, ensemble)
    whole = plan.rollout(ensemble.x, ensemble.BC, ensemble.node_BC, ensemble.type_BC, 48).clone()
    torch.cuda.synchronize()
    r = Rasterizer(xy, faces, grid, device=cuda)
    assert np.array_equal(r.pixel_rows.cpu().numpy(), rows) and (rows >= 0).all()
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = plan.rollout(ensemble.x, ensemble.BC, ensemble.node_BC, ensemble.type_BC, 48)
        fr = r.frames(out, var=0, t_begin=28, t_count=16, row_offset=ranges[3][0])
        fq = r.frames(out, var=1, t_begin=47, row_offset=ranges[1][0], nodata=-1.0)
        maps = flood_maps(out, ranges=ranges, temporal_res=120)
        rasters = [r.sample(m) for m in maps]
    side.synchronize()
    assert torch.equal(out, whole)
    host = whole.cpu().numpy()
    assert torch.equal(fr.view(torch.int32).cpu(),
                       torch.from_numpy(rc.frames_ref(rows, host, 0, 28, 16, ranges[3][0]).view(np.int32)))
    assert torch.equal(fq.view(torch.int32).cpu(),
                       torch.from_numpy(rc.frames_ref(rows, host, 1, 47, 1, ranges[1][0], 0xBF800000).view(np.int32)))
    assert fr.shape == (16, grid.height, grid.width) and fq.shape == (1, grid.height, grid.width)
    for m, (got, mp) in enumerate(zip(rasters, maps)):
        _check_maps(got, mp, rows, f"member {m}")
    assert not torch.equal(rasters[0]["h_max"], rasters[3]["h_max"])
    r.close()
