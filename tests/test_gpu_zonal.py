"""The zonal kernels (msw_zonal_create / _reduce / _frames) on the GPU against the numpy
restatement of tests/zonal_cases.py -- the reference has no counterpart.  Lists, centre pixels,
counts, extremes and every lattice mean are compared bit for bit; full-precision means bit for bit
against the documented summation order and within 1 ulp of ``fsum``.  Every output array sits
between canary words, at bases that are and are not 16-byte aligned, and starts as canaries, so
an element that must stay untouched shows.
"""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

import zonal_cases as zc
from conftest import build_msgnn, weights
from mswegnn import _lib
from mswegnn.ensemble import make_ensemble, member_ranges
from mswegnn.mesh import hydrograph_bc, make_multiscale_mesh, mesh_config
from mswegnn.raster import RasterGrid, Rasterizer, zonal_launch

rc = zc.rc
pytestmark = pytest.mark.gpu

PADS = (37, 40)  # canary words on each side: the array's base is not / is 16-byte aligned
INVALID, UNSUPPORTED = -1, -3
KEYS = ("mean", "count", "min", "max")


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


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def on_device(host, cuda, shift=0):
    """``host`` on the GPU, its base ``shift`` words past a 16-byte boundary."""
    store = torch.zeros(host.size + 8, device=cuda, dtype=torch.int32)
    dev = store[shift:shift + host.size].view(host.shape)
    dev.copy_(torch.from_numpy(np.ascontiguousarray(host).view(np.int32)))
    assert dev.data_ptr() % 16 == (4 * shift) % 16
    return dev


def raster_create(case, cuda):
    xy, faces, rows, grid = case
    xy = np.ascontiguousarray(xy, np.float64)
    faces = np.ascontiguousarray(faces, np.int32)
    rows = None if rows is None else np.ascontiguousarray(rows, np.int32)
    h = C.c_void_p()
    desc = _lib.MswRasterGrid(*[float(v) for v in grid[:4]], int(grid[4]), int(grid[5]))
    _lib.check(_lib.lib().msw_raster_create(xy.ctypes.data_as(C.POINTER(C.c_double)), xy.shape[0],
                                            faces.ctypes.data_as(_lib.c_int32_p),
                                            None if rows is None else rows.ctypes.data_as(_lib.c_int32_p),
                                            faces.shape[0], C.byref(desc), cuda.index or 0, stream_ptr(), C.byref(h)))
    return h


@contextlib.contextmanager
def handles(case, cuda):
    """(raster handle, zonal handle) through ctypes; the raster handle may be destroyed early."""
    lib = _lib.lib()
    hr = raster_create(case, cuda)
    hz = C.c_void_p()
    try:
        _lib.check(lib.msw_zonal_create(hr, stream_ptr(), C.byref(hz)))
        yield hr, hz
    finally:
        lib.msw_zonal_destroy(hz)
        lib.msw_raster_destroy(hr)


def device_words(ptr, count, cuda):
    """``count`` int32 words at a device pointer, copied out with the HIP runtime the library links."""
    out = torch.empty(count, dtype=torch.int32, device=cuda)
    copy = _lib.lib().hipMemcpy
    copy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    if count:
        assert ptr.value and copy(out.data_ptr(), ptr, count * 4, 3) == 0   # hipMemcpyDeviceToDevice
    torch.cuda.synchronize()
    return out.cpu().numpy()


def lists(hz, nf, cuda):
    p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
    _lib.check(_lib.lib().msw_zonal_lists(hz, *[C.byref(v) for v in p]))
    fptr = device_words(p[0], nf + 1, cuda)
    return fptr, device_words(p[1], int(fptr[-1]), cuda), device_words(p[2], nf, cuda)


def reduce(hz, layers, outs, row_offset=0, fill=1, nodata=zc.NODATA, L=None, stride=None, num_rows=None, out_stride=None,
           lp=True, hp=True):
    """msw_zonal_reduce on layers [L, P] (device) into ``outs``: a dict of Out by name."""
    some = next(iter(outs.values())) if outs else None
    n = some.view.shape[1] if some is not None else 0
    ptr = lambda k: outs[k].ptr if k in outs else None  # noqa: E731
    return _lib.lib().msw_zonal_reduce(hz if hp else None, C.c_void_p(layers.data_ptr()) if lp else None,
                                       layers.shape[0] if L is None else L,
                                       layers.stride(0) if stride is None else stride, row_offset,
                                       n if num_rows is None else num_rows, n if out_stride is None else out_stride,
                                       fill, int(nodata), ptr("mean"), ptr("count"), ptr("min"), ptr("max"), stream_ptr())


def frames(hz, fr, pred, var, t_begin, t_count=None, row_offset=0, fill=1, nodata=zc.NODATA, N=None, T=None, stride=None,
           fp=True, pp=True, hp=True):
    return _lib.lib().msw_zonal_frames(hz if hp else None, C.c_void_p(fr.data_ptr()) if fp else None,
                                       fr.stride(0) if stride is None else stride,
                                       C.c_void_p(pred.data_ptr()) if pp else None, pred.shape[0] if N is None else N,
                                       pred.shape[2] if T is None else T, var, t_begin,
                                       fr.shape[0] if t_count is None else t_count, row_offset, fill, int(nodata),
                                       stream_ptr())


def sums_of(name):
    return "exact" if name == "long" else "fsum"     # lattice data: every order gives fsum's bits


# ------------------------------------------------------------------ 1. lists, centres, reduce
@pytest.mark.parametrize("name", zc.NAMES)
def test_lists_and_reduce(cuda, name):
    """Fails on the parent commit: there are no such symbols."""
    case = zc.CASES[name]
    rows, fptr, pix, centre = zc.reference(name)
    frow = zc.face_rows(name)
    nf, off = len(frow), zc.ROW_OFFSET.get(name, 0)
    num_rows = off + int(frow.max(initial=-1)) + 1 + 3
    host, _ = zc.plant(zc.lattice_layers(5, rows.size, seed=len(name)), fptr, pix)
    want = zc.reduce_ref(fptr, pix, centre, frow, host, off, num_rows, sums=sums_of(name))
    nofill = zc.reduce_ref(fptr, pix, centre, frow, host[:4], off, num_rows, False, 0xC61C3C00, sums=sums_of(name))
    with handles(case, cuda) as (hr, hz):
        got = lists(hz, nf, cuda)
        assert np.array_equal(got[0], fptr) and np.array_equal(got[1], pix) and np.array_equal(got[2], centre), name
        s = _lib.MswZonalStats()
        _lib.check(_lib.lib().msw_zonal_get_stats(hz, C.byref(s)))
        n = np.diff(fptr)
        assert (s.num_faces, s.listed_pixels, s.longest_list) == (nf, len(pix), int(n.max(initial=0))), name
        assert s.empty_faces == int(((n == 0) & (frow >= 0)).sum()) and s.build_us > 0
        assert s.wave_faces == int((n > zc.SERIAL).sum())
        assert s.device_bytes >= 4 * (3 * nf + 1 + len(pix))
        for k, L in enumerate((1, 4, 5)):
            dev = on_device(host[:L], cuda, k % 3)
            outs = {key: Out((L, num_rows), cuda, PADS[(k + j) % 2]) for j, key in enumerate(KEYS)}
            _lib.check(reduce(hz, dev, outs, off))
            for key in KEYS:
                outs[key].check(want[key][:L], f"{name} L={L} {key}")       # L = 1 and L = 5 share layer 0's bits
            first = {key: outs[key].view.clone() for key in KEYS}
            _lib.check(reduce(hz, dev, outs, off))                             # repetition
            assert all(torch.equal(outs[key].view, first[key]) for key in KEYS)
        dev = on_device(host[:4], cuda, 1)
        for j, key in enumerate(KEYS):                                        # each output alone, no fill, -9999.0
            one = {key: Out((4, num_rows), cuda, PADS[j % 2])}
            _lib.check(reduce(hz, dev, one, off, fill=0, nodata=0xC61C3C00))
            one[key].check(nofill[key], f"{name} {key} alone")


@pytest.mark.parametrize("name", ["fine20", "straddle64", "long"])
def test_full_precision_means(cuda, name):
    """Values over 60 binades: the mean equals the documented order's bit for bit, and fsum's
    within 1 ulp (the bound of tests/zonal_cases.py)."""
    rows, fptr, pix, centre = zc.reference(name)
    frow = zc.face_rows(name)
    host = zc.full_layers(2, rows.size, seed=3)
    order = zc.reduce_ref(fptr, pix, centre, frow, host, sums="kernel")["mean"]
    exact = zc.reduce_ref(fptr, pix, centre, frow, host)["mean"]
    with handles(zc.CASES[name], cuda) as (hr, hz):
        out = {"mean": Out(order.shape, cuda)}
        _lib.check(reduce(hz, on_device(host, cuda), out))
        got = out["mean"].view.cpu().numpy()
        ulps = int(np.abs(got.astype(np.int64) - exact.view(np.int32).astype(np.int64)).max())
        print(f"{name}: the mean's worst distance from fsum's is {ulps} ulp")
        assert ulps <= 1
        out["mean"].check(order, name)


# ------------------------------------------------------------------ 2. frames
@pytest.mark.parametrize("T", [1, 5, 16, 17])
def test_frames_windows(cuda, T):
    """Windows at every t_begin and t_count alignment; the rows equal the reduce mean bit for bit
    and nothing else in pred changes."""
    name = "unvalued"
    rows, fptr, pix, centre = zc.reference(name)
    frow, off = zc.face_rows(name), zc.ROW_OFFSET[name]
    N = off + int(frow.max()) + 4
    pred = rc.make_pred(N, T, seed=T)
    stack, _ = zc.plant(zc.lattice_layers(min(T, 9), rows.size, seed=T), fptr, pix)
    dstack = on_device(stack, cuda, 1)
    k = 0
    with handles(zc.CASES[name], cuda) as (hr, hz):
        for tb in (0, 1, 3, 4):
            for tc in (1, 2, 3, 4, 8, 9):
                if tb + tc > T or tc > stack.shape[0]:
                    continue
                var = k % 2
                want = zc.frames_ref(fptr, pix, centre, frow, stack[:tc], pred, var, tb, off)
                out = Out(pred.shape, cuda, PADS[k % 2])
                out.view.copy_(torch.from_numpy(pred.view(np.int32)))
                _lib.check(frames(hz, dstack[:tc], out.view, var, tb, row_offset=off))
                out.check(want, f"T={T} window=({tb}, {tc}) var={var}")
                mean = {"mean": Out((tc, N), cuda)}
                _lib.check(reduce(hz, dstack[:tc], mean, off))
                valued = torch.from_numpy(frow[frow >= 0].astype(np.int64) + off).to(cuda)
                assert torch.equal(out.view[valued, var, tb:tb + tc], mean["mean"].view[:, valued].t())
                k += 1
        if T == 1:                                                            # no fill, a nodata of its own
            want = zc.frames_ref(fptr, pix, centre, frow, stack[:1], pred, 1, 0, off, False, 0x80000000)
            out = Out(pred.shape, cuda)
            out.view.copy_(torch.from_numpy(pred.view(np.int32)))
            _lib.check(frames(hz, dstack[:1], out.view, 1, 0, row_offset=off, fill=0, nodata=0x80000000))
            out.check(want)
            assert (want != zc.frames_ref(fptr, pix, centre, frow, stack[:1], pred, 1, 0, off)).any()
    assert k >= 1


# ------------------------------------------------------------------ 3. several rounds of the reduce loop
@pytest.mark.parametrize("rounds", [2, 3])
def test_several_ragged_rounds(cuda, rounds):
    cap, per, one = zonal_launch(1 << 24)
    assert per == 64 and cap * per * one == 1 << 24
    nf = zc.ragged_faces(cap, per, rounds)
    assert zonal_launch(nf) == (cap, per, rounds)
    case, rows = zc.strip_case(nf)
    frow = case[2]
    fptr, pix = zc.cells_ref(rows, frow)
    centre = zc.centre_ref(case[0], case[1], case[3])
    assert int(np.diff(fptr)[-2:].min()) > 64 > zc.SERIAL                    # the last cell, in the ragged round: the wave's path
    host = zc.lattice_layers(2, rows.size, seed=rounds)
    want = zc.reduce_ref(fptr, pix, centre, frow, host, 3, nf + 5, sums="exact")
    with handles(case, cuda) as (hr, hz):
        p = C.c_void_p()
        _lib.check(_lib.lib().msw_raster_pixel_rows(hr, C.byref(p)))
        assert np.array_equal(device_words(p, rows.size, cuda).reshape(rows.shape), rows)
        got = lists(hz, nf, cuda)
        assert np.array_equal(got[0], fptr) and np.array_equal(got[1], pix) and np.array_equal(got[2], centre)
        outs = {key: Out((2, nf + 5), cuda, PADS[j % 2]) for j, key in enumerate(KEYS)}
        _lib.check(reduce(hz, on_device(host, cuda), outs, 3))
        for key in KEYS:
            outs[key].check(want[key], f"{rounds} rounds {key}")


def test_wave_launch_several_rounds(cuda):
    """More long-listed faces than the cap of workgroups: the wave launch loops, its last round
    ragged (8,600 faces of 128 pixels each, 4,096 workgroups)."""
    cap = zonal_launch(1 << 24)[0]
    nf = 2 * cap + 408
    case, rows = zc.strip_case(nf, wide_every=1)
    frow = case[2]
    fptr, pix = zc.cells_ref(rows, frow)
    centre = zc.centre_ref(case[0], case[1], case[3])
    assert (np.diff(fptr) == 128).all() and nf % cap
    host, _ = zc.plant(zc.lattice_layers(2, rows.size, seed=4), fptr, pix)
    want = zc.reduce_ref(fptr, pix, centre, frow, host, 0, nf, sums="exact")
    with handles(case, cuda) as (hr, hz):
        s = _lib.MswZonalStats()
        _lib.check(_lib.lib().msw_zonal_get_stats(hz, C.byref(s)))
        assert s.wave_faces == nf
        got = lists(hz, nf, cuda)
        assert np.array_equal(got[0], fptr) and np.array_equal(got[1], pix)
        outs = {key: Out((2, nf), cuda, PADS[j % 2]) for j, key in enumerate(KEYS)}
        _lib.check(reduce(hz, on_device(host, cuda), outs))
        for key in KEYS:
            outs[key].check(want[key], key)


# ------------------------------------------------------------------ 4. refusals, lifetimes
def test_abi_refusals_keep_the_canaries(cuda):
    lib = _lib.lib()
    hr = raster_create(zc.SHARED_ROW, cuda)
    hz = C.c_void_p(1)
    assert lib.msw_zonal_create(hr, stream_ptr(), C.byref(hz)) == UNSUPPORTED and not hz.value
    assert b"share" in lib.msw_last_error()
    assert lib.msw_zonal_create(hr, stream_ptr(), None) == INVALID
    assert lib.msw_zonal_create(None, stream_ptr(), C.byref(hz)) == INVALID and not hz.value
    lib.msw_raster_destroy(hr)
    name = "permuted_rows"                                                    # face rows 0 .. 21
    rows, fptr, pix, centre = zc.reference(name)
    frow = zc.face_rows(name)
    host, pred = zc.lattice_layers(2, rows.size, seed=1), rc.make_pred(30, 8, seed=1)
    with handles(zc.CASES[name], cuda) as (hr, hz):
        dl = on_device(host, cuda)
        outs = {key: Out((2, 30), cuda) for key in KEYS}
        for kw in (dict(hp=False), dict(lp=False), dict(L=-1), dict(stride=-1), dict(num_rows=-1), dict(out_stride=-1),
                   dict(row_offset=9), dict(row_offset=-1), dict(num_rows=21), dict(num_rows=29, row_offset=8),
                   dict(row_offset=2 ** 62), dict(row_offset=-2 ** 62)):
            assert reduce(hz, dl, outs, **kw) == INVALID and all(o.untouched() for o in outs.values()), kw
        assert reduce(hz, dl, {}, num_rows=30, out_stride=30) == INVALID          # all four outputs NULL
        assert reduce(hz, dl, outs, L=0) == _lib.MSW_OK and all(o.untouched() for o in outs.values())
        fo = Out(pred.shape, cuda, 40)
        ok = dict(var=1, t_begin=2, t_count=2)
        for kw in (dict(hp=False), dict(fp=False), dict(pp=False), dict(var=2), dict(var=-1), dict(t_begin=-1),
                   dict(t_count=-1), dict(t_begin=7), dict(t_count=7), dict(T=3), dict(T=-1), dict(N=-1), dict(N=21),
                   dict(stride=-1), dict(row_offset=9), dict(row_offset=-1), dict(row_offset=2 ** 62)):
            assert frames(hz, dl, fo.view, **{**ok, **kw}) == INVALID and fo.untouched(), kw
        assert frames(hz, dl, fo.view, **{**ok, "t_count": 0}) == _lib.MSW_OK and fo.untouched()
        assert lib.msw_zonal_lists(hz, None, None, None) == INVALID and lib.msw_zonal_get_stats(hz, None) == INVALID
        _lib.check(reduce(hz, dl, outs, 8))                                    # the good calls still work
        want = zc.reduce_ref(fptr, pix, centre, frow, host, 8, 30)
        for key in KEYS:
            outs[key].check(want[key], key)
    assert lib.msw_zonal_destroy(None) == _lib.MSW_OK


def test_zonal_handle_outlives_the_raster_handle(cuda):
    name = "straddle64"
    rows, fptr, pix, centre = zc.reference(name)
    host = zc.lattice_layers(1, rows.size, seed=9)
    want = zc.reduce_ref(fptr, pix, centre, zc.face_rows(name), host)
    lib = _lib.lib()
    hr = raster_create(zc.CASES[name], cuda)
    hz = C.c_void_p()
    _lib.check(lib.msw_zonal_create(hr, stream_ptr(), C.byref(hz)))
    lib.msw_raster_destroy(hr)
    junk = torch.full((rows.size + 64 * 512,), -7, dtype=torch.int32, device=cuda)   # reuse what the raster handle freed
    outs = {key: Out(want[key].shape, cuda) for key in KEYS}
    _lib.check(reduce(hz, on_device(host, cuda), outs))
    for key in KEYS:
        outs[key].check(want[key], key)
    assert np.array_equal(lists(hz, len(fptr) - 1, cuda)[1], pix)
    lib.msw_zonal_destroy(hz)
    del junk


def test_create_and_destroy_fifty_handles(cuda):
    case = zc.CASES["fine20"]
    r = Rasterizer(case[0], case[1], RasterGrid(*case[3]), device=cuda)
    first = None
    for k in range(50):
        cp = r.cells()
        s = cp.stats()
        first = first or s
        assert s["device_bytes"] == first["device_bytes"] > 0 and s["listed_pixels"] == first["listed_pixels"] == len(zc.reference("fine20")[2])
        if k in (0, 49):
            assert np.array_equal(cp.pixels.cpu().numpy(), zc.reference("fine20")[2])
            assert cp.launch() == (8, 64, 1)
        cp.close()
        cp.close()
    r.close()


# ------------------------------------------------------------------ 5. the engine, end to end
@pytest.fixture(scope="module")
def engine(cuda):
    m = build_msgnn(4, 32, 4, state=weights("K4_F32")).to(cuda)
    m.engine = "hip"
    return m


@pytest.fixture(scope="module")
def ensemble(cuda):
    g = make_multiscale_mesh(**mesh_config("tiny"), T=12)
    bcs = [hydrograph_bc(12, peak=p, seed=s) for p, s in ((1.0, 1), (3.0, 2), (4.5, 3), (7.0, 4))]
    return make_ensemble(g, bcs).to(cuda)


def test_rollout_round_trips(cuda, engine, ensemble):
    """rollout -> Rasterizer.frames -> CellPixels.frames_to_rows on fine20 (every cell holds at
    least 2 pixels) gives the rollout's finest rows back bit for bit -- n copies of a float32 sum
    exactly in float64 and (n v) / n = v; a -0.0 comes back as +0.0, as the header says -- for
    members 0 and 3 of the batch through ``row_offset``, on a side stream directly behind the
    rollout, without synchronisation."""
    from mswegnn.engine import plan_for
    case = zc.CASES["fine20"]
    nf = len(case[1])
    ranges = [(int(s), int(e)) for s, e in member_ranges(ensemble)]
    assert len(ranges) == 4 and ranges[0][1] - ranges[0][0] == nf + 1
    plan = plan_for(engine, ensemble)
    whole = plan.rollout(ensemble.x, ensemble.BC, ensemble.node_BC, ensemble.type_BC, 12).clone()
    torch.cuda.synchronize()
    r = Rasterizer(case[0], case[1], RasterGrid(*case[3]), device=cuda)
    cp = r.cells()
    assert np.array_equal(cp.face_ptr.cpu().numpy(), zc.reference("fine20")[1])
    back = torch.full_like(whole, -5.0)
    side = torch.cuda.Stream(cuda)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        out = plan.rollout(ensemble.x, ensemble.BC, ensemble.node_BC, ensemble.type_BC, 12)
        for m, var, tb, tc in ((0, 0, 0, 12), (3, 0, 2, 9), (3, 1, 4, 8)):
            fr = r.frames(out, var=var, t_begin=tb, t_count=tc, row_offset=ranges[m][0])
            cp.frames_to_rows(fr, back, var=var, t_begin=tb, row_offset=ranges[m][0])
        means = cp.mean(r.frames(out, var=0, t_begin=5, t_count=4, row_offset=ranges[3][0]), ranges[3][0], whole.shape[0])
    side.synchronize()
    assert torch.equal(out, whole)
    want = torch.full_like(whole, -5.0)
    for m, var, tb, tc in ((0, 0, 0, 12), (3, 0, 2, 9), (3, 1, 4, 8)):
        s = ranges[m][0]
        want[s:s + nf, var, tb:tb + tc] = whole[s:s + nf, var, tb:tb + tc] + 0.0       # -0.0 -> +0.0
    assert not torch.isnan(whole).any() and torch.equal(back.view(torch.int32), want.view(torch.int32))
    s = ranges[3][0]
    assert torch.equal(means[:, s:s + nf].view(torch.int32), (whole[s:s + nf, 0, 5:9] + 0.0).t().contiguous().view(torch.int32))
    assert not torch.equal(whole[ranges[0][0]:ranges[0][0] + nf], whole[s:s + nf])
    cp.close()
    r.close()
