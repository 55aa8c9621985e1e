"""The yardstick of the zonal statistics (mswegnn.raster.CellPixels, msw_zonal_*): a numpy
restatement of include/mswegnn.h "Zonal statistics" and the named cases.  The reference has no
counterpart.  The restatement needs ``pixel_rows`` alone (tests/raster_cases.py restates that):
lists from a stable argsort, sums with ``math.fsum``, the centre pixel operation for operation in
float64.

Values on a 2^-10 lattice with |v| <= 16 make every float64 sum exact in any order -- at most
22,407 of them below 2^14 lattice units each stay below 2^53 -- so lattice results are compared bit
for bit.  Full-precision data has two yardsticks: ``fsum`` within the derived bound (a float64 sum
of n terms in any order lies within (n - 1) * 2^-53 * sum|v| of the exact sum to first order, so
the float32 mean lies within 1 ulp), and ``kernel_order_sum``, the order include/mswegnn.h
documents, bit for bit.

Each wrong ``variant`` of the restatement must change an asserted value on a named case
(tests/test_zonal.py::test_sensitivity).
"""
import math

import numpy as np

import raster_cases as rc
from mswegnn.mesh import mesh_config, multiscale_geometry

CANARY = np.uint32(rc.CANARY_I.view(np.uint32))
NODATA = np.uint32(rc.NODATA_F)
NEG_ZERO = np.uint32(0x80000000)
SERIAL, WAVE = 32, 64          # include/mswegnn.h: lists up to 32 entries are summed front to back

LIST_VARIANTS = ("drop_last", "mult64", "first64")
CENTRE_VARIANTS = ("floor", "swap_xy", "abs_dy")
REDUCE_VARIANTS = ("nan_counted", "no_offset", "unvalued_written", "fill_never", "fill_always", "minmax_swapped",
                   "zero_tied", "float32")
FRAME_VARIANTS = ("var0", "no_tbegin")


# ----------------------------------------------------------------------------- restatement
def cells_ref(pixel_rows, face_row, variant=None):
    """(face_ptr int32 [nf + 1], pixels int32): face f's list = the pixels p with
    pixel_rows[p] == face_row[f], ascending (a stable argsort keeps them so); empty when
    face_row[f] is -1."""
    rows = np.asarray(pixel_rows, np.int32).reshape(-1)
    face_row = np.asarray(face_row, np.int32)
    order = np.argsort(rows, kind="stable")
    srt = rows[order]
    left = np.searchsorted(srt, face_row, "left").astype(np.int64)
    n = np.searchsorted(srt, face_row, "right").astype(np.int64) - left
    if variant != "unvalued_written":
        n[face_row < 0] = 0
    if variant == "drop_last":
        n = np.maximum(n - 1, 0)
    elif variant == "mult64":
        n = n // 64 * 64
    elif variant == "first64":
        n = np.minimum(n, 64)
    ptr = np.concatenate([[0], np.cumsum(n)])
    src = np.repeat(left - ptr[:-1], n) + np.arange(ptr[-1])
    return ptr.astype(np.int32), order[src].astype(np.int32)


def centre_ref(node_xy, face_nodes, grid, variant=None):
    """centre_pixel int32 [nf]: one float64 operation at a time (numpy rounds each elementwise
    operation on its own), as the header writes them."""
    x0, y0, dx, dy, W, H = grid
    if variant == "abs_dy":
        dy = abs(dy)
    xy = np.asarray(node_xy, np.float64)[np.asarray(face_nodes, np.int64).reshape(-1, 3)]   # [nf, 3, 2]
    cx = ((xy[:, 0, 0] + xy[:, 1, 0]) + xy[:, 2, 0]) / 3.0
    cy = ((xy[:, 0, 1] + xy[:, 1, 1]) + xy[:, 2, 1]) / 3.0
    if variant == "swap_xy":
        cx, cy = cy, cx
    half = 0.0 if variant == "floor" else 0.5
    i = np.floor((cx - x0) / dx + half)
    j = np.floor((cy - y0) / dy + half)
    inside = (i >= 0) & (i < W) & (j >= 0) & (j < H)
    return np.where(inside, np.where(inside, j, 0) * W + np.where(inside, i, 0), -1).astype(np.int32)


def _key(words):
    """IEEE order on non-NaN float32 words as int64 keys, -0.0 below +0.0."""
    b = words.view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7FFFFFFF) - 1)


def _word(key):
    return np.where(key >= 0, key, (-(key + 1)) | 0x80000000).astype(np.uint32)


def kernel_order_sum(v):
    """The float64 sum of a list's values (NaN already replaced by +0.0) in the documented order."""
    v = np.asarray(v, np.float64)
    if len(v) <= SERIAL:
        s = np.float64(0.0)
        for x in v:
            s = s + x
        return s
    part = np.zeros(WAVE, np.float64)
    for t in range(0, len(v), WAVE):
        chunk = v[t:t + WAVE]
        part[:len(chunk)] = part[:len(chunk)] + chunk
    d = WAVE // 2
    while d:
        part = part + part[np.arange(WAVE) ^ d]
        d //= 2
    return part[0]


def reduce_ref(face_ptr, pixels, centre, face_row, layers, row_offset=0, num_rows=None, fill_centre=True,
               nodata=NODATA, init=None, variant=None, sums="fsum"):
    """layers float32 [L, P] -> dict of mean / min / max (uint32 words) and count (int32), each
    [L, num_rows], starting from ``init`` (default: canaries everywhere).  ``sums``: "fsum", "exact"
    (a vectorised float64 sum, for lattice data on large cases, where every order gives the same
    bits) or "kernel" (the documented order)."""
    layers = np.ascontiguousarray(layers, np.float32)
    words = layers.view(np.uint32)
    face_row = np.asarray(face_row, np.int32)
    nl, nf = layers.shape[0], len(face_row)
    if num_rows is None:
        num_rows = row_offset + int(face_row.max(initial=-1)) + 1
    n = np.diff(face_ptr).astype(np.int64)
    full = n > 0
    starts = face_ptr[:-1][full].astype(np.int64)
    pw = words[:, pixels]
    pv = pw.view(np.float32)
    ok = ~np.isnan(pv)
    cnt = np.zeros((nl, nf), np.int64)
    lo, hi = np.zeros((nl, nf), np.int64), np.zeros((nl, nf), np.int64)
    total = np.zeros((nl, nf), np.float64)
    if full.any():
        cnt[:, full] = np.add.reduceat(ok.astype(np.int64), starts, axis=1)
        key = _key(pw)
        if variant == "zero_tied":      # -0.0 and +0.0 compare equal: whichever sign, one key
            key = np.where(pw == NEG_ZERO, 0, key)
        lo[:, full] = np.minimum.reduceat(np.where(ok, key, 1 << 40), starts, axis=1)
        hi[:, full] = np.maximum.reduceat(np.where(ok, key, -(1 << 40)), starts, axis=1)
        clean = np.where(ok, pv, np.float32(0.0))
        if variant == "float32":
            total[:, full] = np.add.reduceat(clean, starts, axis=1, dtype=np.float32)
        elif sums == "exact":
            total[:, full] = 0.0 + np.add.reduceat(clean.astype(np.float64), starts, axis=1)   # S starts from +0.0
        else:
            one = math.fsum if sums == "fsum" else kernel_order_sum
            for f in np.nonzero(full)[0]:
                for l in range(nl):
                    total[l, f] = 0.0 + one(clean[l, face_ptr[f]:face_ptr[f + 1]].astype(np.float64))
    if variant == "nan_counted":
        cnt[:] = n[None]
    if variant == "minmax_swapped":
        lo, hi = hi, lo
    have = cnt > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = (total / cnt).astype(np.float32).view(np.uint32)
    use_centre = (bool(fill_centre) or variant == "fill_always") and variant != "fill_never"
    fill = np.full((nl, nf), nodata, np.uint32)
    if use_centre:
        fill = np.where(centre >= 0, words[:, np.maximum(centre, 0)], fill)
    vals = {"mean": np.where(have, mean, fill), "count": cnt.astype(np.int32),
            "min": np.where(have, _word(lo), fill), "max": np.where(have, _word(hi), fill)}
    out = {}
    written = face_row >= -1 if variant == "unvalued_written" else face_row >= 0
    idx = face_row[written].astype(np.int64) + (0 if variant == "no_offset" else row_offset)
    for k, v in vals.items():
        if init is not None:
            o = np.array(init[k]).view(v.dtype).copy()
        else:
            o = np.full((nl, num_rows), CANARY).view(v.dtype).copy()
        o[:, idx] = v[:, written]
        out[k] = o
    return out


def frames_ref(face_ptr, pixels, centre, face_row, frames, pred, var, t_begin, row_offset=0, fill_centre=True,
               nodata=NODATA, variant=None, sums="fsum"):
    """frames float32 [tc, P] into a copy of pred [N, 2, T] -> its uint32 words."""
    frames = np.ascontiguousarray(frames, np.float32)
    out = np.ascontiguousarray(pred, np.float32).view(np.uint32).copy()
    face_row = np.asarray(face_row, np.int32)
    nf = len(face_row)
    tmp = reduce_ref(face_ptr, pixels, centre, np.arange(nf, dtype=np.int32), frames, 0, nf, fill_centre, nodata,
                     sums=sums)["mean"]
    v = 0 if variant == "var0" else var
    tb = 0 if variant == "no_tbegin" else t_begin
    valued = face_row >= 0
    out[face_row[valued].astype(np.int64) + row_offset, v, tb:tb + frames.shape[0]] = tmp[:, valued].T
    return out


# ----------------------------------------------------------------------------- data
def lattice_layers(L, P, seed):
    """[L, P] float32 on the 2^-10 lattice, |v| <= 16."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-16384, 16385, size=(L, P)).astype(np.float64) / 1024.0).astype(np.float32)


def full_layers(L, P, seed):
    """[L, P] float32 over 60 binades, no zero: float64 sums of them do round."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(1, 4, size=(L, P)) * rng.choice([-1.0, 1.0], size=(L, P)) * 2.0 ** rng.integers(-30, 31, size=(L, P))
    return v.astype(np.float32)


def plant(layers, face_ptr, pixels, seed=0):
    """NaN pixels (with a payload) scattered over every layer; in layer 0 a cell of all NaN, a cell
    of all -0.0 and a cell of +0.0 and -0.0 mixed (the three longest-listed distinct faces with at
    least two pixels, when there are that many) -> (layers, the three faces)."""
    v = layers.copy()
    w = v.view(np.uint32)
    w.reshape(-1)[2::29] = 0x7FC12345
    n = np.diff(face_ptr)
    picks = [int(f) for f in np.argsort(-n, kind="stable")[:3] if n[f] >= 2]
    for f, kind in zip(picks, ("nan", "negzero", "mixed")):
        lst = pixels[face_ptr[f]:face_ptr[f + 1]]
        if kind == "nan":
            w[0, lst] = 0x7FC00001
        elif kind == "negzero":
            w[0, lst] = NEG_ZERO
        else:
            w[0, lst] = np.where(np.arange(len(lst)) % 2 == 0, 0, NEG_ZERO).astype(np.uint32)
    return v, picks


# ----------------------------------------------------------------------------- cases
def grid_of(g):
    return (g.x0, g.y0, g.dx, g.dy, g.width, g.height)


def _named():
    from mswegnn.raster import RasterGrid
    geo = multiscale_geometry(**mesh_config("tiny"), seed=0)
    (fxy, ffaces), (cxy, cfaces) = geo[0], geo[-1]
    c = {}
    c["fine20"] = (fxy, ffaces, None, grid_of(RasterGrid.cover(fxy, 20.0)))
    c["straddle64"] = (fxy, ffaces, None, grid_of(RasterGrid.cover(fxy, 5.0)))
    c["long"] = (cxy, cfaces, None, grid_of(RasterGrid.cover(cxy, 2.5)))
    c["coarse60"] = (fxy, ffaces, None, grid_of(RasterGrid.cover(fxy, 60.0)))
    c["coarse200"] = (fxy, ffaces, None, grid_of(RasterGrid.cover(fxy, 200.0)))
    rows = np.random.default_rng(7).permutation(len(ffaces)).astype(np.int32)
    rows[3::7] = -1
    c["unvalued"] = (fxy, ffaces, rows, grid_of(RasterGrid.cover(fxy, 20.0)))
    c["south_up"] = (fxy, ffaces, None, grid_of(RasterGrid.cover(fxy, 60.0, north_up=False)))
    for name in ("tri_ccw", "hex_vertex_edges", "overlap", "zero_area_first", "novalue_covers", "permuted_rows",
                 "negative_dy", "negative_dx", "outside", "grid_1x1", "huge_tiny_coarse", "huge_tiny_fine"):
        c[name] = rc.CASES[name]
    c["zero_faces"] = (np.array([[0, 0], [1, 0], [0, 1]], np.float64), np.zeros((0, 3), np.int32), None,
                       (0.0, 0.0, 0.25, 0.25, 4, 4))
    return c


CASES = _named()
NAMES = tuple(CASES)
ROW_OFFSET = {"unvalued": 5, "permuted_rows": 2}
# (grid, shortest list, longest list, empty valued faces, pixels outside the mesh); None: not asserted
COUNTS = {"fine20": ((51, 51), 2, 10, 0, None), "straddle64": ((201, 201), 63, 96, 0, None),
          "long": ((401, 401), 17791, 22407, 0, None), "coarse60": ((18, 18), 0, 2, 226, 35),
          "coarse200": ((6, 6), 0, 1, 476, None)}

xy_hex, faces_hex = rc.hex_fan()
SHARED_ROW = (xy_hex, faces_hex, np.array([0, 1, 2, 2, 3, 4], np.int32), (0.0, 0.0, 1.0, 1.0, 9, 9))

_REF = {}


def face_rows(name):
    case = CASES[name]
    return np.arange(len(case[1]), dtype=np.int32) if case[2] is None else np.asarray(case[2], np.int32)


def reference(name):
    """(pixel_rows, face_ptr, pixels, centre_pixel) of a named case, computed once and shared
    (read-only): brute-force location, then the restatement."""
    if name not in _REF:
        case = CASES[name]
        rows = rc.reference(name) if name in rc.CASES else rc.locate_ref(*case)
        fptr, pix = cells_ref(rows, face_rows(name))
        out = (rows, fptr, pix, centre_ref(case[0], case[1], case[3]))
        for a in out:
            a.setflags(write=False)
        _REF[name] = out
    return _REF[name]


# ----------------------------------------------------------------------------- ragged rounds
def strip_case(num_faces, wide_every=4099):
    """A numpy-made strip of ``num_faces`` / 2 cells [X_s, X_s+1] x [0, 1], each cut by the diagonal
    from (X_s+1, 0) to (X_s, 1) into face 2s (below) and 2s + 1 (above); every ``wide_every``-th cell
    and the last are 64 wide (lists of about 128 pixels: the wave's path), the rest 1 wide (lists of 3 and
    1).  Pixels of 0.5 x 0.5 with centres at the quarter points: all coordinates are exact, the
    diagonal passes through pixel centres (ties go to the lower face), and ``pixel_rows`` follows
    from u = (x - X_s) / w + y <= 1.  face_row reverses the faces.
    -> (case, pixel_rows [2, W])."""
    assert num_faces % 2 == 0
    cells = num_faces // 2
    w = np.ones(cells, np.int64)
    w[wide_every - 1::wide_every] = 64
    w[-1] = 64
    X = np.concatenate([[0], np.cumsum(w)]).astype(np.float64)
    xy = np.concatenate([np.stack([X, np.zeros_like(X)], 1), np.stack([X, np.ones_like(X)], 1)])
    s = np.arange(cells)
    top = cells + 1
    faces = np.empty((num_faces, 3), np.int32)
    faces[0::2] = np.stack([s, s + 1, top + s], 1)
    faces[1::2] = np.stack([s + 1, top + s + 1, top + s], 1)
    face_row = np.arange(num_faces, dtype=np.int32)[::-1].copy()
    W = int(2 * X[-1])
    grid = (0.25, 0.25, 0.5, 0.5, W, 2)
    px = 0.25 + 0.5 * np.arange(W)
    cell = np.searchsorted(X, px, "right") - 1
    rows = np.empty((2, W), np.int32)
    for j, y in enumerate((0.25, 0.75)):
        u = (px - X[cell]) / w[cell] + y
        rows[j] = face_row[2 * cell + (u > 1.0)]
    return (xy, faces, face_row, grid), rows


def ragged_faces(grid_cap, faces_per_wg, rounds):
    """A face count that makes ``rounds`` rounds of the reduce loop, the last one ragged in
    workgroups and in faces."""
    return grid_cap * faces_per_wg * (rounds - 1) + 37 * faces_per_wg + 2
