"""The yardstick of the raster products (mswegnn.raster, msw_raster_*): a numpy float64
restatement of include/mswegnn.h "Raster products" -- ``locate_ref`` tries ALL faces at every pixel
(no buckets, no bounding boxes), ``sample_ref`` and ``frames_ref`` gather words -- and the named
cases.  The reference has no counterpart.  Every output is an index decided by fp64 predicates in a
written order or a 32-bit word copied unchanged, so every comparison is bit for bit.

Planted geometry and grids sit on a 2^-10 lattice (2^-12 where a sliver needs it) with small
extents: every edge function at a planted pixel is exact, ties are real zeros.

Each wrong ``variant`` of the restatement must change an asserted value on a named case
(tests/test_raster.py::test_sensitivity).
"""
import numpy as np

from mswegnn.mesh import multiscale_geometry

CANARY_I = np.int32(-1234567)
NODATA_F = 0x7FC00000          # the word of float32 NaN as numpy / torch write it
NODATA_I = 0xFFFFFFFF          # int32 -1

LOCATE_VARIANTS = ("strict", "highest", "keep_zero", "corner", "swap_xy", "abs_dy", "no_face_row")
SAMPLE_VARIANTS = ("no_offset", "nodata0")
FRAME_VARIANTS = ("var0", "no_tbegin", "nodata0")


# ----------------------------------------------------------------------------- restatement
def centres(grid, variant=None):
    x0, y0, dx, dy, W, H = grid
    if variant == "abs_dy":
        dy = abs(dy)
    i, j = np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64)
    if variant == "corner":
        i, j = i - 0.5, j - 0.5
    px, py = x0 + i * dx, y0 + j * dy
    return np.broadcast_to(px[None, :], (H, W)), np.broadcast_to(py[:, None], (H, W))


def edge(xy, u, v, px, py):
    """E(u -> v): from the lower vertex index to the higher, negated when u is the higher."""
    p, q = (u, v) if u < v else (v, u)
    e = (xy[q, 0] - xy[p, 0]) * (py - xy[p, 1]) - (xy[q, 1] - xy[p, 1]) * (px - xy[p, 0])
    return e if u < v else -e


def contains(xy, face, px, py, variant=None):
    a, b, c = (int(v) for v in face)
    area2 = (xy[b, 0] - xy[a, 0]) * (xy[c, 1] - xy[a, 1]) - (xy[b, 1] - xy[a, 1]) * (xy[c, 0] - xy[a, 0])
    if area2 == 0 and variant != "keep_zero":
        return np.zeros(px.shape, bool)
    if not (area2 >= 0 or area2 < 0):
        return np.zeros(px.shape, bool)
    e = [edge(xy, a, b, px, py), edge(xy, b, c, px, py), edge(xy, c, a, px, py)]
    if area2 >= 0:
        return (e[0] > 0) & (e[1] > 0) & (e[2] > 0) if variant == "strict" else (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)
    return (e[0] < 0) & (e[1] < 0) & (e[2] < 0) if variant == "strict" else (e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0)


def locate_ref(node_xy, face_nodes, face_row, grid, variant=None, count=False):
    """pixel_rows [H, W] int32 by brute force; ``count``: also the number of faces holding each pixel."""
    xy = np.asarray(node_xy, np.float64)
    px, py = centres(grid, variant)
    if variant == "swap_xy":
        px, py = py, px
    nf = len(face_nodes)
    rows = np.arange(nf, dtype=np.int32) if face_row is None or variant == "no_face_row" else np.asarray(face_row, np.int32)
    out = np.full(px.shape, -1, np.int32)
    n = np.zeros(px.shape, np.int32)
    order = range(nf) if variant == "highest" else range(nf - 1, -1, -1)  # the last writer wins
    for f in order:
        inside = contains(xy, face_nodes[f], px, py, variant)
        out[inside] = rows[f]
        n += inside
    return (out, n) if count else out


def sample_ref(pixel_rows, layers, row_offset=0, nodata=NODATA_F, variant=None):
    """layers [L, n] (float32 or int32) -> uint32 words [L, H, W]."""
    words = np.ascontiguousarray(layers).view(np.uint32)
    off = 0 if variant == "no_offset" else row_offset
    idx = np.maximum(pixel_rows.astype(np.int64) + off, 0)
    fill = np.uint32(0 if variant == "nodata0" else nodata)
    return np.where(pixel_rows[None] >= 0, words[:, idx], fill).astype(np.uint32)


def frames_ref(pixel_rows, pred, var, t_begin, t_count, row_offset=0, nodata=NODATA_F, variant=None):
    """pred [N, 2, T] float32 -> uint32 words [t_count, H, W]."""
    words = np.ascontiguousarray(pred, np.float32).view(np.uint32)
    v = 0 if variant == "var0" else var
    tb = 0 if variant == "no_tbegin" else t_begin
    idx = np.maximum(pixel_rows.astype(np.int64) + row_offset, 0)
    got = np.moveaxis(words[idx, v, tb:tb + t_count], -1, 0)
    fill = np.uint32(0 if variant == "nodata0" else nodata)
    return np.where(pixel_rows[None] >= 0, got, fill).astype(np.uint32)


# ----------------------------------------------------------------------------- data
def make_layers(L, n, seed, ints=False):
    """[L, n] distinct per (layer, row); floats carry a NaN payload and a -0.0."""
    rng = np.random.default_rng(seed)
    if ints:
        return rng.integers(-2 ** 31, 2 ** 31 - 1, size=(L, n), dtype=np.int64).astype(np.int32)
    v = rng.uniform(-4, 4, size=(L, n)).astype(np.float32)
    w = v.view(np.uint32)
    w.reshape(-1)[0::7] = 0x7FC12345  # a NaN with a payload
    w.reshape(-1)[3::11] = 0x80000000  # -0.0
    return v


def make_pred(N, T, seed):
    v = np.random.default_rng(seed).uniform(-2, 2, size=(N, 2, T)).astype(np.float32)
    w = v.view(np.uint32).reshape(-1)
    w[1::13] = 0x7FC0BEEF
    w[5::17] = 0x80000000
    return v


# ----------------------------------------------------------------------------- planted meshes
def tri(order):
    xy = np.array([[0, 0], [8, 0], [0, 8]], np.float64)
    return xy, np.array([order], np.int32)


def hex_fan(offset=(0.0, 0.0)):
    """6 faces around vertex 0 at (4, 4)."""
    xy = np.array([[4, 4], [8, 4], [6, 8], [2, 8], [0, 4], [2, 0], [6, 0]], np.float64) + np.asarray(offset, np.float64)
    faces = np.array([[0, 1 + k, 1 + (k + 1) % 6] for k in range(6)], np.int32)
    return xy, faces


def squares(n, h=1.0, origin=(0.0, 0.0)):
    """n x n squares of side h, two triangles each, diagonals alternating, both orientations."""
    ii, jj = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    xy = np.stack([ii.ravel() * h + origin[0], jj.ravel() * h + origin[1]], 1).astype(np.float64)
    vid = lambda i, j: i * (n + 1) + j  # noqa: E731
    faces = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = vid(i, j), vid(i + 1, j), vid(i + 1, j + 1), vid(i, j + 1)
            faces += [(a, b, c), (a, d, c)] if (i + j) % 2 == 0 else [(a, b, d), (b, d, c)]
    return xy, np.asarray(faces, np.int32)


def huge_and_tiny():
    """One huge triangle beside 200 tiny ones: long bucket lists, many buckets per face."""
    xy, faces = squares(10, 1.0, origin=(1030.0, 3.0))
    big = np.array([[0, 0], [1024, 0], [0, 1024]], np.float64)
    return np.concatenate([big, xy]), np.concatenate([np.array([[0, 1, 2]], np.int32), faces + 3]).astype(np.int32)


def cover(xy, W, H, north_up=True):
    """A W x H grid over the bounding box of xy, centres on the box's rim."""
    (xlo, ylo), (xhi, yhi) = xy.min(0), xy.max(0)
    dx, dy = (xhi - xlo) / max(W - 1, 1), (yhi - ylo) / max(H - 1, 1)
    return (xlo, yhi, dx, -dy, W, H) if north_up else (xlo, ylo, dx, dy, W, H)


def _cases():
    c = {}
    unit = (0.0, 0.0, 1.0, 1.0, 9, 9)
    c["tri_ccw"] = (*tri((0, 1, 2)), None, (-1.0, -1.0, 0.5, 0.5, 21, 21))
    c["tri_cw"] = (*tri((0, 2, 1)), None, (-1.0, -1.0, 0.5, 0.5, 21, 21))
    # (4, 4): a vertex of 6 faces; (5..7, 4): a shared edge; (7, 6), (3..5, 8): boundary edges
    c["hex_vertex_edges"] = (*hex_fan(), None, unit)
    xy = np.array([[0, 0], [8, 0], [0, 8], [1, 1], [9, 1], [1, 9]], np.float64)
    c["overlap"] = (xy, np.array([[3, 4, 5], [0, 1, 2]], np.int32), np.array([7, 3], np.int32), (0.0, 0.0, 0.5, 0.5, 20, 20))
    xy, faces = squares(4, 2.0)
    zero = np.array([[0, 12, 24]], np.int32)  # (0, 0), (4, 4), (8, 8): collinear, on the diagonal's pixels
    c["zero_area_first"] = (xy, np.concatenate([zero, faces]).astype(np.int32), None, unit)
    xy, faces = hex_fan()
    lid = np.concatenate([xy, [[-2.0, -2.0], [14.0, -2.0], [-2.0, 14.0]]])
    c["novalue_covers"] = (lid, np.concatenate([[[7, 8, 9]], faces]).astype(np.int32),
                           np.array([-1, 0, 1, 2, 3, 4, 5], np.int32), (-3.0, -3.0, 1.0, 1.0, 18, 18))
    c["permuted_rows"] = (xy, faces, np.array([14, 3, 9, 0, 21, 6], np.int32), unit)
    c["negative_dy"] = (xy, faces, None, (0.0, 8.0, 1.0, -1.0, 9, 9))
    c["negative_dx"] = (xy, faces, None, (8.5, 0.25, -0.5, 0.5, 18, 16))
    c["outside"] = (xy, faces, None, (100.0, -50.0, 1.0, 1.0, 12, 5))
    xy, faces = squares(8, 1.0)
    c["window_inside"] = (xy, faces, None, (2.125, 5.875, 0.0625, -0.0625, 40, 30))
    c["far_larger"] = (xy, faces, None, (-60.0, -44.0, 2.5, 2.5, 50, 40))
    for W, H in ((1, 1), (1, 65), (65, 1), (64, 64), (65, 63), (257, 3)):
        c[f"grid_{W}x{H}"] = (xy, faces, None, (0.5 if W == 1 else -0.125, 3.0 if H == 1 else 8.25,
                                                 0.03125 if W == 257 else 0.125, -0.125, W, H))
    xy, faces = huge_and_tiny()
    c["huge_tiny_coarse"] = (xy, faces, None, (-8.0, -8.0, 16.5, 16.5, 65, 64))
    c["huge_tiny_fine"] = (xy, faces, None, (1019.0, 1.75, 0.25, 0.25, 96, 56))
    sliver = np.array([[0, 0], [1024, 0], [512, 2.0 ** -10]], np.float64)  # aspect 2^20 ~ 10^6
    c["sliver"] = (sliver, np.array([[0, 1, 2]], np.int32), None, (-16.0, -2.0 ** -11, 16.0, 2.0 ** -12, 67, 9))
    xy, faces = hex_fan((5e5, 5e6))                                       # UTM-sized coordinates
    c["utm_offset"] = (xy, faces, None, (5e5 - 1.0, 5e6 + 9.0, 0.5, -0.5, 21, 21))
    for seed in (0, 1):
        for s, (xy, faces) in enumerate(multiscale_geometry(3, 4, seed)):
            c[f"generator_seed{seed}_scale{s}"] = (xy, faces, None, cover(xy, 65, 63))
    return c


CASES = _cases()
NAMES = tuple(CASES)
_REF = {}


def reference(name):
    """locate_ref of a named case, computed once and shared (read-only)."""
    if name not in _REF:
        r = locate_ref(*CASES[name])
        r.setflags(write=False)
        _REF[name] = r
    return _REF[name]


def ragged_case(grid_cap, rounds):
    """The hexagon under a grid whose 8 x 8 pixel blocks make ``rounds`` rounds of ``grid_cap``
    workgroups, the last round and both rims ragged."""
    bh = 3
    bw = (grid_cap * (rounds - 1)) // bh + 1
    W, H = 8 * bw - 5, 8 * bh - 1
    xy, faces = hex_fan()
    return (xy, faces, np.array([5, 4, 3, 2, 1, 0], np.int32), (0.0, 0.125, 2.0 ** -12, 0.375, W, H))
