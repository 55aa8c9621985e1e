"""Raster products (C ABI ``msw_raster_*``): per-cell maps and rollout frames on a regular grid.

Everything else this package makes on the device lives on the mesh: the flood maps
(``mswegnn.floodmaps``), the zone series (``mswegnn.series``), the ensemble products and scores
(``mswegnn.ensemble``) and the ``[N, 2, T]`` rollout itself.  GIS layers, warning systems and web
viewers take regular rasters.  A :class:`Rasterizer` locates every pixel centre of a
:class:`RasterGrid` in the triangles of ONE mesh scale once (a HIP kernel over a host-built bucket
grid) and keeps ``pixel_rows`` [H, W], the graph row of the cell under each pixel or -1; every
product after that is a gather through it: :meth:`Rasterizer.sample` for maps (a tensor, or the
dict ``FloodMaps.result()`` returns), :meth:`Rasterizer.frames` for a window of a rollout.  The
reference resamples on the host with a plotting library (``plot_faces``); it has no numerical
counterpart, and there is nothing to tolerate: an output is an index decided by fp64 predicates in
a written order (include/mswegnn.h, "Raster products") or a 32-bit word copied unchanged.

The containing cell's value is the product -- cell values are finite-volume means, so there is no
interpolation, no supersampling and no area coverage; triangles only; no file formats or coordinate
reference systems; masking dry pixels is one ``torch.where`` on the raster.

The other way -- a DEM, a roughness layer, an observed depth raster, the frame stack of a raster
model onto the cells -- is :meth:`Rasterizer.cells`: a :class:`CellPixels` holds, for every face,
the pixels whose centre it contains (C ABI ``msw_zonal_*``, the transpose of ``pixel_rows``) and
reduces rasters over them: :meth:`CellPixels.reduce` (mean, count, min, max per cell, the mean from
a float64 sum in an order that depends on the cell's list alone) and
:meth:`CellPixels.frames_to_rows`, the exact inverse of :meth:`Rasterizer.frames`.

On CPU tensors the same interface runs :func:`_locate_torch` / :func:`_sample_torch` /
:func:`_frames_torch` / :func:`_cells_torch` / :func:`_reduce_torch`, plain numpy / torch
restatements.
"""
from __future__ import annotations

import ctypes as C
import math
import struct

import numpy as np
import torch

from . import _lib as L

__all__ = ["RasterGrid", "Rasterizer", "CellPixels", "raster_launch", "zonal_launch"]

_MAX_PIXELS = 2 ** 31 - 1


class RasterGrid:
    """``width`` x ``height`` pixels; pixel (i, j) has the centre ``(x0 + i * dx, y0 + j * dy)``
    and is element ``[j, i]`` of a raster.  ``dx`` and ``dy`` are non-zero and may be negative
    (``dy < 0``: north-up)."""

    def __init__(self, x0, y0, dx, dy, width, height):
        self.x0, self.y0, self.dx, self.dy = float(x0), float(y0), float(dx), float(dy)
        self.width, self.height = int(width), int(height)
        if not all(math.isfinite(v) for v in (self.x0, self.y0, self.dx, self.dy)):
            raise ValueError("grid origin and pixel size must be finite")
        if self.dx == 0.0 or self.dy == 0.0:
            raise ValueError("pixel size zero")
        if self.width < 1 or self.height < 1:
            raise ValueError("width and height must be at least 1")
        if self.width * self.height > _MAX_PIXELS:
            raise ValueError("width * height exceeds 2^31 - 1")
        px, py = self.centres()
        if not (np.isfinite(px[-1]) and np.isfinite(py[-1])):
            raise ValueError("pixel centres must be finite")

    @classmethod
    def cover(cls, node_xy, pixel, north_up=True):
        """The smallest grid of square pixels of size ``pixel`` whose centres cover the bounding
        box of ``node_xy``: the first centre on its west (and north, or south) side, the last at or
        past the opposite side."""
        xy = np.asarray(node_xy, dtype=np.float64).reshape(-1, 2)
        pixel = float(pixel)
        if not pixel > 0 or xy.shape[0] == 0:
            raise ValueError("pixel size must be positive and the mesh not empty")
        (xlo, ylo), (xhi, yhi) = xy.min(0), xy.max(0)
        w = int(math.ceil((xhi - xlo) / pixel)) + 1
        h = int(math.ceil((yhi - ylo) / pixel)) + 1
        while w > 1 and xlo + (w - 2) * pixel >= xhi:
            w -= 1
        while xlo + (w - 1) * pixel < xhi:
            w += 1
        if north_up:
            while h > 1 and yhi + (h - 2) * -pixel <= ylo:
                h -= 1
            while yhi + (h - 1) * -pixel > ylo:
                h += 1
            return cls(xlo, yhi, pixel, -pixel, w, h)
        while h > 1 and ylo + (h - 2) * pixel >= yhi:
            h -= 1
        while ylo + (h - 1) * pixel < yhi:
            h += 1
        return cls(xlo, ylo, pixel, pixel, w, h)

    @property
    def shape(self):
        return self.height, self.width

    def centres(self):
        """``(px [W], py [H])`` float64: one multiply and one add each."""
        return (self.x0 + np.arange(self.width, dtype=np.float64) * self.dx,
                self.y0 + np.arange(self.height, dtype=np.float64) * self.dy)

    def desc(self):
        return L.MswRasterGrid(self.x0, self.y0, self.dx, self.dy, self.width, self.height)

    def __repr__(self):
        return f"RasterGrid({self.x0}, {self.y0}, {self.dx}, {self.dy}, {self.width}, {self.height})"


def raster_launch(width, height):
    """``(grid, pixels_per_wg, iters)`` of the locate kernel for a ``width`` x ``height`` grid
    (host only)."""
    g, p, it = C.c_int32(), C.c_int32(), C.c_int32()
    L.check(L.lib().msw_raster_launch(int(width), int(height), C.byref(g), C.byref(p), C.byref(it)))
    return g.value, p.value, it.value


def _bits(value):
    """The 32-bit word of a float32 ``value`` as an unsigned int."""
    return struct.unpack("<I", struct.pack("<f", float(value)))[0]


def _signed(word):
    return word - (1 << 32) if word >= 1 << 31 else word


def _edge(u, v, neg, px, py):
    """E(u -> v) at the pixels; ``neg``: u is not the lower vertex index (the edge is taken from
    v and the result negated).  u, v: (x, y) float64 scalars; px, py broadcastable arrays."""
    p, q = (v, u) if neg else (u, v)
    e = (q[0] - p[0]) * (py - p[1]) - (q[1] - p[1]) * (px - p[0])
    return -e if neg else e


def _locate_torch(node_xy, face_nodes, face_row, grid):
    """``pixel_rows`` [H, W] int32 of ``grid`` over the triangles, in numpy float64: the faces in
    descending order, each over the pixels near its bounding box, a later (lower) face overwriting
    an earlier one -- the lowest containing face wins, also when its ``face_row`` is -1."""
    px, py = grid.centres()
    rows = np.full(grid.shape, -1, dtype=np.int32)
    xy = np.asarray(node_xy, dtype=np.float64)
    for f in range(face_nodes.shape[0] - 1, -1, -1):
        ia, ib, ic = (int(v) for v in face_nodes[f])
        a, b, c = xy[ia], xy[ib], xy[ic]
        area2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if not (area2 > 0 or area2 < 0):
            continue
        xlo, xhi = min(a[0], b[0], c[0]), max(a[0], b[0], c[0])
        ylo, yhi = min(a[1], b[1], c[1]), max(a[1], b[1], c[1])
        d = max(xhi - xlo, yhi - ylo)
        m = 2.0 ** -40 * d * (d * d / abs(area2))  # the kernel's margin (csrc/raster.hip face_margin)
        m = m if m <= d else d
        ii = np.nonzero((px >= xlo - m) & (px <= xhi + m))[0]
        jj = np.nonzero((py >= ylo - m) & (py <= yhi + m))[0]
        if not len(ii) or not len(jj):
            continue
        si, sj = slice(ii[0], ii[-1] + 1), slice(jj[0], jj[-1] + 1)  # centres are monotone in i and j
        qx, qy = px[si][None, :], py[sj][:, None]
        e0, e1, e2 = _edge(a, b, ia > ib, qx, qy), _edge(b, c, ib > ic, qx, qy), _edge(c, a, ic > ia, qx, qy)
        if area2 > 0:
            inside = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
        else:
            inside = (e0 <= 0) & (e1 <= 0) & (e2 <= 0)
        rows[sj, si][inside] = face_row[f]
    return torch.from_numpy(rows)


def _sample_torch(pixel_rows, layers, row_offset, nodata_word):
    """``out[l, j, i]`` = the word ``layers[l, row_offset + pixel_rows[j, i]]`` or ``nodata_word``
    (a signed int32) from plain torch ops on the int32 view: bits are copied."""
    words = layers.view(torch.int32)
    hit = pixel_rows >= 0
    idx = (pixel_rows.long() + row_offset).clamp(min=0)
    out = torch.where(hit, words[:, idx], torch.full((), nodata_word, dtype=torch.int32, device=words.device))
    return out.view(layers.dtype)


def _frames_torch(pixel_rows, pred, var, t_begin, t_count, row_offset, nodata_word):
    """``out[k, j, i] = pred[row_offset + pixel_rows[j, i], var, t_begin + k]`` or the nodata word."""
    words = pred.view(torch.int32)[:, var, t_begin:t_begin + t_count]             # [N, tc]
    hit = pixel_rows >= 0
    idx = (pixel_rows.long() + row_offset).clamp(min=0)
    out = torch.where(hit[None], words[idx].permute(2, 0, 1),
                      torch.full((), nodata_word, dtype=torch.int32, device=words.device))
    return out.contiguous().view(torch.float32)


class Rasterizer:
    """``grid`` located in the triangles ``face_nodes`` [nf, 3] over ``node_xy`` [V, 2] of one mesh
    scale (``mswegnn.mesh.multiscale_geometry`` gives the generator's).  ``face_row`` [nf]: the
    graph row holding face f's value (default f; -1: no value, the face still covers its pixels).
    ``device``: a GPU runs the HIP kernels, ``"cpu"`` the restatements."""

    def __init__(self, node_xy, face_nodes, grid, face_row=None, device="cpu", stream=None):
        if not isinstance(grid, RasterGrid):
            grid = RasterGrid(*grid)
        xy = np.ascontiguousarray(torch.as_tensor(node_xy).cpu().numpy() if torch.is_tensor(node_xy) else node_xy,
                                  dtype=np.float64)
        fn = np.asarray(face_nodes.cpu().numpy() if torch.is_tensor(face_nodes) else face_nodes)
        if xy.ndim != 2 or xy.shape[1] != 2:
            raise ValueError("node_xy must be [V, 2]")
        if fn.ndim != 2 or fn.shape[1] != 3:
            raise ValueError("faces are triangles: face_nodes must be [nf, 3]")
        if not np.isfinite(xy).all():
            raise ValueError("node coordinates must be finite")
        if fn.size and (fn.min() < 0 or fn.max() >= xy.shape[0]):
            raise ValueError("vertex index outside [0, V)")
        fn = np.ascontiguousarray(fn, dtype=np.int32)
        nf = fn.shape[0]
        if face_row is None:
            fr = np.arange(nf, dtype=np.int32)
        else:
            fr = np.asarray(face_row.cpu().numpy() if torch.is_tensor(face_row) else face_row).reshape(-1)
            if fr.shape[0] != nf:
                raise ValueError("face_row must hold one row per face")
            if fr.size and (fr.min() < -1 or fr.max() > _MAX_PIXELS):
                raise ValueError("face_row must be -1 or a row index")
            fr = np.ascontiguousarray(fr, dtype=np.int32)
        valued = fr[fr >= 0]
        self.min_row = int(valued.min()) if valued.size else 0
        self.max_row = int(valued.max()) if valued.size else -1
        self.grid, self.device = grid, torch.device(device)
        self.num_faces = nf
        self._geometry = (xy, fn, fr)  # what cells() needs: the centre pixels, the rows of the faces
        self._handle, self._rows = None, None
        if self.device.type == "cuda":
            index = torch.cuda.current_device() if self.device.index is None else self.device.index
            self.device = torch.device("cuda", index)
            out = C.c_void_p()
            desc = grid.desc()
            L.check(L.lib().msw_raster_create(xy.ctypes.data_as(C.POINTER(C.c_double)), xy.shape[0],
                                              fn.ctypes.data_as(L.c_int32_p), fr.ctypes.data_as(L.c_int32_p), nf,
                                              C.byref(desc), index, self._stream(stream), C.byref(out)))
            self._handle = out
        else:
            self._rows = _locate_torch(xy, fn, fr, grid)

    def _stream(self, stream):
        return C.c_void_p(stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream)

    # ------------------------------------------------------------------ products
    @property
    def pixel_rows(self):
        """[H, W] int32: the graph row of the face under each pixel centre, -1 where there is none
        (on a GPU a copy of the handle's array, made on first use)."""
        if self._rows is None:
            if self._handle is None:
                raise RuntimeError("the rasterizer is closed")
            if self.max_row < 0:
                self._rows = torch.full(self.grid.shape, -1, dtype=torch.int32, device=self.device)
            else:  # the identity map sampled with nodata -1 is pixel_rows itself
                ident = torch.arange(self.max_row + 1, dtype=torch.int32, device=self.device)
                self._rows = self._sample(ident[None], 0, 0xFFFFFFFF, None)[0]
        return self._rows

    def _check_rows(self, row_offset, num_rows):
        if self.max_row >= 0 and not (row_offset + self.min_row >= 0 and row_offset + self.max_row < num_rows):
            raise ValueError(f"row_offset {row_offset} + face rows [{self.min_row}, {self.max_row}] lie outside "
                             f"the {num_rows} rows given")

    def _sample(self, layers, row_offset, nodata_word, stream):
        """layers [L, n] float32 / int32 on this device, stride 1 along n -> [L, H, W]."""
        self._check_rows(row_offset, layers.shape[1])
        if layers.device != self.device:
            raise ValueError(f"layers are on {layers.device}, the rasterizer on {self.device}")
        H, W = self.grid.shape
        if self._handle is None:
            return _sample_torch(self._rows, layers, row_offset, _signed(nodata_word))
        if layers.shape[1] > 1 and layers.stride(1) != 1 or layers.shape[0] > 1 and layers.stride(0) < 0:
            layers = layers.contiguous()
        out = torch.empty((layers.shape[0], H, W), dtype=layers.dtype, device=self.device)
        stride = layers.stride(0) if layers.shape[0] > 1 else layers.shape[1]
        L.check(L.lib().msw_raster_sample(self._handle, C.c_void_p(layers.data_ptr()), layers.shape[0], stride,
                                          row_offset, layers.shape[1], nodata_word, C.c_void_p(out.data_ptr()),
                                          self._stream(stream)))
        return out

    def sample(self, layers, row_offset=0, nodata=float("nan"), nodata_int=-1, stream=None):
        """Per-cell maps -> rasters.  ``layers``: a tensor ``[n]`` -> ``[H, W]`` or ``[L, n]`` ->
        ``[L, H, W]`` whose element ``row_offset + face_row[f]`` is face f's value, or a dict of
        such (``FloodMaps.result()``, per-threshold dicts walked; entries that are neither tensors
        nor dicts are left out).  Floating maps give float32 rasters with ``nodata`` where no cell
        lies under the pixel, integer maps int32 rasters with ``nodata_int``; the values are copied
        as bits."""
        if isinstance(layers, dict):
            return {k: self.sample(v, row_offset, nodata, nodata_int, stream) for k, v in layers.items()
                    if isinstance(v, dict) or torch.is_tensor(v)}
        if not torch.is_tensor(layers) or layers.dim() not in (1, 2):
            raise ValueError("layers must be a tensor [n] or [L, n], or a dict of such")
        if layers.is_floating_point():
            v, word = layers if layers.dtype == torch.float32 else layers.float(), _bits(nodata)
        else:
            v, word = layers if layers.dtype == torch.int32 else layers.to(torch.int32), int(nodata_int) & 0xFFFFFFFF
        if v.shape[0] == 0 and v.dim() == 2:
            return torch.empty((0,) + self.grid.shape, dtype=v.dtype, device=self.device)
        out = self._sample(v if v.dim() == 2 else v[None], int(row_offset), word, stream)
        return out if layers.dim() == 2 else out[0]

    def frames(self, pred, var=0, t_begin=0, t_count=None, row_offset=0, nodata=float("nan"), stream=None):
        """Steps ``t_begin .. t_begin + t_count - 1`` of ``pred`` [N, 2, T] (``var`` 0: depth, 1:
        discharge) as frames ``[t_count, H, W]`` float32."""
        if pred.dim() != 3 or pred.shape[1] != 2:
            raise ValueError("pred must be [N, 2, T]")
        if var not in (0, 1):
            raise ValueError("var is 0 (depth) or 1 (discharge)")
        N, T = int(pred.shape[0]), int(pred.shape[2])
        t_begin = int(t_begin)
        t_count = T - t_begin if t_count is None else int(t_count)
        if t_begin < 0 or t_count < 0 or t_begin + t_count > T:
            raise ValueError(f"steps [{t_begin}, {t_begin + t_count}) lie outside the rollout's {T}")
        row_offset = int(row_offset)
        self._check_rows(row_offset, N)
        if pred.device != self.device:
            raise ValueError(f"pred is on {pred.device}, the rasterizer on {self.device}")
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            pred = pred.float().contiguous()
        H, W = self.grid.shape
        if self._handle is None:
            return _frames_torch(self._rows, pred, var, t_begin, t_count, row_offset, _signed(_bits(nodata)))
        out = torch.empty((t_count, H, W), dtype=torch.float32, device=self.device)
        if t_count:
            L.check(L.lib().msw_raster_frames(self._handle, C.c_void_p(pred.data_ptr()), N, T, var, t_begin, t_count,
                                              row_offset, _bits(nodata), C.c_void_p(out.data_ptr()),
                                              self._stream(stream)))
        return out

    def cells(self, stream=None):
        """The transpose of ``pixel_rows``: a :class:`CellPixels` with every face's pixel list, for
        reducing rasters onto the cells.  It copies what it needs and outlives this rasterizer."""
        if self._handle is None and self._rows is None:
            raise RuntimeError("the rasterizer is closed")
        return CellPixels(self, stream)

    # ------------------------------------------------------------------ bookkeeping
    def launch(self):
        """``(grid, pixels_per_wg, iters)`` of the locate kernel for this grid."""
        return raster_launch(self.grid.width, self.grid.height)

    def stats(self):
        """The bucket grid and its cost: ``buckets``, ``buckets_x``, ``buckets_y``,
        ``list_entries``, ``longest_list``, ``device_bytes``, ``host_build_seconds``, ``locate_us``
        (zeros on the CPU, where there is no bucket grid)."""
        s = L.MswRasterStats()
        if self._handle is not None:
            L.check(L.lib().msw_raster_get_stats(self._handle, C.byref(s)))
        return {k: getattr(s, k) for k, _ in L.MswRasterStats._fields_}

    def close(self):
        handle, self._handle = self._handle, None
        if handle is not None:
            L.lib().msw_raster_destroy(handle)
            self._rows = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass


# ---------------------------------------------------------------------- raster -> mesh
def zonal_launch(num_faces):
    """``(grid, faces_per_wg, iters)`` of the reduce kernel over ``num_faces`` faces (host only)."""
    g, p, it = C.c_int32(), C.c_int32(), C.c_int32()
    L.check(L.lib().msw_zonal_launch(int(num_faces), C.byref(g), C.byref(p), C.byref(it)))
    return g.value, p.value, it.value


def _cells_torch(pixel_rows, node_xy, face_nodes, face_row, grid):
    """``(face_ptr [nf + 1], pixels, centre_pixel [nf])`` int32 in numpy: the lists from a stable
    argsort of ``pixel_rows`` (ascending pixel index within a row), the centre pixel operation for
    operation in float64.  No two faces share a row (the caller has checked)."""
    rows = pixel_rows.reshape(-1).numpy()
    nf = face_row.shape[0]
    order = np.argsort(rows, kind="stable")
    order = order[rows[order] >= 0].astype(np.int32)
    valued = face_row >= 0
    top = int(face_row.max()) + 1 if valued.any() else 0
    per_row = np.bincount(rows[rows >= 0], minlength=top)[:top] if top else np.zeros(0, np.int64)
    # a pixel_rows value beyond the faces' rows cannot occur: pixel_rows holds face_row values only
    row_start = np.concatenate([[0], np.cumsum(per_row)])
    n = np.zeros(nf, np.int64)
    n[valued] = per_row[face_row[valued]]
    face_ptr = np.concatenate([[0], np.cumsum(n)])
    src = np.repeat(row_start[np.where(valued, face_row, 0)] - face_ptr[:-1], n) + np.arange(face_ptr[-1])
    pixels = order[src]
    xy = node_xy[face_nodes]                                   # [nf, 3, 2]
    cx = ((xy[:, 0, 0] + xy[:, 1, 0]) + xy[:, 2, 0]) / 3.0
    cy = ((xy[:, 0, 1] + xy[:, 1, 1]) + xy[:, 2, 1]) / 3.0
    with np.errstate(over="ignore", invalid="ignore"):
        i = np.floor((cx - grid.x0) / grid.dx + 0.5)
        j = np.floor((cy - grid.y0) / grid.dy + 0.5)
    inside = (i >= 0) & (i < grid.width) & (j >= 0) & (j < grid.height)
    centre = np.where(inside, np.where(inside, j, 0) * grid.width + np.where(inside, i, 0), -1).astype(np.int32)
    return (torch.from_numpy(face_ptr.astype(np.int32)), torch.from_numpy(np.ascontiguousarray(pixels, np.int32)),
            torch.from_numpy(centre))


def _reduce_torch(face_ptr, pixels, centre, layers, fill_centre, nodata_word):
    """Per-face words ``mean``, ``count``, ``min``, ``max`` [L, nf] int32 of ``layers`` [L, P]
    float32 from plain torch ops: float64 ``index_add_`` sums (sequential on the CPU), the extremes
    through an integer key in IEEE order with -0.0 below +0.0."""
    words = layers.contiguous().view(torch.int32)
    nl, nf = layers.shape[0], centre.shape[0]
    n = (face_ptr[1:] - face_ptr[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(nf), n)
    pw = words[:, pixels.long()]
    pv = pw.view(torch.float32)
    ok = ~torch.isnan(pv)
    total = torch.zeros(nl, nf, dtype=torch.float64).index_add_(1, seg, torch.where(ok, pv, torch.zeros(())).double())
    count = torch.zeros(nl, nf, dtype=torch.int64).index_add_(1, seg, ok.long())
    b = pw.long()
    key = torch.where(b >= 0, b, -(b & 0x7FFFFFFF) - 1)
    big = torch.tensor(1 << 40)
    segs = seg.expand(nl, -1)
    lo = torch.full((nl, nf), 1 << 40).scatter_reduce(1, segs, torch.where(ok, key, big), "amin")
    hi = torch.full((nl, nf), -(1 << 40)).scatter_reduce(1, segs, torch.where(ok, key, -big), "amax")

    def word(k):
        w = torch.where(k >= 0, k, (-(k + 1)) | 0x80000000)
        return (((w + (1 << 31)) % (1 << 32)) - (1 << 31)).to(torch.int32)
    fill = torch.full((nl, nf), nodata_word, dtype=torch.int32)
    if fill_centre:
        fill = torch.where(centre >= 0, words[:, centre.long().clamp(min=0)], fill)
    have = count > 0
    mean = (total / count.clamp(min=1).double()).float().view(torch.int32)
    return {"mean": torch.where(have, mean, fill), "count": count.to(torch.int32),
            "min": torch.where(have, word(lo), fill), "max": torch.where(have, word(hi), fill)}


_OUTPUTS = ("mean", "count", "min", "max")


class CellPixels:
    """For every face of a :class:`Rasterizer` the pixels whose centre it contains (C ABI
    ``msw_zonal_*``), and reductions of rasters over them: :meth:`reduce` / :meth:`mean` for layers
    (a DEM, roughness, an observed depth), :meth:`frames_to_rows` for a frame stack into
    ``[N, 2, T]`` rows -- the inverse of :meth:`Rasterizer.frames`.  Centres only: no fractional
    coverage.  Made by :meth:`Rasterizer.cells`; two faces with the same row are refused."""

    def __init__(self, raster, stream=None):
        xy, fn, fr = raster._geometry
        valued = fr[fr >= 0]
        if np.unique(valued).size != valued.size:
            raise ValueError("two faces share a face_row: the lists are keyed by face")
        self.grid, self.device = raster.grid, raster.device
        self.num_faces, self.min_row, self.max_row = raster.num_faces, raster.min_row, raster.max_row
        self._face_row = torch.from_numpy(fr)
        self._handle, self._lists = None, None
        if raster._handle is not None:
            out = C.c_void_p()
            L.check(L.lib().msw_zonal_create(raster._handle, raster._stream(stream), C.byref(out)))
            self._handle = out
        else:
            self._lists = _cells_torch(raster._rows, xy, fn, fr, raster.grid)

    def _stream(self, stream):
        return C.c_void_p(stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream)

    def _get_lists(self):
        """On a GPU: copies of the handle's arrays, made on first use."""
        if self._lists is None:
            if self._handle is None:
                raise RuntimeError("the cell lists are closed")
            ptrs = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
            L.check(L.lib().msw_zonal_lists(self._handle, *[C.byref(p) for p in ptrs]))
            sizes = (self.num_faces + 1, self.stats()["listed_pixels"], self.num_faces)
            copy = L.lib().hipMemcpy  # the HIP runtime the library links
            copy.argtypes, copy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
            out = []
            with torch.cuda.device(self.device):
                for p, size in zip(ptrs, sizes):
                    t = torch.empty(size, dtype=torch.int32, device=self.device)
                    if size and copy(t.data_ptr(), p, 4 * size, 3) != 0:   # hipMemcpyDeviceToDevice
                        raise RuntimeError("hipMemcpy failed")
                    out.append(t)
                torch.cuda.synchronize(self.device)
            self._lists = tuple(out)
        return self._lists

    @property
    def face_ptr(self):
        """[num_faces + 1] int32: face f's list is ``pixels[face_ptr[f]:face_ptr[f + 1]]``."""
        return self._get_lists()[0]

    @property
    def pixels(self):
        """int32 pixel indices ``j * width + i``, ascending within a face's list."""
        return self._get_lists()[1]

    @property
    def centre_pixel(self):
        """[num_faces] int32: the pixel nearest to each face's centroid, -1 outside the grid."""
        return self._get_lists()[2]

    # ------------------------------------------------------------------ reductions
    def _check(self, row_offset, num_rows):
        if self.max_row >= 0 and not (row_offset + self.min_row >= 0 and row_offset + self.max_row < num_rows):
            raise ValueError(f"row_offset {row_offset} + face rows [{self.min_row}, {self.max_row}] lie outside "
                             f"the {num_rows} rows given")

    def _layers(self, layers, what):
        H, W = self.grid.shape
        if not torch.is_tensor(layers) or layers.dim() != 3 or tuple(layers.shape[1:]) != (H, W):
            raise ValueError(f"{what} must be [L, {H}, {W}]")
        if layers.device != self.device:
            raise ValueError(f"{what} are on {layers.device}, the cell lists on {self.device}")
        if layers.dtype != torch.float32 or not layers.is_contiguous():
            layers = layers.float().contiguous()
        return layers

    def _scatter(self, out, values, row_offset):
        """CPU: the per-face words [L, nf] into ``out`` [L, n] at the faces' rows."""
        valued = self._face_row >= 0
        idx = self._face_row[valued].long() + row_offset
        out.view(torch.int32)[:, idx] = values[:, valued]

    def reduce(self, layers, row_offset=0, num_rows=None, fill_centre=True, nodata=float("nan"), out=None,
               stream=None):
        """Per-cell statistics of ``layers`` ``[H, W]`` or ``[L, H, W]`` -> a dict of ``mean``,
        ``min``, ``max`` (float32) and ``count`` (int32), each ``[num_rows]`` or ``[L, num_rows]``:
        face f's values at element ``row_offset + face_row[f]``.  NaN pixels are skipped; a cell
        with nothing left takes the pixel nearest to its centroid (``fill_centre``) or ``nodata``,
        its count 0.  ``out``: a dict of existing contiguous tensors (any of the four names) to
        write into, every other element left untouched -- successive scales fill one array; without
        it the outputs start as ``nodata`` / 0 and ``num_rows`` defaults to the rows the faces need."""
        single = torch.is_tensor(layers) and layers.dim() == 2
        layers = self._layers(layers[None] if single else layers, "layers")
        nl, row_offset = layers.shape[0], int(row_offset)
        if out is None:
            n = row_offset + self.max_row + 1 if num_rows is None else int(num_rows)
            self._check(row_offset, n)
            res = {k: torch.full((nl, n), 0 if k == "count" else float(nodata),
                                 dtype=torch.int32 if k == "count" else torch.float32, device=self.device)
                   for k in _OUTPUTS}
        else:
            if not out or set(out) - set(_OUTPUTS):
                raise ValueError(f"out holds any of {_OUTPUTS}")
            res = {}
            for k, t in out.items():
                want = torch.int32 if k == "count" else torch.float32
                if t.dtype != want or t.device != self.device or not t.is_contiguous() or t.dim() != (1 if single else 2):
                    raise ValueError(f"out[{k!r}] must be a contiguous {want} tensor on {self.device}")
                res[k] = t[None] if single else t
            shapes = {tuple(t.shape) for t in res.values()}
            n = next(iter(shapes))[1]
            if len(shapes) != 1 or next(iter(shapes))[0] != nl or (num_rows is not None and int(num_rows) != n):
                raise ValueError("the outputs must share one shape [L, num_rows]")
            self._check(row_offset, n)
        if nl and self.max_row >= 0:
            if self._handle is None:
                if self._lists is None:
                    raise RuntimeError("the cell lists are closed")
                got = _reduce_torch(*self._lists, layers.reshape(nl, -1), fill_centre, _signed(_bits(nodata)))
                for k, t in res.items():
                    self._scatter(t, got[k], row_offset)
            else:
                ptr = lambda k: C.c_void_p(res[k].data_ptr()) if k in res else None  # noqa: E731
                L.check(L.lib().msw_zonal_reduce(self._handle, C.c_void_p(layers.data_ptr()), nl, layers.stride(0),
                                                 row_offset, n, n, int(bool(fill_centre)), _bits(nodata), ptr("mean"),
                                                 ptr("count"), ptr("min"), ptr("max"), self._stream(stream)))
        return {k: (t[0] if single else t) for k, t in res.items()}

    def mean(self, layers, row_offset=0, num_rows=None, fill_centre=True, nodata=float("nan"), stream=None):
        """The mean of :meth:`reduce` alone."""
        single = torch.is_tensor(layers) and layers.dim() == 2
        nl = 1 if single else (layers.shape[0] if torch.is_tensor(layers) and layers.dim() == 3 else 0)
        n = int(row_offset) + self.max_row + 1 if num_rows is None else int(num_rows)
        if n < 0:
            raise ValueError("num_rows negative")
        out = torch.full((n,) if single else (nl, n), float(nodata), dtype=torch.float32, device=self.device)
        return self.reduce(layers, row_offset, n, fill_centre, nodata, {"mean": out}, stream)["mean"]

    def frames_to_rows(self, frames, pred, var=0, t_begin=0, row_offset=0, fill_centre=True, nodata=float("nan"),
                       stream=None):
        """Frames ``[t_count, H, W]`` into ``pred`` [N, 2, T] (float32, contiguous, written in
        place): ``pred[row_offset + face_row[f], var, t_begin + k]`` = the :meth:`mean` of frame k
        on face f, bit for bit; nothing else in ``pred`` changes.  Returns ``pred``."""
        if not torch.is_tensor(pred) or pred.dim() != 3 or pred.shape[1] != 2:
            raise ValueError("pred must be [N, 2, T]")
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            raise ValueError("pred is written in place: it must be float32 and contiguous")
        if var not in (0, 1):
            raise ValueError("var is 0 (depth) or 1 (discharge)")
        frames = self._layers(frames, "frames")
        N, T, tc = int(pred.shape[0]), int(pred.shape[2]), int(frames.shape[0])
        t_begin, row_offset = int(t_begin), int(row_offset)
        if t_begin < 0 or t_begin + tc > T:
            raise ValueError(f"steps [{t_begin}, {t_begin + tc}) lie outside the rollout's {T}")
        if pred.device != self.device:
            raise ValueError(f"pred is on {pred.device}, the cell lists on {self.device}")
        self._check(row_offset, N)
        if not tc or self.max_row < 0:
            return pred
        if self._handle is None:
            if self._lists is None:
                raise RuntimeError("the cell lists are closed")
            got = _reduce_torch(*self._lists, frames.reshape(tc, -1), fill_centre, _signed(_bits(nodata)))["mean"]
            valued = self._face_row >= 0
            idx = self._face_row[valued].long() + row_offset
            pred.view(torch.int32)[idx, var, t_begin:t_begin + tc] = got[:, valued].t()
        else:
            L.check(L.lib().msw_zonal_frames(self._handle, C.c_void_p(frames.data_ptr()), frames.stride(0),
                                             C.c_void_p(pred.data_ptr()), N, T, var, t_begin, tc, row_offset,
                                             int(bool(fill_centre)), _bits(nodata), self._stream(stream)))
        return pred

    # ------------------------------------------------------------------ bookkeeping
    def launch(self):
        """``(grid, faces_per_wg, iters)`` of the reduce kernel for these faces."""
        return zonal_launch(self.num_faces)

    def stats(self):
        """``num_faces``, ``listed_pixels``, ``longest_list``, ``empty_faces`` (valued faces with an
        empty list), ``wave_faces`` (lists of more than 32 pixels: a wave each on the GPU),
        ``device_bytes``, ``build_us`` (the last two zero on the CPU)."""
        s = L.MswZonalStats()
        if self._handle is not None:
            L.check(L.lib().msw_zonal_get_stats(self._handle, C.byref(s)))
        elif self._lists is not None:
            n = (self._lists[0][1:] - self._lists[0][:-1])
            s.num_faces, s.listed_pixels = self.num_faces, int(self._lists[0][-1])
            s.longest_list = int(n.max()) if self.num_faces else 0
            s.empty_faces = int(((n == 0) & (self._face_row >= 0)).sum())
            s.wave_faces = int((n > 32).sum())
        return {k: getattr(s, k) for k, _ in L.MswZonalStats._fields_}

    def close(self):
        handle, self._handle = self._handle, None
        self._lists = None
        if handle is not None:
            L.lib().msw_zonal_destroy(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass
