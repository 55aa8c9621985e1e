"""Mesh graphs (C ABI ``msw_locator_*`` / ``msw_mesh_dual_*``): multiscale graphs in the reference's
layout from plain triangulations, and graph rows from (x, y) points.

Everything downstream of a :class:`mswegnn.mesh.Graph` runs on the device; this module is the way
in for a mesh that is not one of ``mswegnn.mesh``'s synthetic quadtrees.  The reference builds its
graphs on the host (``database/graph_creation.py``: meshkernel, networkx, and one matplotlib
``Path.contains_points`` call per coarse face over all fine centres); here

* :class:`PointLocator` finds the face under arbitrary points with the rasters' fp64 predicates
  (include/mswegnn.h, "Raster products": edge functions taken from the lower vertex index, the
  lowest face index wins) over the rasters' bucket grid, and turns gauge positions into
  :meth:`mswegnn.series.Zones.gauges`;
* :class:`DualGraph` is the dual graph of one scale from coordinates and vertex lists alone:
  centroids, areas, the face across each edge, the coalesced ``edge_index``, the centroid distances
  and the boundary edges;
* :func:`intra_edges` is the reference's coarse-to-fine rule (``connect_coarse_to_fine_mesh``): one
  locate plus a stable argsort;
* :func:`graph_from_meshes` assembles a ``Graph`` with every attribute
  ``mswegnn.mesh.make_multiscale_mesh`` sets, in the same layout; on the generator's own geometry
  (``multiscale_geometry``) it reproduces the generator's graph.

Out of scope: mesh generation and refinement themselves, quadrilateral or polygonal faces, more
than one BC edge per scale, the reference's ``get_slopes``, reading the reference's pickles, and any
renumbering of the built graph -- it keeps the caller's face order.  A mesh numbered without
locality need not run the engine's gathers without it: ``graph_from_meshes(..., locality=True)`` sets
``graph.row_order`` (``mswegnn.locality``), the order in which a plan lays the rows out internally.

On CPU tensors the same interface runs :func:`_locate_numpy` / :func:`_dual_numpy`, plain numpy
restatements of the kernels.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .mesh import Graph, _standardize, hydrograph_bc
from .series import Zones

__all__ = ["PointLocator", "DualGraph", "MeshGraph", "intra_edges", "graph_from_meshes", "locate_launch",
           "mesh_dual_launch"]


def _launch(fn, n):
    g, p, it = C.c_int32(), C.c_int32(), C.c_int32()
    L.check(fn(int(n), C.byref(g), C.byref(p), C.byref(it)))
    return g.value, p.value, it.value


def locate_launch(n):
    """``(grid, points_per_wg, iters)`` of the locate kernel for ``n`` points (host only)."""
    return _launch(L.lib().msw_locate_launch, n)


def mesh_dual_launch(num_faces):
    """``(grid, faces_per_wg, iters)`` of the dual-graph kernels over ``num_faces`` faces (host only)."""
    return _launch(L.lib().msw_mesh_dual_launch, num_faces)


def _numpy(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def _mesh(node_xy, face_nodes):
    """-> (xy float64 [V, 2], fn [nf, 3]) as contiguous numpy, shapes checked (values are not)."""
    xy = np.ascontiguousarray(_numpy(node_xy), dtype=np.float64)
    fn = _numpy(face_nodes)
    if xy.ndim != 2 or xy.shape[1] != 2:
        raise ValueError("node_xy must be [V, 2]")
    if fn.ndim != 2 or fn.shape[1] != 3:
        raise ValueError("faces are triangles: face_nodes must be [nf, 3]")
    if fn.size and not np.issubdtype(fn.dtype, np.integer):
        raise ValueError("face_nodes must hold integers")
    return xy, fn


def _device(device):
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def _copy_out(ptr, shape, dtype, device):
    """A torch copy of a handle's device array (with the HIP runtime the library links)."""
    t = torch.empty(shape, dtype=dtype, device=device)
    if t.numel():
        copy = L.lib().hipMemcpy
        copy.argtypes, copy.restype = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int], C.c_int
        if copy(t.data_ptr(), ptr, t.numel() * t.element_size(), 3) != 0:   # hipMemcpyDeviceToDevice
            raise RuntimeError("hipMemcpy failed")
    return t


# ---------------------------------------------------------------------------------- point locator
def _edge(u, v, neg, px, py):
    """E(u -> v) at the points; ``neg``: u is not the lower vertex index (the edge is taken from v
    and the result negated)."""
    p, q = (v, u) if neg else (u, v)
    e = (q[0] - p[0]) * (py - p[1]) - (q[1] - p[1]) * (px - p[0])
    return -e if neg else e


def _locate_numpy(xy, fn, fr, pts):
    """rows [n] int32 of the points ``pts`` [n, 2] in numpy float64: the faces in descending order,
    each over the points in its bounding box widened by the kernel's margin, a later (lower) face
    overwriting an earlier one -- the lowest containing face wins, also when its ``face_row`` is
    -1.  A NaN or infinite point lies in no box."""
    n = pts.shape[0]
    rows = np.full(n, -1, dtype=np.int32)
    finite = np.nonzero(np.isfinite(pts).all(1))[0]
    order = finite[np.argsort(pts[finite, 0], kind="stable")]
    sx, sy = pts[order, 0], pts[order, 1]
    for f in range(fn.shape[0] - 1, -1, -1):
        ia, ib, ic = (int(v) for v in fn[f])
        a, b, c = xy[ia], xy[ib], xy[ic]
        area2 = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
        if not (area2 > 0 or area2 < 0):
            continue
        xlo, xhi = min(a[0], b[0], c[0]), max(a[0], b[0], c[0])
        ylo, yhi = min(a[1], b[1], c[1]), max(a[1], b[1], c[1])
        d = max(xhi - xlo, yhi - ylo)
        m = 2.0 ** -40 * d * (d * d / abs(area2))  # csrc/raster_handle.h face_margin
        m = m if m <= d else d
        k0, k1 = np.searchsorted(sx, xlo - m, "left"), np.searchsorted(sx, xhi + m, "right")
        if k0 >= k1:
            continue
        qx, qy = sx[k0:k1], sy[k0:k1]
        e0, e1, e2 = _edge(a, b, ia > ib, qx, qy), _edge(b, c, ib > ic, qx, qy), _edge(c, a, ic > ia, qx, qy)
        if area2 > 0:
            inside = (e0 >= 0) & (e1 >= 0) & (e2 >= 0)
        else:
            inside = (e0 <= 0) & (e1 <= 0) & (e2 <= 0)
        rows[order[k0:k1][inside]] = fr[f]
    return rows


class PointLocator:
    """The face under arbitrary points, in the triangles ``face_nodes`` [nf, 3] over ``node_xy``
    [V, 2] of one mesh scale.  ``face_row`` [nf]: the row reported for face f (default f; -1: the
    face takes part and yields -1).  ``device``: a GPU runs ``k_locate_points`` over a host-built
    bucket grid, ``"cpu"`` the numpy restatement."""

    def __init__(self, node_xy, face_nodes, face_row=None, device="cpu"):
        xy, fn = _mesh(node_xy, face_nodes)
        if not np.isfinite(xy).all():
            raise ValueError("node coordinates must be finite")
        if fn.size and (fn.min() < 0 or fn.max() >= xy.shape[0]):
            raise ValueError("vertex index outside [0, V)")
        fn = np.ascontiguousarray(fn, dtype=np.int32)
        nf = fn.shape[0]
        if face_row is None:
            fr = np.arange(nf, dtype=np.int32)
        else:
            fr = _numpy(face_row).reshape(-1)
            if fr.shape[0] != nf:
                raise ValueError("face_row must hold one row per face")
            if fr.size and (fr.min() < -1 or fr.max() > 2 ** 31 - 1):
                raise ValueError("face_row must be -1 or a row index")
            fr = np.ascontiguousarray(fr, dtype=np.int32)
        self.num_faces, self.device = nf, _device(device)
        self._geometry = (xy, fn, fr)
        self._handle = None
        if self.device.type == "cuda":
            out = C.c_void_p()
            L.check(L.lib().msw_locator_create(xy.ctypes.data_as(C.POINTER(C.c_double)), xy.shape[0],
                                               fn.ctypes.data_as(L.c_int32_p), fr.ctypes.data_as(L.c_int32_p), nf,
                                               self.device.index, C.byref(out)))
            self._handle = out

    def locate(self, xy, stream=None):
        """``xy`` [n, 2] (float64 is used as given; anything else is converted) -> int32 rows [n] on
        this locator's device: ``face_row`` of the lowest face containing each point, -1 for none."""
        pts = xy if torch.is_tensor(xy) else torch.from_numpy(np.ascontiguousarray(_numpy(xy), dtype=np.float64))
        if pts.dim() != 2 or pts.shape[1] != 2:
            raise ValueError("points must be [n, 2]")
        pts = pts.to(self.device, torch.float64).contiguous()
        n = pts.shape[0]
        if self.device.type != "cuda":
            return torch.from_numpy(_locate_numpy(*self._geometry, pts.numpy()))
        if self._handle is None:
            raise RuntimeError("the locator is closed")
        with torch.cuda.device(self.device):
            rows = torch.empty(n, dtype=torch.int32, device=self.device)
            st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream)
            L.check(L.lib().msw_locate_points(self._handle, C.c_void_p(pts.data_ptr()), n,
                                              C.c_void_p(rows.data_ptr()), st))
        return rows

    def gauges(self, xy, num_rows, row_offset=0):
        """A :meth:`Zones.gauges` set, one zone per point: graph row ``row_offset`` + the located
        row (``num_rows``: the rows of the graph the series will run on).  Raises for a point in no
        cell."""
        rows = self.locate(xy).cpu().long()
        missing = torch.nonzero(rows < 0).reshape(-1)
        if missing.numel():
            raise ValueError(f"{missing.numel()} point(s) lie in no cell (first: point {int(missing[0])})")
        return Zones.gauges(rows + int(row_offset), num_rows)

    def stats(self):
        """``buckets``, ``buckets_x``, ``buckets_y``, ``list_entries``, ``longest_list``,
        ``device_bytes``, ``host_build_seconds`` (zeros on the CPU, where there is no bucket grid)."""
        s = L.MswLocatorStats()
        if self._handle is not None:
            L.check(L.lib().msw_locator_get_stats(self._handle, C.byref(s)))
        return {k: getattr(s, k) for k, _ in L.MswLocatorStats._fields_}

    def close(self):
        handle, self._handle = self._handle, None
        if handle is not None:
            L.lib().msw_locator_destroy(handle)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass


# ---------------------------------------------------------------------------------- dual graph
def _dual_numpy(xy, fn):
    """The arrays of ``msw_mesh_dual_create`` in numpy, the checks and their order included
    (``ValueError("face F: ...")``).  -> centroid [nf, 2], area [nf], adjacent [nf, 3] int32,
    edge_index [2, E] int64, edge_length [E], boundary [nb, 2] int32."""
    nf, V = fn.shape[0], xy.shape[0]
    fn = fn.astype(np.int64)

    def refuse(bad, what):
        raise ValueError(f"face {int(np.nonzero(bad)[0][0])}: {what}")

    with np.errstate(all="ignore"):
        if nf:
            out = ((fn < 0) | (fn >= V)).any(1)
            safe = np.where(out[:, None], 0, fn) if V else np.zeros_like(fn)
            rep = (fn[:, 0] == fn[:, 1]) | (fn[:, 1] == fn[:, 2]) | (fn[:, 2] == fn[:, 0])
            p = xy[safe] if V else np.zeros((nf, 3, 2))
            a, b, c = p[:, 0], p[:, 1], p[:, 2]
            nonfin = ~np.isfinite(p).all((1, 2))
            area2 = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (c[:, 0] - a[:, 0]) * (b[:, 1] - a[:, 1])
            flat = ~np.isfinite(area2) | (area2 == 0)
            bad = out | rep | nonfin | flat
            if bad.any():  # the lowest face that fails, and the first check that it fails
                f = int(np.nonzero(bad)[0][0])
                what = ("vertex index outside [0, num_nodes)" if out[f] else "repeats a vertex" if rep[f] else
                        "a coordinate is not finite" if nonfin[f] else "area2 is zero or not finite")
                raise ValueError(f"face {f}: {what}")
        if not np.isfinite(xy).all():
            raise ValueError("node coordinate not finite")
        if nf == 0:
            return (np.zeros((0, 2)), np.zeros(0), np.zeros((0, 3), np.int32), np.zeros((2, 0), np.int64),
                    np.zeros(0), np.zeros((0, 2), np.int32))
        centroid = ((a + b) + c) / 3.0
        area = 0.5 * np.abs(area2)
    u, w = fn, fn[:, [1, 2, 0]]                              # slot k: (a, b), (b, c), (c, a)
    key = (np.minimum(u, w) * V + np.maximum(u, w)).reshape(-1)
    order = np.argsort(key, kind="stable")                   # equal keys: ascending (face, slot)
    sk = key[order]
    start = np.concatenate([[True], sk[1:] != sk[:-1]])
    gid = np.cumsum(start) - 1
    size = np.bincount(gid)
    crowded = np.zeros(nf, bool)
    crowded[order[size[gid] > 2] // 3] = True
    if crowded.any():
        refuse(crowded, "an edge is shared by more than two faces")
    adjacent = np.full(3 * nf, -1, np.int64)
    first = np.nonzero(start & (size[gid] == 2))[0]
    adjacent[order[first]] = order[first + 1] // 3
    adjacent[order[first + 1]] = order[first] // 3
    adjacent = adjacent.reshape(nf, 3)
    twice = ((adjacent[:, 0] >= 0) & ((adjacent[:, 0] == adjacent[:, 1]) | (adjacent[:, 0] == adjacent[:, 2]))) | \
            ((adjacent[:, 1] >= 0) & (adjacent[:, 1] == adjacent[:, 2]))
    if twice.any():
        refuse(twice, "shares more than one edge with another face")
    cols = np.sort(np.where(adjacent < 0, np.iinfo(np.int64).max, adjacent), 1)
    keep = cols != np.iinfo(np.int64).max
    rows = np.broadcast_to(np.arange(nf)[:, None], (nf, 3))[keep]
    cols = cols[keep]
    d = centroid[cols] - centroid[rows]
    edge_length = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
    boundary = np.argwhere(adjacent < 0).astype(np.int32)    # face-major, slots ascending
    return (centroid, area, adjacent.astype(np.int32), np.stack([rows, cols]).astype(np.int64), edge_length,
            boundary)


class DualGraph:
    """The dual graph of one scale (graph nodes are faces) from ``node_xy`` [V, 2] and
    ``face_nodes`` [nf, 3] alone, as tensors on ``device``: ``centroid`` [nf, 2] and ``area`` [nf]
    float64, ``adjacent`` [nf, 3] int32 (the face across the edges (a, b), (b, c), (c, a); -1 on the
    boundary), ``edge_index`` [2, E] int64 (both directions, rows ascending, each row's columns
    ascending), ``edge_length`` [E] float64 between the centroids and ``boundary`` [nb, 2] int32
    ``(face, slot)`` pairs.  Faces may have either orientation and vertices may be unused; a face
    that repeats a vertex, has no area, an index out of range or a non-finite coordinate, an edge
    shared by more than two faces and two faces sharing more than one edge are refused with the
    lowest offending face named.  A GPU runs ``k_mesh_faces`` / ``k_mesh_edges``."""

    _NAMES = ("centroid", "area", "adjacent", "edge_index", "edge_length", "boundary")

    def __init__(self, node_xy, face_nodes, device="cpu", stream=None):
        xy, fn = _mesh(node_xy, face_nodes)
        self.num_faces, self.device = fn.shape[0], _device(device)
        self._stats = None
        if self.device.type != "cuda":
            arrays = [torch.from_numpy(np.ascontiguousarray(a)) for a in _dual_numpy(xy, fn)]
        else:
            if fn.size and (fn.min() < -2 ** 31 or fn.max() > 2 ** 31 - 1):
                raise ValueError("face 0: vertex index outside int32")
            fn = np.ascontiguousarray(fn, dtype=np.int32)
            nf = fn.shape[0]
            handle = C.c_void_p()
            with torch.cuda.device(self.device):
                st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(self.device).cuda_stream)
                rc = L.lib().msw_mesh_dual_create(xy.ctypes.data_as(C.POINTER(C.c_double)), xy.shape[0],
                                                  fn.ctypes.data_as(L.c_int32_p), nf, self.device.index, st,
                                                  C.byref(handle))
                if rc != L.MSW_OK:
                    msg = L.lib().msw_last_error().decode(errors="replace")
                    if rc == -1 or msg.startswith("face "):
                        raise ValueError(msg)
                    L.check(rc)
                try:
                    p = [C.c_void_p() for _ in range(6)]
                    E, nb = C.c_int64(), C.c_int64()
                    L.check(L.lib().msw_mesh_dual_arrays(handle, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]),
                                                         C.byref(p[3]), C.byref(p[4]), C.byref(E), C.byref(p[5]),
                                                         C.byref(nb)))
                    shapes = ((nf, 2), (nf,), (nf, 3), (2, E.value), (E.value,), (nb.value, 2))
                    dtypes = (torch.float64, torch.float64, torch.int32, torch.int64, torch.float64, torch.int32)
                    arrays = [_copy_out(q, s, t, self.device) for q, s, t in zip(p, shapes, dtypes)]
                    torch.cuda.synchronize(self.device)
                    s = L.MswMeshDualStats()
                    L.check(L.lib().msw_mesh_dual_get_stats(handle, C.byref(s)))
                    self._stats = {k: getattr(s, k) for k, _ in L.MswMeshDualStats._fields_}
                finally:
                    L.lib().msw_mesh_dual_destroy(handle)
        for name, a in zip(self._NAMES, arrays):
            setattr(self, name, a)

    @property
    def num_edges(self):
        return int(self.edge_index.shape[1])

    def stats(self):
        """``msw_mesh_dual_stats`` of the build (``None`` on the CPU)."""
        return self._stats


# ---------------------------------------------------------------------------------- intra edges
def intra_edges(fine, coarse):
    """The reference's coarse-to-fine rule: one (coarse, fine) pair per fine face whose centroid
    lies in a coarse face -> int64 [2, n] (row 0 coarse, row 1 fine), coarse-major, fine ascending.
    A centroid on a shared edge or vertex goes to the lowest coarse face; a fine face in no coarse
    face has no pair.  ``fine``: a :class:`DualGraph` or centroids [n, 2]; ``coarse``: a
    :class:`PointLocator` over the coarse faces."""
    centroid = fine.centroid if isinstance(fine, DualGraph) else fine
    parent = coarse.locate(centroid).long()
    child = torch.nonzero(parent >= 0).reshape(-1)
    order = torch.argsort(parent[child], stable=True)
    return torch.stack([parent[child][order], child[order]])


# ---------------------------------------------------------------------------------- the builder
class MeshGraph:
    """What :func:`graph_from_meshes` returns: ``graph`` (a :class:`mswegnn.mesh.Graph` on the CPU,
    as ``make_multiscale_mesh`` returns) and, per scale (finest first), ``locators``, ``centroids``
    (float64 [nf, 2]), ``bc_face``, ``bc_edge`` (``(face, slot)``), ``bc_point`` (the midpoint of
    that edge), ``orphans`` (faces with no parent in the next coarser scale; 0 for the coarsest) and
    ``childless`` (faces with no child in the next finer scale; 0 for the finest).  Raw edge
    attributes the reference also keeps, over all of ``graph.edge_index`` and not part of
    ``graph``: ``face_relative_distance`` float64 [E, 2] (centroid of the column minus that of the
    row; a ghost's centroid is its BC face's mirrored in the BC edge) and ``edge_slope`` float64 [E]
    ((DEM[row] - DEM[column]) / length)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def row_xy(self):
        """float64 [N, 2], one coordinate per graph row for ``mswegnn.locality.row_order``: each
        face's centroid, each scale's ghost row at the centroid of its BC face (equal keys go to the
        lower row, so the ghost follows that face)."""
        return torch.cat([torch.cat([c, c[f:f + 1]]) for c, f in zip(self.centroids, self.bc_face)])

    def gauges(self, xy, scale=0):
        """Zones of one graph row per point, located in the faces of ``scale``."""
        g = self.graph
        return self.locators[scale].gauges(xy, g.num_nodes, int(g.node_ptr[scale]))


def _per_scale_dem(dem, nfs):
    if isinstance(dem, (list, tuple)) and len(dem) == len(nfs) and all(np.ndim(_numpy(d)) >= 1 for d in dem):
        out = [np.asarray(_numpy(d), dtype=np.float64).reshape(-1) for d in dem]
        for s, (d, nf) in enumerate(zip(out, nfs)):
            if d.shape[0] != nf:
                raise ValueError(f"dem of scale {s} must hold one value per face ({nf})")
        return out
    d = np.asarray(_numpy(dem), dtype=np.float64).reshape(-1)
    if d.shape[0] != nfs[0]:
        raise ValueError(f"dem must hold one value per finest face ({nfs[0]}), or be one array per scale")
    return [d]


def graph_from_meshes(scales, bc_xy, dem, previous_t=3, T=48, BC=None, type_BC=2, device="cpu", locality=False):
    """A multiscale graph in the reference's layout from plain triangulations.

    ``scales``: finest first, each ``(node_xy float64 [V, 2], face_nodes int32 [nf, 3])`` (what
    ``mswegnn.mesh.multiscale_geometry`` returns); they need not be nested.  ``bc_xy``: the inflow
    point.  Per scale, finest first, the BC edge is the boundary edge whose midpoint is nearest to
    the current point (ties: the lowest (face, slot)), and that midpoint becomes the point for the
    next coarser scale.  ``dem``: one value per finest face (``CellPixels.mean`` of a DEM raster
    gives it) or one array per scale; from the finest array every coarser face takes the float64
    mean of its children summed in ascending order, a childless face the value of the finer face
    that contains its centroid (none: ``ValueError`` with the count).  ``BC``: [nBC, previous_t,
    T + 1] (default: ``mswegnn.mesh.hydrograph_bc``).  ``device``: where the kernels run; the
    standardisation runs in numpy float64 on the host, and the graph is returned on the CPU.
    ``locality=True`` also sets ``graph.row_order`` (``mswegnn.locality.row_order`` of
    ``MeshGraph.row_xy``, computed on ``device``): the graph's arrays are the same either way.

    Layout (``mswegnn.mesh``): each scale's faces then its ghost row; each scale's dual edges
    sorted by (row, col) then the directed ghost -> BC-face edge; intra pairs coarse-major with the
    ghost -> ghost pair last; ``x = [area standardised per scale, DEM - global minimum,
    2 * previous_t zeros]``; the ghost takes its BC face's area and DEM, its edge twice the distance
    from the BC face's centroid to the BC edge's line."""
    device = _device(device)
    if len(scales) < 1:
        raise ValueError("at least one scale")
    point = np.asarray(_numpy(bc_xy), dtype=np.float64).reshape(-1)
    if point.shape[0] != 2 or not np.isfinite(point).all():
        raise ValueError("bc_xy must be a finite (x, y)")
    S = len(scales)
    sc = []
    for s, (node_xy, face_nodes) in enumerate(scales):
        xy, fn = _mesh(node_xy, face_nodes)
        dual = DualGraph(xy, fn, device=device)
        if dual.num_faces == 0 or dual.boundary.shape[0] == 0:
            raise ValueError(f"scale {s} has no face or no boundary edge")
        c, area = dual.centroid.cpu().numpy(), dual.area.cpu().numpy()
        ei, dist = dual.edge_index.cpu().numpy(), dual.edge_length.cpu().numpy()
        bnd = dual.boundary.cpu().numpy().astype(np.int64)
        # ---- the BC edge: nearest midpoint, ties to the lowest (face, slot); it moves the point
        u = fn[bnd[:, 0], bnd[:, 1]]
        v = fn[bnd[:, 0], (bnd[:, 1] + 1) % 3]
        mid = 0.5 * (xy[u] + xy[v])
        mx, my = mid[:, 0] - point[0], mid[:, 1] - point[1]
        k = int(np.argmin(mx * mx + my * my))
        bc_face, bc_slot = int(bnd[k, 0]), int(bnd[k, 1])
        point = mid[k].copy()
        p, q = xy[u[k]], xy[v[k]]
        ex, ey = q[0] - p[0], q[1] - p[1]
        elen = np.sqrt(ex * ex + ey * ey)
        cross = ex * (c[bc_face, 1] - p[1]) - ey * (c[bc_face, 0] - p[0])
        ghost_len = 2.0 * (abs(cross) / elen)
        ghost_c = c[bc_face] - 2.0 * (cross / elen) * np.array([-ey, ex]) / elen   # mirrored in the edge's line
        nf = fn.shape[0]
        sc.append(dict(
            nf=nf, c=c, ghost_c=ghost_c, area=np.append(area, area[bc_face]),
            edge_index=np.concatenate([ei, np.array([[nf], [bc_face]])], 1),
            dist=np.append(dist, ghost_len), bc_face=bc_face, bc_edge=(bc_face, bc_slot), bc_point=point.copy(),
            bc_edge_len=elen, locator=PointLocator(xy, fn, device=device), dual=dual))

    # ---- parents, and the DEM pooled up the scales
    dems = _per_scale_dem(dem, [d["nf"] for d in sc])
    pooled = len(dems) == 1 and S > 1
    parents, orphans, childless = [], [0] * S, [0] * S
    for s in range(S - 1):
        fine, coarse = sc[s], sc[s + 1]
        parent = coarse["locator"].locate(fine["dual"].centroid).cpu().numpy().astype(np.int64)
        has = parent >= 0
        parents.append(parent)
        orphans[s] = int((~has).sum())
        cnt = np.bincount(parent[has], minlength=coarse["nf"])
        empty = np.nonzero(cnt == 0)[0]
        childless[s + 1] = int(empty.shape[0])
        if pooled:
            sm = np.zeros(coarse["nf"])
            np.add.at(sm, parent[has], dems[-1][has])          # ascending child order (mesh.py:215-221)
            d = sm / np.maximum(cnt, 1)
            if empty.shape[0]:
                under = fine["locator"].locate(coarse["dual"].centroid[torch.from_numpy(empty).to(device)])
                under = under.cpu().numpy().astype(np.int64)
                if (under < 0).any():
                    raise ValueError(f"{int((under < 0).sum())} childless face(s) of scale {s + 1} have no finer "
                                     "face under their centroid to take a DEM value from")
                d[empty] = dems[-1][under]
            dems.append(d)
    dem_min = min(d.min() for d in dems)
    for s in range(S):
        d = dems[s] - dem_min
        sc[s]["dem"] = np.append(d, d[sc[s]["bc_face"]])       # the ghost copies its BC face

    # ---- assembly, as mswegnn.mesh.make_multiscale_mesh
    face_ptr = np.cumsum([0] + [d["nf"] + 1 for d in sc])
    edge_ptr = np.cumsum([0] + [d["edge_index"].shape[1] for d in sc])
    N = int(face_ptr[-1])
    edge_index = np.concatenate([d["edge_index"] + face_ptr[s] for s, d in enumerate(sc)], 1)
    edge_attr = np.concatenate([_standardize(d["dist"]) for d in sc])[:, None]
    area = np.concatenate([_standardize(d["area"]) for d in sc])
    dem_all = np.concatenate([d["dem"] for d in sc])
    intra = []
    for s in range(S - 1):
        parent = parents[s]
        child = np.nonzero(parent >= 0)[0]
        order = np.argsort(parent[child], kind="stable")      # coarse-major, fine ascending
        pairs = np.stack([np.append(parent[child][order], sc[s + 1]["nf"]),   # the ghost nests in the coarse ghost
                          np.append(child[order], sc[s]["nf"])])
        intra.append(pairs + np.array([[face_ptr[s + 1]], [face_ptr[s]]]))
    intra_edge_ptr = np.cumsum([0] + [p.shape[1] for p in intra])
    intra_edge_index = np.concatenate(intra, 1) if intra else np.zeros((2, 0), np.int64)

    x = np.zeros((N, 2 + 2 * previous_t), dtype=np.float32)
    x[:, 0] = area
    x[:, 1] = dem_all
    bc = hydrograph_bc(T, previous_t) if BC is None else np.asarray(_numpy(BC), dtype=np.float32)
    if bc.ndim != 3 or bc.shape[1] != previous_t or bc.shape[2] != T + 1:
        raise ValueError(f"BC must be [nBC, {previous_t}, {T + 1}]")
    cc = np.concatenate([np.concatenate([d["c"], d["ghost_c"][None]], 0) for d in sc], 0)
    rel = cc[edge_index[1]] - cc[edge_index[0]]
    raw_len = np.concatenate([d["dist"] for d in sc])
    graph = Graph(
        x=torch.from_numpy(x),
        edge_index=torch.from_numpy(edge_index.astype(np.int64)),
        edge_attr=torch.from_numpy(edge_attr.astype(np.float32)),
        edge_ptr=torch.from_numpy(edge_ptr.astype(np.int64)),
        node_ptr=torch.from_numpy(face_ptr.astype(np.int64)),
        intra_mesh_edge_index=torch.from_numpy(intra_edge_index.astype(np.int64)),
        intra_edge_ptr=torch.from_numpy(intra_edge_ptr.astype(np.int64)),
        BC=torch.from_numpy(np.ascontiguousarray(bc, dtype=np.float32)),
        node_BC=torch.from_numpy(np.array([face_ptr[0] + sc[0]["nf"]], dtype=np.int32)),
        type_BC=torch.tensor(int(type_BC), dtype=torch.int),
        y=torch.zeros(N, 2, T),
        temporal_res=torch.tensor(120),
        previous_t=torch.tensor(previous_t),
        area=torch.from_numpy(np.concatenate([d["area"] for d in sc]).astype(np.float32)),
        edge_BC_length=torch.tensor([d["bc_edge_len"] for d in sc], dtype=torch.float32),
    )
    out = MeshGraph(
        graph=graph, locators=[d["locator"] for d in sc], centroids=[torch.from_numpy(d["c"]) for d in sc],
        bc_face=[d["bc_face"] for d in sc], bc_edge=[d["bc_edge"] for d in sc],
        bc_point=[d["bc_point"] for d in sc], orphans=orphans, childless=childless,
        face_relative_distance=torch.from_numpy(rel),
        edge_slope=torch.from_numpy((dem_all[edge_index[0]] - dem_all[edge_index[1]]) / raw_len))
    if locality:
        from .locality import row_order
        graph.row_order = row_order(graph, out.row_xy, device=device)
    return out
