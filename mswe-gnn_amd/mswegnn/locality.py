"""Locality row order (C ABI ``msw_locality_order`` / ``msw_plan_create_ordered``): a base row order
for a plan from per-row coordinates.

A plan keeps the caller's numbering at every boundary and lays each (graph, scale) range out in graph
order, so a mesh numbered without locality runs every row gather of the step without it.
:func:`row_order` sorts the rows of each range along one Hilbert curve (order 16, 65,536 cells a
side) over the bounding square of the graph's coordinates; set as ``graph.row_order`` it becomes the
order in which ``EnginePlan`` lays the rows out (``msw_plan_create_ordered``).  Nothing is
relabelled: x, y, node_BC, zones, raster ``face_row`` and gauges keep their row numbers, and the
plan gives the bits of the plan without an order.

* all scales of one graph share one box, so the curve nests across scales and the children of a
  coarse face land near each other;
* ``mswegnn.batch.collate`` drops ``row_order`` (concatenated, the members' orders would lack their
  offsets and the plan would refuse them): a batch of ordered graphs carries none; compute the
  order on the collated batch, whose ``node_ptr`` is ``[G, S+1]``;
* the torch path of a model ignores the attribute; partitioned plans refuse it.

On CPU tensors the same interface runs the numpy restatement (:func:`_keys_numpy` and a stable
argsort per segment), which is the definition of the kernels' output, bit for bit.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L

__all__ = ["row_order", "hilbert_keys", "locality_launch", "block_span", "bounding_square"]

CURVE_ORDER = 16
LAST_KEY = 0xFFFFFFFF


def locality_launch(n):
    """``(grid, items_per_wg, iters)`` of the key kernel and of every sort pass over ``n`` rows
    (host only)."""
    g, p, it = C.c_int32(), C.c_int32(), C.c_int32()
    L.check(L.lib().msw_locality_launch(int(n), C.byref(g), C.byref(p), C.byref(it)))
    return g.value, p.value, it.value


def _hilbert_index(ix, iy, order=CURVE_ORDER):
    """The index of cell (ix, iy) on the Hilbert curve of ``order`` bits a side (int64 arrays): the
    bit loop of csrc/locality.hip, vectorised."""
    x, y = np.array(ix, dtype=np.int64), np.array(iy, dtype=np.int64)
    d = np.zeros(x.shape, dtype=np.int64)
    last = (1 << order) - 1
    s = 1 << (order - 1)
    while s > 0:
        rx, ry = (x & s) != 0, (y & s) != 0
        d += s * s * ((3 * rx.astype(np.int64)) ^ ry.astype(np.int64))
        flip = ~ry & rx
        x, y = np.where(flip, last - x, x), np.where(flip, last - y, y)
        x, y = np.where(~ry, y, x), np.where(~ry, x, y)
        s >>= 1
    return d


def _keys_numpy(xy, box):
    """uint32 keys [n] of ``xy`` float64 [n, 2] in the box ``(x0, y0, side)``: the kernel's float64
    operations one by one, then the curve; a non-finite coordinate gives the last key."""
    xy = np.asarray(xy, dtype=np.float64).reshape(-1, 2)
    x0, y0, side = (np.float64(v) for v in box)
    with np.errstate(all="ignore"):
        sc = np.float64(65536.0) / side
        cells = []
        for v, lo in ((xy[:, 0], x0), (xy[:, 1], y0)):
            f = (v - lo) * sc
            inside = np.floor(np.where(np.isfinite(f) & (f >= 0) & (f < 65536.0), f, 0.0)).astype(np.int64)
            cells.append(np.where(f < 0, 0, np.where(f >= 65536.0, 65535, inside)))
    keys = _hilbert_index(cells[0], cells[1])
    keys = np.where(np.isfinite(xy).all(1), keys, LAST_KEY)
    return keys.astype(np.uint32)


def _check_box(box):
    x0, y0, side = (float(v) for v in box)
    with np.errstate(all="ignore"):
        ok = np.isfinite([x0, y0, side]).all() and side > 0 and np.isfinite(np.float64(65536.0) / np.float64(side))
    if not ok:
        raise ValueError("box must be finite (x0, y0, side) with side > 0 and 65536 / side finite")
    return x0, y0, side


def _xy_tensor(xy, device):
    t = xy if torch.is_tensor(xy) else torch.from_numpy(np.ascontiguousarray(np.asarray(xy), dtype=np.float64))
    if t.dim() != 2 or t.shape[1] != 2:
        raise ValueError("coordinates must be [n, 2]")
    return t.to(device, torch.float64).contiguous()


def _device(device, like=None):
    if device is None:
        device = like.device if torch.is_tensor(like) else "cpu"
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    return device


def hilbert_keys(xy, box, device=None):
    """The Hilbert keys of ``xy`` [n, 2] in ``box = (x0, y0, side)`` -> int64 [n] (values below
    2^32) on ``device`` (default: where ``xy`` lives).  A GPU runs ``k_hilbert_keys``."""
    device = _device(device, xy)
    box = _check_box(box)
    pts = _xy_tensor(xy, device)
    n = pts.shape[0]
    if device.type != "cuda":
        return torch.from_numpy(_keys_numpy(pts.numpy(), box).astype(np.int64))
    with torch.cuda.device(device):
        keys = torch.empty(n, dtype=torch.int32, device=device)
        st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        L.check(L.lib().msw_hilbert_keys(C.c_void_p(pts.data_ptr()), n, *box, C.c_void_p(keys.data_ptr()), st))
    return keys.to(torch.int64) & LAST_KEY


def bounding_square(xy):
    """``(x0, y0, side)``: the bounding square of the finite rows of ``xy`` [n, 2], anchored at
    their minimum; (0, 0, 1) when there is none, side 1 when they coincide (or lie so close that
    65536 / side overflows)."""
    xy = xy if torch.is_tensor(xy) else torch.from_numpy(np.asarray(xy, dtype=np.float64))
    ok = torch.isfinite(xy).all(1)
    if not bool(ok.any()):
        return 0.0, 0.0, 1.0
    pts = xy[ok]
    lo, hi = pts.min(0).values.tolist(), pts.max(0).values.tolist()
    side = max(hi[0] - lo[0], hi[1] - lo[1])
    with np.errstate(all="ignore"):
        usable = side > 0 and np.isfinite(side) and np.isfinite(np.float64(65536.0) / np.float64(side))
    return lo[0], lo[1], side if usable else 1.0


def _segments(graph):
    """-> (seg_ptr int64 [nseg + 1] tiling [0, N), graph index of each segment)."""
    N = int(graph.x.shape[0])
    if "node_ptr" not in graph.keys():
        return np.array([0, N], np.int64), np.zeros(1, np.int64)
    ptr = graph.node_ptr.detach().cpu().numpy().astype(np.int64)
    ptr = ptr.reshape(1, -1) if ptr.ndim == 1 else ptr
    starts, ends = ptr[:, :-1].reshape(-1), ptr[:, 1:].reshape(-1)
    owner = np.repeat(np.arange(ptr.shape[0]), ptr.shape[1] - 1)
    by_start = np.lexsort((ends, starts))  # an empty range sorts before the range that starts where it does
    starts, ends, owner = starts[by_start], ends[by_start], owner[by_start]
    if starts[0] != 0 or ends[-1] != N or (starts[1:] != ends[:-1]).any() or (ends < starts).any():
        raise ValueError("node_ptr does not tile [0, N)")
    return np.append(starts, N).astype(np.int64), owner


def row_order(graph, row_xy, device=None, stats=None):
    """The locality order of ``graph``'s rows -> int64 [N] on the CPU, for ``graph.row_order``.

    ``row_xy``: float64 [N, 2], one coordinate per graph row (``MeshGraph.row_xy``: face centroids,
    a ghost at its BC face's).  The segments are the ranges of ``graph.node_ptr`` (``[S+1]`` or, for
    a collated batch, ``[G, S+1]``; a graph without it is one segment).  All scales of one graph
    share the bounding square of that graph's finite coordinates.  Inside a segment the rows ascend
    by Hilbert key, ties to the lower row; rows with a non-finite coordinate come last.
    ``device`` (default: where ``row_xy`` lives): a GPU runs ``msw_locality_order``, the CPU the numpy
    restatement.  ``stats``: a dict that receives ``msw_locality_stats`` of a GPU run."""
    device = _device(device, row_xy)
    N = int(graph.x.shape[0])
    pts = _xy_tensor(row_xy, device)
    if pts.shape[0] != N:
        raise ValueError(f"row_xy holds {pts.shape[0]} rows, the graph {N}")
    seg_ptr, owner = _segments(graph)
    nseg = len(owner)
    per_graph = {}
    for g in np.unique(owner):
        mine = [pts[seg_ptr[j]:seg_ptr[j + 1]] for j in range(nseg) if owner[j] == g]
        per_graph[int(g)] = bounding_square(torch.cat(mine))
    boxes = np.ascontiguousarray([per_graph[int(g)] for g in owner], dtype=np.float64)
    if device.type != "cuda":
        xy = pts.numpy()
        out = np.empty(N, np.int64)
        for j in range(nseg):
            a, b = int(seg_ptr[j]), int(seg_ptr[j + 1])
            out[a:b] = a + np.argsort(_keys_numpy(xy[a:b], boxes[j]), kind="stable")
        return torch.from_numpy(out)
    with torch.cuda.device(device):
        order = torch.empty(N, dtype=torch.int32, device=device)
        st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        s = L.MswLocalityStats()
        L.check(L.lib().msw_locality_order(C.c_void_p(pts.data_ptr()), N, seg_ptr.ctypes.data_as(L.c_int64_p), nseg,
                                           boxes.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(order.data_ptr()),
                                           device.index, st, C.byref(s)))
    if stats is not None:
        stats.update({k: getattr(s, k) for k, _ in L.MswLocalityStats._fields_})
    return order.cpu().to(torch.int64)


def block_span(graph, row_order=None, scale=0, block=64, group=16):
    """The figure of merit of a row order: over the dual edges of ``scale`` (of the first graph),
    the mean number of distinct ``block``-row source blocks that one group of ``group`` consecutive
    destination rows touches, rows counted in laid-out order (``row_order``: int64 [N] as
    :func:`row_order` returns, or any order of the scale's rows; None: the graph's numbering).
    Plain numpy."""
    N = int(graph.x.shape[0])
    if "node_ptr" in graph.keys():
        ptr = graph.node_ptr.detach().cpu().numpy().astype(np.int64).reshape(-1, graph.node_ptr.shape[-1])[0]
        eptr = graph.edge_ptr.detach().cpu().numpy().astype(np.int64).reshape(-1)
        a, b, e0, e1 = int(ptr[scale]), int(ptr[scale + 1]), int(eptr[scale]), int(eptr[scale + 1])
    else:
        a, b, e0, e1 = 0, N, 0, int(graph.edge_index.shape[1])
    ei = graph.edge_index.detach().cpu().numpy().astype(np.int64)[:, e0:e1]
    keep = (ei[0] >= a) & (ei[0] < b) & (ei[1] >= a) & (ei[1] < b)
    src, dst = ei[0][keep], ei[1][keep]
    pos = np.full(N, -1, np.int64)  # laid-out position of every row of the scale
    if row_order is None:
        pos[a:b] = np.arange(b - a)
    else:
        ro = np.asarray(row_order.detach().cpu().numpy() if torch.is_tensor(row_order) else row_order, np.int64)
        ro = ro[(ro >= a) & (ro < b)]
        if len(ro) != b - a:
            raise ValueError("row_order does not hold every row of the scale once")
        pos[ro] = np.arange(b - a)
    pairs = np.unique(np.stack([pos[dst] // group, pos[src] // block], 1), axis=0)
    groups = (b - a + group - 1) // group
    return float(len(pairs)) / max(groups, 1)
