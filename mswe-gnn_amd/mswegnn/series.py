"""On-device zone series (C ABI ``msw_zone_series_update``): a rollout reduced over space.

The flood maps (``mswegnn.floodmaps``) reduce a rollout over time into per-cell maps; this is the
other half, per-step series for regions.  A zone is an arbitrary list of graph rows -- a district,
a polder, a river reach, one simulation of a batch -- and a gauge is a zone of one row.  Per zone
and step one streaming HIP kernel produces the stored volume ``sum(area * h)`` (what the
reference's mass-conservation metric sums, training/loss.py:120-169), the flooded area and cell
count per depth threshold, and the largest depth and discharge.  The sums are fp64 and added in an
order that the zone's row list alone fixes, so a rollout fed piece by piece
(:func:`rollout_zone_series`, :func:`rollout_products`) gives the series of the whole bit for bit.

On CPU tensors the same interface runs :func:`_series_torch`, a plain torch restatement in float64
(and the yardstick of the kernel's tests).
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .floodmaps import FloodMaps, rollout_chunks
from .metrics import finest_ranges

__all__ = ["SERIES_NAMES", "Zones", "ZoneSeries", "zone_series", "rollout_zone_series", "rollout_products"]

SERIES_NAMES = ("volume", "wet_area", "wet_cells", "h_max", "q_max")
_THR_SERIES = ("wet_area", "wet_cells")
_DTYPES = {"volume": torch.float64, "wet_area": torch.float64, "wet_cells": torch.int32,
           "h_max": torch.float32, "q_max": torch.float32}


class Zones:
    """A set of zones over the rows of one graph / batch: zone z lists the graph rows
    ``rows[ptr[z]:ptr[z + 1]]`` (any order; a row may sit in several zones, or twice in one and
    then counts twice; a zone may be empty).  Sets over the same rows concatenate with ``+``, so
    one pass takes regions and gauges together.  On the GPU the object owns the ``msw_zones``
    handle (one per device, made on first use); :meth:`close` frees it."""

    def __init__(self, ptr, rows, num_rows):
        self.ptr = torch.as_tensor(ptr, dtype=torch.int64).reshape(-1).cpu().contiguous()
        self.rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1).cpu().to(torch.int32).contiguous()
        self.num_rows = int(num_rows)
        if self.ptr.numel() < 1 or int(self.ptr[0]) != 0 or bool((self.ptr[1:] < self.ptr[:-1]).any()) \
                or int(self.ptr[-1]) != self.rows.numel():
            raise ValueError("ptr must rise from 0 to the number of listed rows")
        if self.rows.numel() and (int(self.rows.min()) < 0 or int(self.rows.max()) >= self.num_rows):
            raise ValueError(f"row ids must lie in [0, {self.num_rows})")
        self._handles = {}
        self._lists = {}

    # ------------------------------------------------------------------ constructors
    @classmethod
    def from_lists(cls, lists, num_rows):
        """One zone per entry of ``lists`` (each a sequence / tensor of graph rows)."""
        lists = [torch.as_tensor(l, dtype=torch.int64).reshape(-1).cpu() for l in lists]
        ptr = torch.zeros(len(lists) + 1, dtype=torch.int64)
        if lists:
            ptr[1:] = torch.tensor([l.numel() for l in lists], dtype=torch.int64).cumsum(0)
        rows = torch.cat(lists) if lists else torch.zeros(0, dtype=torch.int64)
        return cls(ptr, rows, num_rows)

    @classmethod
    def from_labels(cls, labels, num_zones=None):
        """``labels`` [N] integers: the zone of every row, -1 = none.  Zones 0 .. max(labels) (or
        ``num_zones``), each listing its rows in ascending order."""
        labels = torch.as_tensor(labels).reshape(-1).cpu().to(torch.int64)
        if labels.numel() and int(labels.min()) < -1:
            raise ValueError("labels must be >= -1")
        Z = int(labels.max()) + 1 if labels.numel() else 0
        if num_zones is not None:
            if int(num_zones) < Z:
                raise ValueError(f"labels name {Z} zones, num_zones is {num_zones}")
            Z = int(num_zones)
        order = torch.argsort(labels, stable=True)
        order = order[labels[order] >= 0]
        ptr = torch.zeros(Z + 1, dtype=torch.int64)
        ptr[1:] = torch.bincount(labels[order], minlength=Z).cumsum(0)
        return cls(ptr, order, labels.numel())

    @classmethod
    def gauges(cls, rows, num_rows):
        """One zone per row of ``rows``."""
        rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1)
        return cls(torch.arange(rows.numel() + 1), rows, num_rows)

    @classmethod
    def finest(cls, graph):
        """One zone per simulation of a graph / batch: its finest-scale rows
        (``mswegnn.metrics.finest_ranges``)."""
        return cls.from_lists([torch.arange(s, e) for s, e in finest_ranges(graph)], graph.x.shape[0])

    def __add__(self, other):
        if not isinstance(other, Zones):
            return NotImplemented
        if other.num_rows != self.num_rows:
            raise ValueError("zone sets over different numbers of rows")
        return Zones(torch.cat((self.ptr, other.ptr[1:] + self.ptr[-1])), torch.cat((self.rows, other.rows)),
                     self.num_rows)

    # ------------------------------------------------------------------ views
    @property
    def num_zones(self):
        return self.ptr.numel() - 1

    @property
    def sizes(self):
        return self.ptr[1:] - self.ptr[:-1]

    def __len__(self):
        return self.num_zones

    def lists(self, device):
        """``(zone, row)`` of every list entry as int64 tensors on ``device`` (the torch path)."""
        device = torch.device(device)
        if device not in self._lists:
            zone = torch.repeat_interleave(torch.arange(self.num_zones), self.sizes)
            self._lists[device] = (zone.to(device), self.rows.to(device, torch.int64))
        return self._lists[device]

    # ------------------------------------------------------------------ the GPU handle
    def handle(self, device):
        """The ``msw_zones`` handle on GPU ``device`` (an index; -1: a host-only handle for launch
        queries), created on first use."""
        index = device if isinstance(device, int) else torch.device(device).index
        index = torch.cuda.current_device() if index is None else int(index)
        if index not in self._handles:
            out = C.c_void_p()
            rows = self.rows.numpy()
            ptr = self.ptr.numpy()
            L.check(L.lib().msw_zones_create(ptr.ctypes.data_as(L.c_int64_p), rows.ctypes.data_as(L.c_int32_p),
                                             self.num_zones, self.num_rows, index, C.byref(out)))
            self._handles[index] = out
        return self._handles[index]

    def launch(self, t_count, device=-1):
        """``(grid, units_per_wg, iters)`` of the update of a window of ``t_count`` steps."""
        g, u, it = C.c_int32(), C.c_int32(), C.c_int32()
        L.check(L.lib().msw_zone_series_launch(self.handle(device), int(t_count), C.byref(g), C.byref(u), C.byref(it)))
        return g.value, u.value, it.value

    def close(self):
        handles, self._handles = self._handles, {}
        for h in handles.values():
            L.lib().msw_zones_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass


def _series_torch(pred, zone, rows, num_zones, area=None, thresholds=(0.05, 0.3)):
    """The series of ``pred`` [N, 2, T] from plain torch ops: list entry i puts graph row
    ``rows[i]`` into zone ``zone[i]``.  Sums in float64 of exactly representable terms; comparisons
    and maxima on the float32 values.  Returns every series of SERIES_NAMES, the threshold series
    as ``[n_thr, Z, T]``."""
    T = pred.shape[2]
    dev = pred.device
    h = pred[rows, 0, :].float()
    q = pred[rows, 1, :].float().abs()
    a = torch.ones(rows.shape[0], dtype=torch.float64, device=dev) if area is None else area[rows].float().double()
    a = a[:, None].expand(-1, T)
    out = {}
    out["volume"] = torch.zeros(num_zones, T, dtype=torch.float64, device=dev).index_add_(0, zone, a * h.double())
    idx = zone[:, None].expand(-1, T)
    for k, v in (("h_max", h), ("q_max", q)):  # an empty zone keeps the 0
        out[k] = torch.zeros(num_zones, T, device=dev).scatter_reduce_(0, idx, v, "amax", include_self=False)
    wa, wc = [], []
    for thr in thresholds:
        wet = h > thr  # strict, float32 against the float32 threshold
        wa.append(torch.zeros(num_zones, T, dtype=torch.float64, device=dev)
                  .index_add_(0, zone, torch.where(wet, a, torch.zeros((), dtype=torch.float64, device=dev))))
        wc.append(torch.zeros(num_zones, T, dtype=torch.int32, device=dev).index_add_(0, zone, wet.to(torch.int32)))
    out["wet_area"] = torch.stack(wa) if wa else torch.zeros(0, num_zones, T, dtype=torch.float64, device=dev)
    out["wet_cells"] = torch.stack(wc) if wc else torch.zeros(0, num_zones, T, dtype=torch.int32, device=dev)
    return out


class ZoneSeries:
    """The series of ``zones`` over ``steps`` steps, filled column by column by successive
    :meth:`update` calls.  ``area``: [N] cell areas by graph row (``graph.area``), default 1 per
    cell; ``want``: the series to produce (names of SERIES_NAMES, default all)."""

    def __init__(self, zones, steps, area=None, thresholds=(0.05, 0.3), want=None, device="cpu"):
        self.zones, self.steps = zones, int(steps)
        self.thresholds = tuple(float(t) for t in thresholds)
        if len(self.thresholds) > L.MAX_MAP_THRESHOLDS:
            raise ValueError(f"at most {L.MAX_MAP_THRESHOLDS} thresholds")
        self.device = torch.device(device)
        self.want = tuple(SERIES_NAMES if want is None else want)
        unknown = set(self.want) - set(SERIES_NAMES)
        if unknown:
            raise ValueError(f"unknown series {sorted(unknown)}; choose from {SERIES_NAMES}")
        self.area = None
        if area is not None:
            self.area = torch.as_tensor(area).reshape(-1).to(self.device, torch.float32).contiguous()
            if self.area.shape[0] != zones.num_rows:
                raise ValueError("area must hold one value per graph row")
        zone, rows = zones.lists(self.device)
        a = torch.ones(rows.shape[0], dtype=torch.float64, device=self.device) if self.area is None \
            else self.area[rows].double()
        self.zone_area = torch.zeros(zones.num_zones, dtype=torch.float64, device=self.device).index_add_(0, zone, a)
        self.steps_seen = 0
        Z = zones.num_zones
        self.series = {}
        for k in self.want:  # every update overwrites its columns: no initialisation
            shape = (len(self.thresholds), Z, self.steps) if k in _THR_SERIES else (Z, self.steps)
            self.series[k] = torch.empty(shape, dtype=_DTYPES[k], device=self.device)

    def update(self, pred, t_begin=0, t_count=None, stream=None):
        """Reduce steps ``t_begin .. t_begin + t_count - 1`` of ``pred`` [N, 2, T] (graph
        numbering, N = the zone set's rows) into the next ``t_count`` columns."""
        if pred.dim() != 3 or pred.shape[1] != 2:
            raise ValueError("pred must be [N, 2, T]")
        T = int(pred.shape[2])
        t_begin = int(t_begin)
        t_count = T - t_begin if t_count is None else int(t_count)
        if t_begin < 0 or t_count < 0 or t_begin + t_count > T:
            raise ValueError(f"steps [{t_begin}, {t_begin + t_count}) lie outside the rollout's {T}")
        if pred.shape[0] != self.zones.num_rows:
            raise ValueError(f"pred has {pred.shape[0]} rows, the zones are over {self.zones.num_rows}")
        if pred.device != self.device:
            raise ValueError(f"pred is on {pred.device}, the series on {self.device}")
        if self.steps_seen + t_count > self.steps:
            raise ValueError(f"{self.steps_seen} + {t_count} steps exceed the {self.steps} the series hold")
        if t_count == 0 or self.zones.num_zones == 0:
            self.steps_seen += t_count
            return self
        if pred.is_cuda:
            self._update_hip(pred, T, t_begin, t_count, stream)
        else:
            zone, rows = self.zones.lists(self.device)
            new = _series_torch(pred[:, :, t_begin:t_begin + t_count], zone, rows, self.zones.num_zones,
                                self.area, self.thresholds)
            for k in self.want:
                self.series[k][..., self.steps_seen:self.steps_seen + t_count] = new[k]
        self.steps_seen += t_count
        return self

    def _update_hip(self, pred, T, t_begin, t_count, stream):
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            pred = pred.float().contiguous()
        out = L.MswZoneSeries(**{k: self.series[k].data_ptr() for k in self.want})
        thr = (C.c_float * max(len(self.thresholds), 1))(*self.thresholds)
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(pred.device).cuda_stream)
        L.check(L.lib().msw_zone_series_update(self.zones.handle(pred.device), C.c_void_p(pred.data_ptr()), T, t_begin,
                                               t_count, C.c_void_p(self.area.data_ptr() if self.area is not None else 0),
                                               thr, len(self.thresholds), self.steps, self.steps_seen, C.byref(out), st))

    def result(self):
        """The series of the steps seen so far as a dict: ``volume`` (float64), ``h_max``,
        ``q_max`` [Z, steps]; ``wet_area`` (float64), ``wet_cells`` as {threshold: [Z, steps]};
        ``zone_area`` [Z] (float64: the zone's summed cell area, its cell count without ``area``);
        ``h_mean`` = volume / zone_area in float64 (NaN for an empty zone); ``steps``."""
        n = self.steps_seen
        out = {"steps": n, "zone_area": self.zone_area}
        for k in self.want:
            v = self.series[k][..., :n]
            out[k] = {t: v[i] for i, t in enumerate(self.thresholds)} if k in _THR_SERIES else v
        if "volume" in self.series:
            out["h_mean"] = out["volume"] / self.zone_area[:, None]
        return out


def zone_series(pred, zones, **kw):
    """The series of a stored rollout ``pred`` [N, 2, T] in one shot -> ``ZoneSeries.result``.
    Keywords: ``area``, ``thresholds``, ``want`` (:class:`ZoneSeries`)."""
    return ZoneSeries(zones, pred.shape[2], device=pred.device, **kw).update(pred).result()


def rollout_products(model, graph, maps=None, series=None, steps=None, chunk=16):
    """Roll out ``chunk`` steps at a time (``rollout_chunks``; ``chunk=None``: one
    ``model.rollout``) and feed every piece to the :class:`FloodMaps` of ``maps`` (one, or a list)
    and to the :class:`ZoneSeries` ``series`` in the same pass: a long horizon yields both products
    without the rollout ever existing whole.  Returns ``(maps results, series result)``, the first
    shaped like ``maps``, ``None`` for a product not asked for."""
    T = int(graph.y.shape[-1] if steps is None else steps)
    fms = [] if maps is None else [maps] if isinstance(maps, FloodMaps) else list(maps)
    pieces = [(0, model.rollout(graph, T))] if chunk is None else rollout_chunks(model, graph, T, chunk)
    for _, pred in pieces:
        for fm in fms:
            fm.update(pred)
        if series is not None:
            series.update(pred)
    res = [fm.result() for fm in fms]
    return (None if maps is None else res[0] if isinstance(maps, FloodMaps) else res,
            None if series is None else series.result())


def rollout_zone_series(model, graph, zones, steps=None, chunk=None, **kw):
    """Roll out and reduce to zone series -> ``ZoneSeries.result``.  ``chunk=None``: one
    ``model.rollout`` then one update; otherwise the rollout runs ``chunk`` steps at a time and
    never holds more than one piece.  Keywords as :func:`zone_series`."""
    T = int(graph.y.shape[-1] if steps is None else steps)
    zs = ZoneSeries(zones, T, device=graph.x.device, **kw)
    return rollout_products(model, graph, series=zs, steps=T, chunk=chunk)[1]
