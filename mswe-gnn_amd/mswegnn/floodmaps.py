"""On-device flood maps and chunked rollouts (C ABI ``msw_flood_maps_update``).

What a forecaster takes away from a run is hazard maps, not the ``[N, 2, T]`` rollout.  The
reference builds them on the host after every rollout: flood-arrival time (``WD_to_FAT``,
utils/miscellaneous.py:56-68, used at utils/visualization.py:672-673), peak depth and discharge
(utils/visualization.py:592-598), velocity and Froude number (``get_velocity`` / ``get_Froude``,
utils/miscellaneous.py:44-54, used at utils/visualization.py:864-867).  Here one streaming HIP
kernel reads every rollout value once and reduces it over time into per-cell maps, with
carry-over state: :class:`FloodMaps` can be fed a rollout piece by piece, and
:func:`rollout_chunks` runs a rollout piece by piece, so a long horizon is reduced to maps
without ever being held whole (:func:`rollout_flood_maps`).

On CPU tensors the same interface runs :func:`_maps_torch`, a plain torch restatement of the
reference's functions (and the yardstick of the kernel's tests).
"""
from __future__ import annotations

import copy
import ctypes as C

import torch

from . import _lib as L

__all__ = ["MAP_NAMES", "FloodMaps", "flood_maps", "rollout_chunks", "rollout_flood_maps"]

MAP_NAMES = ("h_max", "t_h_max", "q_max", "t_q_max", "vel_max", "froude_max",
             "wet_steps", "first_wet", "last_wet")
_FLOAT_MAPS = ("h_max", "q_max", "vel_max", "froude_max")
_THR_MAPS = ("wet_steps", "first_wet", "last_wet")


def _first_where(mask, t_offset, none):
    """First step (global numbering) at which each row of ``mask`` [n, T] holds, else ``none``."""
    steps = torch.arange(mask.shape[1], dtype=torch.int32, device=mask.device) + t_offset
    big = torch.iinfo(torch.int32).max
    f = torch.where(mask, steps, torch.full_like(steps, big)).amin(1)
    return torch.where(f == big, torch.full_like(f, none), f)


def _last_where(mask, t_offset):
    steps = torch.arange(mask.shape[1], dtype=torch.int32, device=mask.device) + t_offset
    return torch.where(mask, steps, torch.full_like(steps, -1)).amax(1)


def _maps_torch(pred, thresholds=(0.05, 0.3), vel_eps=0.01, t_offset=0):
    """The maps of ``pred`` [n, 2, T] (T >= 1) from plain torch ops, one ``[n, T]`` pass each.
    Returns every map of MAP_NAMES; the threshold maps are ``[n_thr, n]``."""
    h = pred[:, 0, :]
    q = pred[:, 1, :].abs()                                   # visualization.py:597 abs(...)
    out = {}
    out["h_max"] = h.max(1).values                            # visualization.py:592 rollout[:,0,:].max()
    out["t_h_max"] = _first_where(h == out["h_max"][:, None], t_offset, -1)
    out["q_max"] = q.max(1).values                            # visualization.py:597 abs(rollout[:,1:,:]).max()
    out["t_q_max"] = _first_where(q == out["q_max"][:, None], t_offset, -1)
    vel = q / h                                               # get_velocity, miscellaneous.py:45
    vel[h <= vel_eps] = 0                                     # miscellaneous.py:46-47
    fr = vel / torch.sqrt(9.81 * h)                           # get_Froude, miscellaneous.py:51-52
    fr[h <= 0] = 0                                            # miscellaneous.py:53
    out["vel_max"] = vel.max(1).values                        # visualization.py:864-865, then its peak
    out["froude_max"] = fr.max(1).values                      # visualization.py:866-867, visualization.py:870
    wet, fst, lst = [], [], []
    for thr in thresholds:
        flooded = h > thr                                     # WD_to_FAT, miscellaneous.py:63
        wet.append(flooded.sum(1).to(torch.int32))            # miscellaneous.py:64 flooded_time
        fst.append(_first_where(flooded, t_offset, -1))
        lst.append(_last_where(flooded, t_offset))
    n = h.shape[0]
    empty = torch.zeros(0, n, dtype=torch.int32, device=pred.device)
    out["wet_steps"] = torch.stack(wet) if wet else empty
    out["first_wet"] = torch.stack(fst) if fst else empty
    out["last_wet"] = torch.stack(lst) if lst else empty
    return out


def _merge_torch(old, new):
    """Continue the maps ``old`` with those of later steps, ``new`` (the kernel's carry-over rule:
    a maximum moves only to a strictly larger value, first_wet is kept once set)."""
    out = {}
    for v, t in (("h_max", "t_h_max"), ("q_max", "t_q_max")):
        later = new[v] > old[v]
        out[v] = torch.where(later, new[v], old[v])
        out[t] = torch.where(later, new[t], old[t])
    for v in ("vel_max", "froude_max"):
        out[v] = torch.maximum(old[v], new[v])
    out["wet_steps"] = old["wet_steps"] + new["wet_steps"]
    out["first_wet"] = torch.where(old["first_wet"] >= 0, old["first_wet"], new["first_wet"])
    out["last_wet"] = torch.maximum(old["last_wet"], new["last_wet"])
    return out


class FloodMaps:
    """The flood maps of rows ``[row0, row0 + num_rows)`` of a rollout, accumulated over
    successive :meth:`update` calls.  ``want``: the maps to produce (names of MAP_NAMES, default
    all); the kernel skips the division and square root without ``vel_max`` / ``froude_max`` and
    the threshold work without a threshold map."""

    def __init__(self, num_rows, row0=0, thresholds=(0.05, 0.3), vel_eps=0.01, device="cpu", want=None):
        self.num_rows, self.row0 = int(num_rows), int(row0)
        self.thresholds = tuple(float(t) for t in thresholds)
        if len(self.thresholds) > L.MAX_MAP_THRESHOLDS:
            raise ValueError(f"at most {L.MAX_MAP_THRESHOLDS} thresholds")
        self.vel_eps = float(vel_eps)
        self.device = torch.device(device)
        self.want = tuple(MAP_NAMES if want is None else want)
        unknown = set(self.want) - set(MAP_NAMES)
        if unknown:
            raise ValueError(f"unknown maps {sorted(unknown)}; choose from {MAP_NAMES}")
        self.steps_seen = 0
        self.maps = {}
        for k in self.want:  # the first update overwrites them: no initialisation
            shape = (len(self.thresholds), self.num_rows) if k in _THR_MAPS else (self.num_rows,)
            self.maps[k] = torch.empty(shape, device=self.device,
                                       dtype=torch.float32 if k in _FLOAT_MAPS else torch.int32)

    def update(self, pred, t_begin=0, t_count=None, stream=None):
        """Reduce steps ``t_begin .. t_begin + t_count - 1`` of ``pred`` [N, 2, T] (graph
        numbering, N >= row0 + num_rows) into the maps; they follow the steps already seen."""
        if pred.dim() != 3 or pred.shape[1] != 2:
            raise ValueError("pred must be [N, 2, T]")
        T = int(pred.shape[2])
        t_begin = int(t_begin)
        t_count = T - t_begin if t_count is None else int(t_count)
        if t_begin < 0 or t_count < 0 or t_begin + t_count > T:
            raise ValueError(f"steps [{t_begin}, {t_begin + t_count}) lie outside the rollout's {T}")
        if pred.shape[0] < self.row0 + self.num_rows:
            raise ValueError(f"pred has {pred.shape[0]} rows, the maps cover rows up to {self.row0 + self.num_rows}")
        if pred.device != self.device:
            raise ValueError(f"pred is on {pred.device}, the maps on {self.device}")
        if t_count == 0 or self.num_rows == 0:
            return self
        if pred.is_cuda:
            self._update_hip(pred, T, t_begin, t_count, stream)
        else:
            rows = pred[self.row0:self.row0 + self.num_rows, :, t_begin:t_begin + t_count].float()
            new = _maps_torch(rows, self.thresholds, self.vel_eps, self.steps_seen)
            if self.steps_seen:
                full = dict(new)
                full.update(self.maps)  # maps not produced are not carried, as in the kernel
                new = _merge_torch(full, new)
            for k in self.want:
                self.maps[k] = new[k]
        self.steps_seen += t_count
        return self

    def _update_hip(self, pred, T, t_begin, t_count, stream):
        if pred.dtype != torch.float32 or not pred.is_contiguous():
            pred = pred.float().contiguous()
        m = L.MswFloodMaps(**{k: self.maps[k].data_ptr() for k in self.want})
        thr = (C.c_float * max(len(self.thresholds), 1))(*self.thresholds)
        st = C.c_void_p(stream if stream is not None else torch.cuda.current_stream(pred.device).cuda_stream)
        L.check(L.lib().msw_flood_maps_update(C.c_void_p(pred.data_ptr()), T, t_begin, t_count, self.steps_seen,
                                              self.row0, self.num_rows, thr, len(self.thresholds), self.vel_eps,
                                              int(self.steps_seen == 0), C.byref(m), st))

    def result(self, temporal_res=None, time_start=0):
        """The maps as a dict: ``h_max``, ``t_h_max``, ``q_max``, ``t_q_max``, ``vel_max``,
        ``froude_max`` [num_rows]; ``wet_steps``, ``first_wet``, ``last_wet`` as {threshold:
        [num_rows]} (steps count from 0 at the first step seen; -1 = never wet); ``steps``.
        With ``temporal_res`` (minutes per step) also, per threshold,
          fat_hours      the reference's flood-arrival map, WD_to_FAT(h, temporal_res, thr, time_start)
          arrival_hours  the time of the first wet step, NaN where the cell was never wet
        which agree on the cells that never dry again."""
        if not self.steps_seen:
            raise RuntimeError("no step has been reduced yet")
        out = {"steps": self.steps_seen}
        for k in self.want:
            if k in _THR_MAPS:
                out[k] = {t: self.maps[k][i] for i, t in enumerate(self.thresholds)}
            else:
                out[k] = self.maps[k]
        if temporal_res is not None:
            total_time = time_start + self.steps_seen                      # miscellaneous.py:61
            if "wet_steps" in self.maps:
                out["fat_hours"] = {}
                for t, flooded_time in out["wet_steps"].items():
                    fat = -(flooded_time.long() - total_time)              # miscellaneous.py:65
                    out["fat_hours"][t] = _over_60(fat * temporal_res)     # miscellaneous.py:66
            if "first_wet" in self.maps:
                out["arrival_hours"] = {}
                for t, f in out["first_wet"].items():
                    hours = _over_60((time_start + f.long()) * temporal_res)
                    out["arrival_hours"][t] = torch.where(f >= 0, hours, torch.full_like(hours, float("nan")))
        return out


def _over_60(minutes):
    """``minutes / 60`` as WD_to_FAT evaluates it on the CPU (miscellaneous.py:66: the dividend
    converted to float32, one correctly rounded division), on any device.  A GPU divides a tensor by
    a scalar as a product with the reciprocal, one ulp off for e.g. 600 / 60; the float64 quotient
    rounded once is the float32 quotient: p / 60 is exact or at least 1 / (60 * 2^25) (relative)
    from a float32 rounding boundary, far more than float64's error."""
    return (minutes.double() / 60).to(torch.result_type(minutes, 1.0))


def _split_kw(kw):
    res = {k: kw.pop(k) for k in ("temporal_res", "time_start") if k in kw}
    return kw, res


def _make(pred_rows, device, ranges, kw):
    rng = [(0, pred_rows)] if ranges is None else [(int(s), int(e)) for s, e in ranges]
    return [FloodMaps(e - s, s, device=device, **kw) for s, e in rng]


def flood_maps(pred, ranges=None, **kw):
    """The maps of a stored rollout ``pred`` [N, 2, T] in one shot -> ``FloodMaps.result``.
    ``ranges``: [(start, end)] row ranges -> a list with one result each (with
    ``mswegnn.metrics.finest_ranges(graph)``: one per simulation of a batch, finest scale only);
    default all rows -> one result.  Keywords: ``thresholds``, ``vel_eps``, ``want``
    (:class:`FloodMaps`), ``temporal_res``, ``time_start`` (:meth:`FloodMaps.result`)."""
    kw, res = _split_kw(dict(kw))
    out = [fm.update(pred).result(**res) for fm in _make(pred.shape[0], pred.device, ranges, kw)]
    return out[0] if ranges is None else out


def rollout_chunks(model, graph, steps=None, chunk=16):
    """``model.rollout(graph, steps)`` piece by piece: yields ``(t0, pred[:, :, t0:t0 + n])`` with
    n = ``chunk`` (the last piece may be shorter); the pieces concatenated equal the whole rollout
    bit for bit.  ``graph``: one graph, or a batch already passed through
    ``adapt_batch_training``.  Each piece is an ordinary ``model.rollout`` (HIP engine or torch
    path) of a shallow copy of the graph whose ``x`` holds the static columns followed by the last
    ``previous_t`` slots of [old window ; predictions], and whose ``BC`` is ``BC[:, :, t0:]``:
    every step overwrites all window slots of the BC cells before the forward, so the predictions
    determine the state.  Chunk lengths that are multiples of 16 keep the engine on its 16-step
    captured graphs."""
    T = int(graph.y.shape[-1] if steps is None else steps)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    dyn = int(model.previous_t) * 2
    x = graph.x
    n_static = x.shape[1] - dyn
    t0 = 0
    while t0 < T:
        n = min(chunk, T - t0)
        g = copy.copy(graph)
        g.x = x
        g.BC = graph.BC[:, :, t0:]
        pred = model.rollout(g, n)
        yield t0, pred
        t0 += n
        if t0 < T:
            # [old window ; predictions] as (h, q) pairs, oldest first; its last previous_t pairs
            # (a chunk shorter than previous_t keeps part of the old window)
            window = torch.cat((x[:, n_static:], pred.permute(0, 2, 1).reshape(x.shape[0], 2 * n).to(x.dtype)), 1)
            x = torch.cat((x[:, :n_static], window[:, window.shape[1] - dyn:]), 1)


def rollout_flood_maps(model, graph, steps=None, chunk=None, ranges=None, keep_rollout=False, **kw):
    """Roll out and reduce to flood maps -> the result(s) of :func:`flood_maps`.  ``chunk=None``:
    one ``model.rollout`` then one update; otherwise the rollout runs ``chunk`` steps at a time
    (:func:`rollout_chunks`) and never holds more than one piece.  ``keep_rollout=True`` returns
    ``(result, rollout)`` with the pieces concatenated (tests)."""
    kw, res = _split_kw(dict(kw))
    T = int(graph.y.shape[-1] if steps is None else steps)
    fms = _make(graph.x.shape[0], graph.x.device, ranges, kw)
    kept = []
    pieces = [(0, model.rollout(graph, T))] if chunk is None else rollout_chunks(model, graph, T, chunk)
    for _, pred in pieces:
        for fm in fms:
            fm.update(pred)
        if keep_rollout:
            kept.append(pred)
    out = [fm.result(**res) for fm in fms]
    out = out[0] if ranges is None else out
    return (out, torch.cat(kept, -1)) if keep_rollout else out
